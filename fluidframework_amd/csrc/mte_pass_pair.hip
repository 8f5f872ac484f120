// Pass 1 of the flat replay (pair_kernel, mte_replay.h; its step, mte_step1.h)
// in its own translation unit: the unit has a compiler option of its own
// (PAIR_FLAGS, Makefile) that passes 2 and 3 (mte_pass_flat.hip) do not take.
#define MTE_PASS1_UNIT 1  // mte_step1.h: what is written for this unit's compile alone
#include "mte_passes.h"
#include "mte_replay.h"

namespace mte {

// Waves per SIMD an instantiation is built for: six (at most 80 VGPRs) where
// that costs it no scratch and no spilled VGPR, else five (96).  The plain
// K = 0 kernel and both K = 8 kernels spill at 80 (DESIGN.md §6 "Document
// pools" has the compiler's table of all eight at 5 and at 6).
template <int K, bool S>
constexpr int pair_waves() {
  return (K == 8 || (K == 0 && !S)) ? kPass1WavesMin : kPass1WavesMax;
}

template <int K, bool S>
hipError_t launch_pair(const ReplayArgs& a, uint32_t blocks, hipStream_t s) {
  hipLaunchKernelGGL((pair_kernel<K, S, kPairsPerBlock, pair_waves<K, S>()>), dim3(blocks),
                     dim3(kPairsPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

int pass1_waves(int K, bool S) {
  if (K == 0) return S ? pair_waves<0, true>() : pair_waves<0, false>();
  if (K == 8) return S ? pair_waves<8, true>() : pair_waves<8, false>();
  if (K == kPack4) return S ? pair_waves<kPack4, true>() : pair_waves<kPack4, false>();
  return S ? pair_waves<4, true>() : pair_waves<4, false>();
}

#define MTE_INST(K, S) template hipError_t launch_pair<K, S>(const ReplayArgs&, uint32_t, hipStream_t);
MTE_INST(0, false) MTE_INST(0, true) MTE_INST(4, false) MTE_INST(4, true) MTE_INST(8, false) MTE_INST(8, true)
// the four property planes packed into one register (kPack4)
MTE_INST(kPack4, false) MTE_INST(kPack4, true)
#undef MTE_INST

}  // namespace mte
