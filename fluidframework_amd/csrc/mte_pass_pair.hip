// Pass 1 of the flat replay (pair_kernel, mte_replay.h; its step, mte_step1.h)
// in its own translation unit: the unit has a compiler option of its own
// (PAIR_FLAGS, Makefile) that passes 2 and 3 (mte_pass_flat.hip) do not take.
#define MTE_PASS1_UNIT 1  // mte_step1.h: what is written for this unit's compile alone
#include "mte_passes.h"
#include "mte_replay.h"

namespace mte {

template <int K, bool S>
hipError_t launch_pair(const ReplayArgs& a, uint32_t blocks, hipStream_t s) {
  hipLaunchKernelGGL((pair_kernel<K, S, kPairsPerBlock, MTE_PAIR_WAVES>), dim3(blocks), dim3(kPairsPerBlock * kWave),
                     0, s, a);
  return hipGetLastError();
}

int pass1_waves() { return MTE_PAIR_WAVES; }

#define MTE_INST(K, S) template hipError_t launch_pair<K, S>(const ReplayArgs&, uint32_t, hipStream_t);
MTE_INST(0, false) MTE_INST(0, true) MTE_INST(4, false) MTE_INST(4, true) MTE_INST(8, false) MTE_INST(8, true)
// the four property planes packed into one register (kPack4)
MTE_INST(kPack4, false) MTE_INST(kPack4, true)
#undef MTE_INST

}  // namespace mte
