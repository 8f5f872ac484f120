// The batched queries (mte_query.h) in their own translation unit.
#include "mte_query.h"

namespace mte {

hipError_t launch_find_tiles(const TileArgs& a, hipStream_t s) {
  const uint32_t blocks = (a.n + kQueriesPerBlock - 1) / kQueriesPerBlock;
  hipLaunchKernelGGL(find_tiles_kernel, dim3(blocks), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

}  // namespace mte
