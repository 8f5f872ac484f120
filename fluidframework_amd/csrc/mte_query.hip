// The batched queries (mte_query.h) in their own translation unit.
#include "mte_query.h"

namespace mte {

namespace {
inline uint32_t query_blocks(uint32_t n) { return (n + kQueriesPerBlock - 1) / kQueriesPerBlock; }
}  // namespace

hipError_t launch_find_tiles(const TileArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(find_tiles_kernel, dim3(query_blocks(a.n)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_text_count(const TextArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(text_count_kernel, dim3(query_blocks(a.n)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_text_gather(const TextArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(text_gather_kernel, dim3(query_blocks(a.n)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_props_at(const PosArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(props_at_kernel, dim3(query_blocks(a.n)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ref_positions(const RefArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ref_positions_kernel, dim3(query_blocks(a.n_tasks)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_segs_count(const SegsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(segs_count_kernel, dim3(query_blocks(a.n)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_segs_gather(const SegsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(segs_gather_kernel, dim3(query_blocks(a.n)), dim3(kQueriesPerBlock * kWave), 0, s, a);
  return hipGetLastError();
}

}  // namespace mte
