// pool_layout.h — pass 1's document pools: which flat documents a workgroup of
// pair_kernel (mte_replay.h) shares among its waves.  Host code only, no HIP:
// mte_load_docs (mte_engine.hip) lays the batch out with it, and
// tests/test_pass1_pools_layout.py compiles it alone with the host compiler.
//
// The rule.  The chip holds `resident` = CUs x 4 SIMDs x W pass-1 waves at
// once, in workgroups of `wpb` waves.
//   - A batch of at most `resident` flat documents runs one document per wave:
//     ceil(nf / wpb) pools of at most wpb documents.
//   - A larger batch gets one pool per resident workgroup (resident / wpb of
//     them), so every document is on the chip from the start and the waves of a
//     workgroup take turns on its documents, one burst at a time.
//   - A pool holds at most `pool_cap` documents (the LDS images of their
//     headers); a batch beyond resident / wpb x pool_cap gets ceil(nf /
//     pool_cap) pools, more workgroups than are resident at once.
// The flat documents are dealt to the pools in consecutive runs whose sizes
// differ by at most one: with q = nf / n_pools and r = nf % n_pools the first r
// pools take q + 1 documents and the others q.
#pragma once

#include <stdint.h>

#include <vector>

namespace mte {

struct PoolLayout {
  uint32_t n_pools = 0;
  uint32_t pool_max = 0;        // documents in the largest pool
  std::vector<uint32_t> first;  // pool p holds flat documents [first[p], first[p + 1]); n_pools + 1 entries
};

inline PoolLayout pool_layout(uint32_t nf, uint32_t cus, uint32_t waves_per_simd, uint32_t wpb, uint32_t pool_cap) {
  PoolLayout L;
  const uint64_t resident = (uint64_t)cus * 4 * waves_per_simd;
  uint64_t pools;
  if (nf <= resident) {
    pools = ((uint64_t)nf + wpb - 1) / wpb;
  } else {
    pools = resident / wpb;
    const uint64_t need = ((uint64_t)nf + pool_cap - 1) / pool_cap;
    if (pools < need) pools = need;
  }
  L.n_pools = (uint32_t)pools;
  L.first.assign((size_t)pools + 1, 0u);
  if (!pools) return L;
  const uint32_t q = (uint32_t)(nf / pools), r = (uint32_t)(nf % pools);
  for (uint32_t p = 0; p < L.n_pools; p++) L.first[p + 1] = L.first[p] + q + (p < r ? 1u : 0u);
  L.pool_max = q + (r ? 1u : 0u);
  return L;
}

}  // namespace mte
