// mte_regdoc.h — a document held in registers (Regs<E, K>, mte_kernels.h):
// property planes, load / store, the split patch and the LDS zamboni.  Layer
// above mte_docrun.h; included by the steps (mte_step1.h, mte_step8.h), the
// flat kernels (mte_replay.h, mte_stream.h) and the register tree (mte_tree.h).
#pragma once

#include "mte_kernels.h"
#include "mte_docrun.h"

namespace mte {

// ISegment.addProperties for a remote op (segmentPropertiesManager.ts:63-151):
// entries in order, value 0 (null) deletes.  The first two entries come with
// the compiled propset record; longer sets are read here.  Applied to the slots with
// sel[j] set (E slots per lane, K planes); no lambdas, so the register arrays
// never need an address.
template <int E>
__device__ __forceinline__ void set_one_plane(uint32_t (&p)[E], const bool (&sel)[E], uint32_t val) {
#pragma unroll
  for (int jj = 0; jj < E; jj++) {
    uint32_t x = sel[jj] ? val : p[jj];
    asm volatile("" : "+v"(x));  // keeps each case's selects distinct, so no case merging into p[key]
    p[jj] = x;
  }
}

template <int E, int K>
__device__ __forceinline__ void set_plane(uint32_t (&pr)[kRP<K>][E], const bool (&sel)[E], uint32_t key,
                                          uint32_t val) {
  // `key` is wave-uniform: one scalar branch picks the plane, so only that
  // plane's E selects issue (a branch-free form costs K x E selects, and a
  // `kk == key` test per plane gets folded into pr[key], a dynamic index that
  // would push the whole register file to scratch)
  switch (key) {
    case 0: if constexpr (K > 0) set_one_plane<E>(pr[K > 0 ? 0 : 0], sel, val); break;
    case 1: if constexpr (K > 1) set_one_plane<E>(pr[K > 1 ? 1 : 0], sel, val); break;
    case 2: if constexpr (K > 2) set_one_plane<E>(pr[K > 2 ? 2 : 0], sel, val); break;
    case 3: if constexpr (K > 3) set_one_plane<E>(pr[K > 3 ? 3 : 0], sel, val); break;
    case 4: if constexpr (K > 4) set_one_plane<E>(pr[K > 4 ? 4 : 0], sel, val); break;
    case 5: if constexpr (K > 5) set_one_plane<E>(pr[K > 5 ? 5 : 0], sel, val); break;
    case 6: if constexpr (K > 6) set_one_plane<E>(pr[K > 6 ? 6 : 0], sel, val); break;
    case 7: if constexpr (K > 7) set_one_plane<E>(pr[K > 7 ? 7 : 0], sel, val); break;
    default: break;
  }
}

template <int E, int K>
__device__ __forceinline__ void apply_props(uint32_t (&pr)[kRP<K>][E], const bool (&sel)[E], uint32_t pk,
                                            uint32_t v0, uint32_t v1, uint32_t psi, const ReplayArgs& a) {
  // the packed plane takes the whole set as one (keep, val) pair, folded by
  // props_kernel (seg_op_v, put_new_v)
  static_assert(K != kPack4, "kPack4 applies the compiled (keep, val) pair");
  const uint32_t k0 = pk & 0xffu, k1 = (pk >> 8) & 0xffu;
  if (k0 != kNoKey) set_plane<E, K>(pr, sel, k0, v0);
  if (k1 != kNoKey) set_plane<E, K>(pr, sel, k1, v1);
  if (pk >> 16) {
    const mte_propset ps = a.ps[psi];
    for (uint32_t t = 2; t < ps.count; t++) {
      const mte_prop p = a.pe[ps.first + t];
      if (p.key < a.n_keys) set_plane<E, K>(pr, sel, uni(p.key), uni(p.value));
    }
  }
}

// one plane of the zamboni stream compaction: scatter kept slots to their
// compacted index in LDS, gather back lane-major
template <int E, typename T>
__device__ __forceinline__ void compact_plane(T (&F)[E], const bool (&keep)[E], const int32_t (&dst)[E],
                                              uint32_t* zlds) {
  const int base = lane_id() * E;
#pragma unroll
  for (int jj = 0; jj < E; jj++)
    if (keep[jj]) zlds[dst[jj]] = (uint32_t)F[jj];
  fence_wave();
#pragma unroll
  for (int jj = 0; jj < E; jj++) F[jj] = (T)zlds[base + jj];
  fence_wave();
}

template <int E, int K>
__device__ __forceinline__ void load_regs(Regs<E, K>& R, const DocRun& D, const ReplayArgs& a) {
  const uint32_t* pl = a.planes + (uint64_t)D.doc * a.cap;
  const uint64_t st = a.stride;
  const int base = lane_id() * E;
#pragma unroll
  for (int j = 0; j < E; j++) {
    const int i = base + j;
    const bool v = i < D.n;
    const uint32_t x = (uint32_t)(v ? i : 0);
    R.len[j] = v ? (int32_t)pl[x] : 0;
    R.seq[j] = v ? (int32_t)pl[st + x] : 0;
    R.rseq[j] = v ? (int32_t)pl[2 * st + x] : kPad;
    R.rmask[j] = v ? pl[3 * st + x] : 0u;
    R.meta[j] = v ? pl[4 * st + x] : 0u;
    R.toff[j] = v ? pl[5 * st + x] : 0u;
    if constexpr (K == kPack4) {
      // the side key's value of a marker rides in its toff register
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t pv = v ? pl[(kFieldPlanes + k) * st + x] : 0u;
        if ((uint32_t)k == a.side_key) R.toff[j] = (R.meta[j] >> 8) ? pv : R.toff[j];
        else w |= pv << (8 * k);
      }
      R.pr[0][j] = w;
    } else {
#pragma unroll
      for (int k = 0; k < K; k++) R.pr[k][j] = v ? pl[(kFieldPlanes + k) * st + x] : 0u;
    }
  }
}

template <int E, int K>
__device__ __forceinline__ void store_regs(const Regs<E, K>& R, const DocRun& D, const ReplayArgs& a) {
  uint32_t* pl = a.planes + (uint64_t)D.doc * a.cap;
  const uint64_t st = a.stride;
  const int base = lane_id() * E;
#pragma unroll
  for (int j = 0; j < E; j++) {
    const int i = base + j;
    if (i < D.n) {
      const uint32_t x = (uint32_t)i;
      pl[x] = (uint32_t)R.len[j];
      pl[st + x] = (uint32_t)R.seq[j];
      pl[2 * st + x] = (uint32_t)R.rseq[j];
      pl[3 * st + x] = R.rmask[j];
      pl[4 * st + x] = R.meta[j];
      if constexpr (K == kPack4) {
        const bool mk = (R.meta[j] >> 8) != 0 && a.side_key < 4u;
        pl[5 * st + x] = mk ? 0u : R.toff[j];
#pragma unroll
        for (int k = 0; k < 4; k++)
          pl[(kFieldPlanes + k) * st + x] =
              (uint32_t)k == a.side_key ? (mk ? R.toff[j] : 0u) : (R.pr[0][j] >> (8 * k)) & 0xffu;
      } else {
        pl[5 * st + x] = R.toff[j];
#pragma unroll
        for (int k = 0; k < K; k++) pl[(kFieldPlanes + k) * st + x] = R.pr[k][j];
      }
    }
  }
}

// A split of one leaf, applied after the shift: the head keeps [0, o) at
// slot h, the tail [o, len) lands at slot tl with its text offset advanced.
struct SplitPatch {
  int h, tl;      // -1: none
  int32_t o, len; // offset, length of the leaf before the split
  uint32_t toff;  // text offset of the leaf before the split
  int32_t pos;    // document position of the tail (P of the tail slot)
};

// zamboni of a register-resident document at E > 1 slots per lane: drop the
// tombstones with removedSeq <= msn (padding included) by a stream compaction
// staged through LDS.  Returns the new segment count (n: nothing dropped).
template <int E, int K>
__device__ __forceinline__ int zamboni_lds(Regs<E, K>& R, int n, int32_t msn, uint32_t* zlds) {
  bool keep[E];
  int32_t cntl = 0;
#pragma unroll
  for (int jj = 0; jj < E; jj++) {
    keep[jj] = R.rseq[jj] > msn;
    cntl += keep[jj] ? 1 : 0;
  }
  const int32_t incl = wave_incl_scan(cntl);
  const int n_new = rdlane(incl, kWave - 1);
  if (n_new != n) {
    int32_t dst[E];
    int32_t d0 = incl - cntl;
#pragma unroll
    for (int jj = 0; jj < E; jj++) {
      dst[jj] = d0;
      d0 += keep[jj] ? 1 : 0;
    }
    compact_plane<E>(R.len, keep, dst, zlds);
    compact_plane<E>(R.seq, keep, dst, zlds);
    compact_plane<E>(R.rseq, keep, dst, zlds);
    compact_plane<E>(R.rmask, keep, dst, zlds);
    compact_plane<E>(R.meta, keep, dst, zlds);
    compact_plane<E>(R.toff, keep, dst, zlds);
#pragma unroll
    for (int kk = 0; kk < kRegPlanes<K>; kk++) compact_plane<E>(R.pr[kk], keep, dst, zlds);
    const int base = lane_id() * E;
#pragma unroll
    for (int jj = 0; jj < E; jj++) {
      const bool pad = base + jj >= n_new;
      R.rseq[jj] = pad ? kPad : R.rseq[jj];
      R.len[jj] = pad ? 0 : R.len[jj];
    }
  }
  return n_new;
}

}  // namespace mte
