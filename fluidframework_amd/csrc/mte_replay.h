// mte_replay.h — the replay kernels.
//
//   pair_kernel  — pass 1: two documents per wavefront, E in {1, 2} (<= 126
//                  segments each).  The wave alternates between its two
//                  documents op by op, so all documents of a 10k-doc batch
//                  are resident on the chip at once (one wave per doc would
//                  need 10k resident waves; the chip holds 8 per SIMD).
//   big_kernel   — pass 2: one document per wavefront, E in {4, 8, 16}
//                  (<= 1022 segments), for documents pass 1 escalated.
//   stream_kernel — pass 3 (mte_stream.h): larger documents, HBM-resident.
//
// The tiers E >= 8 run the per-op step doc_step on a register-resident
// document: op records (32 B, mte_kernels.h) are read with scalar loads
// straight into SGPRs (the op index is wave-uniform), the next op's record in
// flight while the current op runs, and a vector load touches the records
// ahead so the scalar loads hit L2.  The pass-1 tiers run the per-slot-flag
// step (mte_step1.h): E <= 2 takes its records 64 at a time, one per lane,
// and decodes and window-checks them vector-wide (block_run); E = 4 fetches
// each op's record with a vector load (doc_step_v).
#pragma once

#include <type_traits>

#include "mte_kernels.h"

// Build-time knobs (tools/variants.sh builds A/B variants; defaults are the product build).
#ifndef MTE_PAIR_WAVES  // pass-1 waves per SIMD the register budget is sized for (5: 96 VGPRs, 4: 128)
#define MTE_PAIR_WAVES 5
#endif
#ifndef MTE_BURST
#define MTE_BURST 128
#endif
#ifndef MTE_PASS1_EMAX  // largest pass-1 register tier (4, or 2: documents over 126 segments go to pass 2)
#define MTE_PASS1_EMAX 4
#endif

namespace mte {

constexpr uint32_t kBurst = MTE_BURST;  // ops per burst in pass 1
constexpr int kStepVEmax = 4;           // tiers up to this E run the per-slot-flag step (doc_step_v), larger ones doc_step

// per-document replay state (wave-uniform); op cursors are 32-bit, relative
// to the document's first record of the batch
struct DocRun {
  int doc;
  int n;
  int32_t min_seq, cur_seq;
  int32_t status;
  uint32_t flags;
  bool running;
  const uint4* recp;  // the doc's first op record (2 x uint4 each)
  uint32_t k, k1;     // current op, end
};

__device__ __forceinline__ void fence_wave() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- scalar op fetch -------------------------------------------------------
// Records are read through the constant address space: the op index is
// wave-uniform, so the compiler emits s_load straight into SGPRs (no vector
// load, no readfirstlane) and tracks the lgkmcnt wait itself.  The records
// are never written while a replay kernel runs.
typedef int32_t s8v __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(4))) s8v* cs8p;

__device__ __forceinline__ s8v sload8(const uint4* p) { return *(cs8p)(const void*)p; }
// compiled propset `psi` (mte_kernels.h)
__device__ __forceinline__ s8v sload_props(const ReplayArgs& a, uint32_t psi) { return sload8(a.cps + 2 * psi); }

// L2 prefetch: lane l touches record `from + 4 l` (one 128-B line per lane,
// 256 records).  The loaded word is folded into `sink` one prefetch later, so
// the wait for it never stalls.
constexpr uint32_t kTouchSpan = 4 * kWave;
__device__ __forceinline__ void touch_records(const DocRun& D, uint32_t from, uint32_t& pending, uint32_t& sink) {
  sink ^= pending;
  const uint32_t r = from + 4u * (uint32_t)lane_id();
  pending = r < D.k1 + kRecPad ? reinterpret_cast<const uint32_t*>(D.recp + 2 * r)[0] : 0u;
}

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

template <int E, int NF, typename T>
__device__ __forceinline__ void shift_grab(uint32_t (&last)[NF], uint32_t (&last2)[NF], int f, const T (&F)[E]) {
  last[f] = (uint32_t)F[E - 1];
  last2[f] = (uint32_t)F[E >= 2 ? E - 2 : 0];
}

template <int E, int NF, typename T>
__device__ __forceinline__ void shift_apply(T (&F)[E], const uint32_t (&p1)[NF], const uint32_t (&p2)[NF], int f,
                                            const bool (&g1)[E], const bool (&g2)[E]) {
#pragma unroll
  for (int j = E - 1; j >= 0; j--) {
    const T m1 = (j >= 1) ? F[j >= 1 ? j - 1 : 0] : (T)p1[f];
    const T m2 = (j >= 2) ? F[j >= 2 ? j - 2 : 0] : ((j == 1) ? (T)p1[f] : (T)p2[f]);
    F[j] = g2[j] ? m2 : (g1[j] ? m1 : F[j]);
  }
}

// Shift every plane (and, for range ops, the L / P planes): new[i] =
// old[i - d(i)] with d(i) = (i > t1) + (i > t2), as pull_shift does for one
// plane.  The cross-lane moves of all planes are issued first and the selects
// after, so no DPP read waits on the VALU write just before it (a chained
// move per plane costs two hazard nops each).  For the tiers of doc_step
// (E > 1; shift_v, mte_step1.h, is the same shift on per-slot flags).
template <int E, int K, bool LP>
__device__ __forceinline__ void shift_all(Regs<E, K>& R, int32_t (&L)[E], int32_t (&P)[E], int t1, int t2) {
  static_assert(E >= 2, "one slot per lane shifts with ds_bpermute (shift_v)");
  constexpr int NF = kFieldPlanes + kRegPlanes<K> + (LP ? 2 : 0);
  uint32_t last[NF], last2[NF];
  shift_grab<E, NF>(last, last2, 0, R.len);
  shift_grab<E, NF>(last, last2, 1, R.seq);
  shift_grab<E, NF>(last, last2, 2, R.rseq);
  shift_grab<E, NF>(last, last2, 3, R.rmask);
  shift_grab<E, NF>(last, last2, 4, R.meta);
  shift_grab<E, NF>(last, last2, 5, R.toff);
#pragma unroll
  for (int k = 0; k < kRegPlanes<K>; k++) shift_grab<E, NF>(last, last2, kFieldPlanes + k, R.pr[k]);
  if constexpr (LP) {
    shift_grab<E, NF>(last, last2, NF - 2, L);
    shift_grab<E, NF>(last, last2, NF - 1, P);
  }
  uint32_t p1[NF], p2[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) p1[f] = (uint32_t)lane_prev((int32_t)last[f]);  // old[base - 1]
#pragma unroll
  for (int f = 0; f < NF; f++) p2[f] = (uint32_t)lane_prev((int32_t)last2[f]);  // old[base - 2]
  const int base = lane_id() * E;
  bool g1[E], g2[E];
#pragma unroll
  for (int j = 0; j < E; j++) {
    g1[j] = base + j > t1;
    g2[j] = base + j > t2;
  }
  shift_apply<E, NF>(R.len, p1, p2, 0, g1, g2);
  shift_apply<E, NF>(R.seq, p1, p2, 1, g1, g2);
  shift_apply<E, NF>(R.rseq, p1, p2, 2, g1, g2);
  shift_apply<E, NF>(R.rmask, p1, p2, 3, g1, g2);
  shift_apply<E, NF>(R.meta, p1, p2, 4, g1, g2);
  shift_apply<E, NF>(R.toff, p1, p2, 5, g1, g2);
#pragma unroll
  for (int k = 0; k < kRegPlanes<K>; k++) shift_apply<E, NF>(R.pr[k], p1, p2, kFieldPlanes + k, g1, g2);
  if constexpr (LP) {
    shift_apply<E, NF>(L, p1, p2, NF - 2, g1, g2);
    shift_apply<E, NF>(P, p1, p2, NF - 1, g1, g2);
  }
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

// Statistics (mte_stats: the Client.measureOps-style accounting and the
// algorithmic byte count) are a compile-time option of the replay kernels:
// S = false drops every counter update from the per-op path.
#define MTE_STAT(...) \
  if constexpr (S) {    \
    __VA_ARGS__         \
  }

// The collab-window error of an applied op, checked in the reference's order:
// completeAndLogOp (client.ts:525-528), then updateSeqNumbers (937-945) ->
// setMinSeq (mergeTree.ts:1078-1084), which sets currentSeq before its asserts.
// The test and update around it stay written out at their four sites (doc_step,
// doc_step_v, ch_ops, tree_step): folded into a helper that returns error / 0 /
// "minSeq advanced", the code comes back as selects that the site tests again,
// and the register allocation of the whole op loop changes with it.
__device__ __forceinline__ int window_error(DocRun& D, bool live, bool end, int32_t s, int32_t msn) {
  if (live) {
    if (!(D.cur_seq < s)) return MTE_E_SEQ_ORDER;
    if (!(D.min_seq <= msn)) return MTE_E_MSN_ORDER;
  }
  if (end) {
    if (!(D.cur_seq <= s)) return MTE_E_SEQ_ORDER;
    D.cur_seq = s;
    if (!(msn <= s)) return MTE_E_MSN_GT_SEQ;
    if (!(D.min_seq <= msn)) return MTE_E_MSN_ORDER;
  }
  return MTE_E_STATE;  // unreachable: the caller saw a violation
}

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

// One op record of one document: Client.applyMsg -> applyRemoteOp ->
// insertSegments / markRangeRemoved / annotateRange -> updateSeqNumbers
// (client.ts:918-945).  Returns 0 (applied), 1 (re-pick the register tier
// before this op, or after a compaction that shrank the doc), or a negative
// MTE_E_* (the doc stops).
//
// Structure: a scalar decision phase (visibility lengths, prefix scan and the
// split / insert-slot lookups, then wave-uniform shift thresholds and split
// patches) followed by ONE vector apply phase shared by all op types, so the
// register state flows through a single path (no per-branch copies).
template <int E, int K, bool S>
__device__ __forceinline__ int doc_step(Regs<E, K>& R, DocRun& D, uint32_t (&st)[kNumStats], s8v& cur,
                                        const ReplayArgs& a, uint32_t* zlds, int emin) {
  const int l = lane_id();
  const int base = l * E;
  const int lim = kWave * E < (int)a.cap ? kWave * E : (int)a.cap;
  if (D.n + 2 > lim) return 1;
  if constexpr (S) {
    if (st[kStOps] >= (1u << 20)) return 1;
  }

  // ---- op record: words 0..7 were prefetched into `cur` -------------------
  const s8v op = cur;
  const uint4* rec = D.recp + 2 * D.k;
  // next op, in flight during this one; past a doc's last op this reads the
  // next doc's first record or the zeroed kRecPad tail (never used).  Scalar
  // loads complete out of order, so a wait for `op` is an lgkmcnt(0) that
  // would also wait for this prefetch: the empty asm takes `op` as an input
  // and hands the prefetch its address, so the wait lands before the issue.
  uint64_t next = reinterpret_cast<uint64_t>(rec + 2);
  asm volatile("" : "+s"(next) : "s"(op));
  cur = sload8(reinterpret_cast<const uint4*>(next));
  const uint32_t w3 = (uint32_t)op[3];
  const uint32_t type = w3 & 0xffu, c = (w3 >> 8) & 0xffu, flags = w3 >> 16;
  if (c >= MTE_MAX_CLIENTS) return MTE_E_CLIENT_RANGE;
  MTE_STAT(st[kStOps]++;)
  MTE_STAT(st[kStMaxSegs] = (uint32_t)D.n > st[kStMaxSegs] ? (uint32_t)D.n : st[kStMaxSegs];)
  const int32_t s = op[0];
  const int32_t msn = op[2];
  int n = D.n;

  if (type == MTE_OP_INSERT || type == MTE_OP_REMOVE || type == MTE_OP_ANNOTATE) {
    const bool ins = type == MTE_OP_INSERT;
    MTE_STAT(st[kStScanned] += (uint32_t)n;)
    const int32_t r = op[1];
    const int32_t pos1 = op[4], pos2 = op[5];
    int32_t L[E], P[E];
    leaf_lengths<E, K>(R, r, c + 1, (int)c, D.min_seq, (D.flags & MTE_DOC_NEW_LENGTH_CALC) != 0, L);
    const int32_t total = prefix<E>(L, P);

    // ---- scalar decisions ------------------------------------------------
    int t1 = INT32_MAX, t2 = INT32_MAX;  // shift thresholds (pull_shift)
    SplitPatch pa{-1, -1, 0, 0, 0u, 0}, pb{-1, -1, 0, 0, 0u, 0};
    int g = -1;  // slot of the new segment
    if (ins) {
      // Client.applyInsertOp -> MergeTree.insertSegments (client.ts:470-505,
      // mergeTree.ts:1394-1422): ensureIntervalBoundary, then insertingWalk
      const int32_t nlen = (flags & MTE_F_MARKER) ? 1 : pos2;  // markers have length 1
      int32_t off = 0;
      const int xs = find_split<E>(L, P, pos1, &off);
      if (xs >= 0) {
        pa.h = xs;
        pa.o = off;
        pa.len = bcast<E>(R.len, xs);
        pa.toff = bcast<E>(R.toff, xs);
        t1 = xs;
        if (nlen > 0) {  // [head][new][tail]
          t2 = xs + 1;
          g = xs + 1;
          pa.tl = xs + 2;
          MTE_STAT(st[kStWritten] += 3;)
        } else {
          pa.tl = xs + 1;
          MTE_STAT(st[kStWritten] += 2;)
        }
        n += 1;
      } else if (nlen > 0) {
        g = find_slot<E>(L, P, pos1);
        if (g < 0) {
          if (pos1 > total) return MTE_E_INSERT_FAILED;  // mergeTree.ts:1666-1672
          g = n;
        }
        t1 = g - 1;
        MTE_STAT(st[kStWritten] += 1;)
      }
      if (nlen > 0) n += 1;
    } else {
      // markRangeRemoved (mergeTree.ts:1908-2000) / annotateRange
      // (1864-1906): the two ensureIntervalBoundary calls, ordered by position
      const int32_t b1 = pos1 < pos2 ? pos1 : pos2, b2 = pos1 < pos2 ? pos2 : pos1;
      int32_t o1 = 0, o2 = 0;
      int x1 = find_split<E>(L, P, b1, &o1);
      int x2 = b2 != b1 ? find_split<E>(L, P, b2, &o2) : -1;
      int32_t bb1 = b1;
      if (x1 < 0) {
        x1 = x2;
        o1 = o2;
        bb1 = b2;
        x2 = -1;
      }
      if (x1 >= 0) {
        pa.h = x1;
        pa.tl = x1 + 1;
        pa.o = o1;
        pa.len = bcast<E>(R.len, x1);
        pa.toff = bcast<E>(R.toff, x1);
        pa.pos = bb1;
        t1 = x1;
        n += 1;
        MTE_STAT(st[kStWritten] += 2;)
        if (x2 >= 0) {
          // after the first split the second leaf sits at x2 + 1; when both
          // boundaries fall in one leaf it is the first split's tail
          const bool same = x2 == x1;
          pb.h = x2 + 1;
          pb.tl = x2 + 2;
          pb.o = same ? o2 - o1 : o2;
          pb.len = same ? pa.len - o1 : bcast<E>(R.len, x2);
          pb.toff = same ? pa.toff + (uint32_t)o1 : bcast<E>(R.toff, x2);
          pb.pos = b2;
          t2 = x2 + 1;
          n += 1;
          MTE_STAT(st[kStWritten] += 2;)
        }
      }
    }

    // ---- vector apply ----------------------------------------------------
    if (t1 != INT32_MAX) {
      if (ins) shift_all<E, K, false>(R, L, P, t1, t2);
      else shift_all<E, K, true>(R, L, P, t1, t2);
    }
#pragma unroll
    for (int pi = 0; pi < 2; pi++) {
      const SplitPatch& p = pi == 0 ? pa : pb;
      if (p.h >= 0) {
#pragma unroll
        for (int jj = 0; jj < E; jj++) {
          const bool hd = base + jj == p.h, tl = base + jj == p.tl;
          R.len[jj] = hd ? p.o : (tl ? p.len - p.o : R.len[jj]);
          R.toff[jj] = tl ? p.toff + (uint32_t)p.o : R.toff[jj];
          if (!ins) {
            L[jj] = hd ? p.o : (tl ? p.len - p.o : L[jj]);
            P[jj] = tl ? p.pos : P[jj];
          }
        }
      }
    }
    if (g >= 0) {
      // the new segment (mergeTree.ts:1599-1611, textSegment.ts:40-48,
      // mergeTreeNodes.ts:602-609)
      const bool marker = (flags & MTE_F_MARKER) != 0;
      const uint32_t meta = (c + 1u) | (marker ? (1u + (uint32_t)pos2) << 8 : 0u);
      const uint32_t toff = marker ? 0u : a.text_base + (uint32_t)op[6];
      const uint32_t psi = (uint32_t)op[7];
      uint32_t pr[kRP<K>][1];
      const bool one[1] = {true};
#pragma unroll
      for (int kk = 0; kk < kRP<K>; kk++) pr[kk][0] = 0;
      if (K > 0 && psi != MTE_NO_PROPS) {
        const s8v q2 = sload_props(a, psi);
        apply_props<1, K>(pr, one, (uint32_t)q2[0], (uint32_t)q2[1], (uint32_t)q2[2], psi, a);
        MTE_STAT(st[kStPwrites] += (uint32_t)q2[3];)
      }
      MTE_STAT(if (!marker) st[kStUnits] += (uint32_t)pos2;)
      const int32_t nlen = marker ? 1 : pos2;
#pragma unroll
      for (int jj = 0; jj < E; jj++) {
        const bool at = base + jj == g;
        R.len[jj] = at ? nlen : R.len[jj];
        R.seq[jj] = at ? s : R.seq[jj];
        R.rseq[jj] = at ? kNone : R.rseq[jj];
        R.rmask[jj] = at ? 0u : R.rmask[jj];
        R.meta[jj] = at ? meta : R.meta[jj];
        R.toff[jj] = at ? toff : R.toff[jj];
#pragma unroll
        for (int kk = 0; kk < kRegPlanes<K>; kk++) R.pr[kk][jj] = at ? pr[kk][0] : R.pr[kk][jj];
      }
    }
    if (!ins && pos2 != pos1) {
      // nodeMap (mergeTree.ts:2274-2330): after the splits no visible leaf
      // straddles start or end, so a leaf is in range iff start <= P < end
      bool in[E];
      uint32_t cnt = 0;
#pragma unroll
      for (int jj = 0; jj < E; jj++) {
        in[jj] = L[jj] > 0 && P[jj] >= pos1 && P[jj] < pos2;
        cnt += (uint32_t)__popcll(__ballot(in[jj]));
      }
      MTE_STAT(st[kStWritten] += cnt;)
      if (type == MTE_OP_REMOVE) {
        // markRemoved (mergeTree.ts:1924-1962): keep the earliest removedSeq,
        // add the client to removedClientIds
        const uint32_t bit = 1u << c;
#pragma unroll
        for (int jj = 0; jj < E; jj++) {
          R.rseq[jj] = (in[jj] && R.rseq[jj] == kNone) ? s : R.rseq[jj];
          R.rmask[jj] = in[jj] ? (R.rmask[jj] | bit) : R.rmask[jj];
        }
      } else if (cnt > 0) {
        // PropertiesManager.addProperties (segmentPropertiesManager.ts:63-151)
        const uint32_t psi = (uint32_t)op[6];
        const s8v q2 = sload_props(a, psi);
        if (flags & MTE_F_REWRITE) {
#pragma unroll
          for (int kk = 0; kk < kRegPlanes<K>; kk++)
#pragma unroll
            for (int jj = 0; jj < E; jj++) R.pr[kk][jj] = in[jj] ? 0u : R.pr[kk][jj];
          if constexpr (K == kPack4) {
            // the side key's value of a marker is in its toff register (load_regs)
            if (a.side_key < 4u) {
#pragma unroll
              for (int jj = 0; jj < E; jj++) R.toff[jj] = (in[jj] && (R.meta[jj] >> 8)) ? 0u : R.toff[jj];
            }
          }
        }
        apply_props<E, K>(R.pr, in, (uint32_t)q2[0], (uint32_t)q2[1], (uint32_t)q2[2], psi, a);
        MTE_STAT(st[kStPwrites] += cnt * (uint32_t)q2[3];)
      }
    }
  } else if (type != MTE_OP_NOOP) {
    return MTE_E_INVALID_ARG;
  }
  D.n = n;
  D.k++;

  // Client.completeAndLogOp (client.ts:525-528) and updateSeqNumbers
  // (client.ts:937-945) -> setMinSeq (mergeTree.ts:1077-1093): one combined
  // test on the fast path, the exact code (in the reference's order) after
  const bool live = type != MTE_OP_NOOP, end = (flags & MTE_F_MSG_END) != 0;
  const bool bad = (live & (s <= D.cur_seq)) | (end & (s < D.cur_seq)) | ((live | end) & (msn < D.min_seq)) |
                   (end & (msn > s));
  if (bad) return window_error(D, live, end, s, msn);
  if (end) {
    D.cur_seq = s;
    if (msn > D.min_seq) {
      D.min_seq = msn;
      const int n_new = zamboni_lds<E, K>(R, n, msn, zlds);
      if (n_new != n) {
        D.n = n_new;
        // drop to a smaller register tier once the doc fits in half of it
        if (E > emin && n_new + 2 + 16 <= 32 * E) return 1;
      }
    }
  }
  return 0;
}

}  // namespace mte

#include "mte_step1.h"

namespace mte {

__device__ __forceinline__ void run_init(DocRun& D, const ReplayArgs& a, int doc, bool escalated_only) {
  D.doc = doc;
  D.running = false;
  D.n = 0;
  D.status = 0;
  D.k = D.k1 = 0;
  if (doc < 0) return;
  const DocHdr h = a.hdr[doc];
  const uint64_t kb = a.op_off[doc];
  D.n = h.nseg;
  D.min_seq = h.min_seq;
  D.cur_seq = h.cur_seq;
  D.status = h.status;
  D.flags = h.flags;
  D.recp = a.recs + 2 * kb;
  D.k = h.resume;
  D.k1 = (uint32_t)(a.op_off[doc + 1] - kb);
  if (h.status != 0) return;
  if (escalated_only && !(h.flags & kHdrNeedsEsc)) return;
  D.flags &= ~kHdrNeedsEsc;
  D.running = D.k < D.k1;
}

// add the 32-bit per-doc counters into the doc's 64-bit stats in HBM
__device__ __forceinline__ void run_flush_stats(const DocRun& D, uint32_t (&st)[kNumStats], const ReplayArgs& a) {
  if (D.doc >= 0 && lane_id() == 0) {
    unsigned long long* sd = a.stats + (size_t)D.doc * kNumStats;
#pragma unroll
    for (int t = 0; t < kNumStats; t++) {
      if (t == kStMaxSegs) sd[t] = sd[t] > st[t] ? sd[t] : st[t];
      else sd[t] += st[t];
    }
  }
#pragma unroll
  for (int t = 0; t < kNumStats; t++) st[t] = 0;
}

__device__ __forceinline__ void run_finish(DocRun& D, const ReplayArgs& a) {
  if (D.doc < 0) return;
  if (lane_id() == 0) {
    DocHdr h;
    h.nseg = D.n;
    h.min_seq = D.min_seq;
    h.cur_seq = D.cur_seq;
    h.status = D.status;
    h.flags = D.flags;
    h.resume = D.k;
    h.pad0 = a.hdr[D.doc].pad0;  // MTE_DOC_ROUND_SYNC check state (round_sync_kernel)
    h.pad1 = a.hdr[D.doc].pad1;
    a.hdr[D.doc] = h;
  }
}

// One burst of up to `limit` ops of one document at register tier E: load
// its segments into VGPRs, replay, write them back.  Returns early when the
// document needs another tier or stops.
template <int E, int K, bool S>
__device__ __forceinline__ void burst_run(DocRun& D, const ReplayArgs& a, uint32_t* zlds, int emin, uint32_t limit) {
  Regs<E, K> R;
  uint32_t st[kNumStats] = {};
  if constexpr (E <= kStepVEmax) {
    // pass 1 reads `a` in place (args_in_place).  What every step reads of it
    // (side_key, cap) the compiler hoists out of the op loop itself;
    // text_base is first read under the step's insert branch and would be
    // loaded there, on every insert, so it is read once here
    const uint32_t text_base = a.text_base;
    asm volatile("" ::"s"(text_base));
    if constexpr (E <= kBlockEmax) {
      // likewise cps in the block tiers (pass 1 alone runs them): under the
      // insert and annotate branches it was a load, a wait and then the
      // dependent load of the set, on every insert with a set and every
      // annotate that marks something
      const uint4* const cps = a.cps;
      asm volatile("" ::"s"(cps));
    }
  }
  load_regs<E, K>(R, D, a);
  const uint32_t kend = D.k1 - D.k > limit ? D.k + limit : D.k1;
  s8v cur;
  uint32_t vcur;
  [[maybe_unused]] const uint32_t* vrec = nullptr;  // this lane's dword of the record in vcur
  if constexpr (E <= kBlockEmax) {
    // block decode (mte_step1.h): the records come 64 at a time, in block_run
  } else if constexpr (E <= kStepVEmax) {
    // the E = 4 tier reads op records through a vector load: dword i in lane
    // i < 8.  Its wait is on vmcnt, so the LDS traffic of an op (shift
    // permutes, zamboni) never waits for the next record as it does for a
    // scalar load in flight (SMEM and LDS share lgkmcnt, and SMEM returns out
    // of order, so any LDS wait becomes lgkmcnt(0)).  Every lane loads (lanes
    // >= 8 repeat lanes 0-7, the same cache line), so the load needs no change
    // of the exec mask around it; only lanes 0-7 are read.
    vrec = reinterpret_cast<const uint32_t*>(D.recp + 2 * D.k) + (lane_id() & 7);
    vcur = *vrec;
  } else {
    cur = sload8(D.recp + 2 * D.k);
  }
  uint32_t pending = 0, sink = 0;
  // L2 prefetch of the records: short bursts (pass 1) touch the span after
  // this burst once, at its start (the first burst its own span too); long
  // runs touch ahead every kTouchSpan / 2 ops
  const bool per_burst = limit <= kTouchSpan / 2;
  if (per_burst) touch_records(D, D.k == 0 ? 0u : D.k + limit, pending, sink);
  else touch_records(D, D.k + 16, pending, sink);
  if constexpr (E <= kBlockEmax) {
    // these tiers only run pass 1's short bursts, touched ahead once (above)
    const int rc = block_run<E, K, S>(R, D, st, a, zlds, emin, kend);
    if (rc < 0) {
      D.status = rc;
      D.running = false;
    }
  } else {
    for (;;) {
      if (!per_burst && (D.k & (kTouchSpan / 2 - 1)) == 0) touch_records(D, D.k + kTouchSpan / 2, pending, sink);
      int rc;
      if constexpr (E <= kStepVEmax) rc = doc_step_v<E, K, S>(R, D, st, vcur, vrec, a, zlds, emin);
      else rc = doc_step<E, K, S>(R, D, st, cur, a, zlds, emin);
      if (rc != 0) {
        if (rc < 0) {
          D.status = rc;
          D.running = false;
        }
        break;
      }
      if (D.k >= kend) break;
    }
  }
  if (D.k >= D.k1) D.running = false;
  store_regs<E, K>(R, D, a);
  if constexpr (S) run_flush_stats(D, st, a);
  sink ^= pending;
  if (sink == 0x9e3779b9u && D.doc < 0) a.stats[0] = sink;  // keeps the prefetch loads alive
}

// tier for the next burst in pass 1 (E <= 4, 254 segments); larger documents
// continue in pass 2
__device__ __forceinline__ int pick_pass1_tier(DocRun& D, uint32_t cap) {
  if (D.n + 2 > (int)cap) {
    D.status = MTE_E_CAPACITY;
    D.running = false;
    return 0;
  }
  if (D.n + 2 <= kWave) return 1;
  if (D.n + 2 <= 2 * kWave) return 2;
  if (MTE_PASS1_EMAX >= 4 && D.n + 2 <= 4 * kWave) return 4;
  D.flags |= kHdrNeedsEsc;  // continue in the big-doc pass
  D.running = false;
  return 0;
}

template <int K, bool S>
__device__ __forceinline__ void pass1_burst(DocRun& D, const ReplayArgs& a, uint32_t* zlds) {
  const int e = pick_pass1_tier(D, a.cap);
#if defined(MTE_ISA_STUDY)  // ISA inspection only: one tier
  if (e) burst_run<MTE_ISA_STUDY, K, S>(D, a, zlds, 1, kBurst);
#else
  if (e == 1) burst_run<1, K, S>(D, a, zlds, 1, kBurst);
  else if (e == 2) burst_run<2, K, S>(D, a, zlds, 1, kBurst);
  else if constexpr (MTE_PASS1_EMAX >= 4) {
    if (e == 4) burst_run<4, K, S>(D, a, zlds, 1, kBurst);
  }
#endif
}

// DocRun <-> a DocHdr image in LDS (pass 1 keeps both documents of a pair
// there between bursts, so only the running document's state occupies SGPRs)
__device__ __forceinline__ bool run_from_lds(DocRun& D, const DocHdr* hl, int doc, const ReplayArgs& a) {
  const uint4 h0 = reinterpret_cast<const uint4*>(hl)[0], h1 = reinterpret_cast<const uint4*>(hl)[1];
  D.doc = doc;
  D.n = uni((int32_t)h0.x);
  D.min_seq = uni((int32_t)h0.y);
  D.cur_seq = uni((int32_t)h0.z);
  D.status = uni((int32_t)h0.w);
  D.flags = uni(h1.x);
  D.k = uni(h1.y);
  const uint64_t kb = a.op_off[doc];
  D.recp = a.recs + 2 * kb;
  D.k1 = (uint32_t)(a.op_off[doc + 1] - kb);
  D.running = D.status == 0 && D.k < D.k1 && !(D.flags & kHdrNeedsEsc);
  return D.running;
}

__device__ __forceinline__ void run_to_lds(const DocRun& D, DocHdr* hl) {
  if (lane_id() == 0) {
    uint4* p = reinterpret_cast<uint4*>(hl);
    p[0] = make_uint4((uint32_t)D.n, (uint32_t)D.min_seq, (uint32_t)D.cur_seq, (uint32_t)D.status);
    reinterpret_cast<uint2*>(hl)[2] = make_uint2(D.flags, D.k);  // pad0 / pad1 kept
  }
  fence_wave();
}

// The kernel's ReplayArgs, read in place from the kernel argument segment (they
// are the kernel's first argument).  Taken by value, every field is loaded at
// the kernel's entry and then lives in an SGPR for the whole kernel, or in a
// spill lane, though the op loop reads four of them: with the scalar registers
// full, the loop's own values get spilled around them.  Through this reference
// each field is a scalar load where it is used (the pointer passes through an
// empty asm so the loads stay there), and burst_run reads the op loop's fields
// once, ahead of the loop.
__device__ __forceinline__ const ReplayArgs& args_in_place() {
  typedef const __attribute__((address_space(4))) ReplayArgs* kargp;
  uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
  asm("" : "+s"(p));
  return *(const ReplayArgs*)(kargp)p;
}

// pass 1: `a.group` documents per wavefront (1 when the batch fits the chip
// at one per wave), replayed in turn one burst each, so a 10k-document batch is
// resident on the chip at once with the register budget of one document
// (E <= 4); W = waves per SIMD the register budget is sized for.
//
// Fair issue between the waves sharing a SIMD: the SIMD arbiter favours the
// oldest wave, so with equal work per wave the youngest starves, then runs
// alone (latency-bound) at the end: measured on config 3 the pass-1 waves
// ended in five steps by dispatch order, 14.9 ms to 26.3 ms (tools/
// wave_clock.py).  After every burst the wave sets its priority (4 levels)
// from its progress against the schedule of the previous run, which keeps the
// waves of a SIMD abreast, so they finish together.
template <int K, bool S, int WPB, int W>
__global__ __launch_bounds__(WPB * kWave, W * 4 / WPB) void pair_kernel(ReplayArgs) {
  const ReplayArgs& a = args_in_place();
  __shared__ uint32_t zlds_all[WPB][kWave * 4];
  __shared__ DocHdr hl_all[WPB][kGroupMax];
  const int w = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int pair = (int)blockIdx.x * WPB + w;
  if (pair >= (int)a.n_pairs) return;
  if (a.wclock && lane_id() == 0) a.wclock[2 * pair] = __builtin_amdgcn_s_memrealtime();
  const int g = (int)a.group;
  DocHdr* hl = hl_all[w];
  uint32_t* zlds = zlds_all[w];
  uint32_t live = 0;  // bit t: document t still has ops to run in this pass
  uint32_t total = 0;  // ops of the group in this pass, and those left (for the issue priority)
  for (int t = 0; t < g; t++) {
    const int doc = (int)a.pair_docs[(uint32_t)g * (uint32_t)pair + (uint32_t)t];
    if (doc >= 0) {
      DocHdr h = a.hdr[doc];
      const bool rel = (h.flags & kHdrRel) != 0;  // the streamed pass's this batch
      if (!rel) h.flags &= ~kHdrNeedsEsc;
      if (lane_id() == 0) hl[t] = h;
      if (!rel) {
        live |= 1u << t;
        total += (uint32_t)(a.op_off[doc + 1] - a.op_off[doc]) - h.resume;
      }
    }
  }
  fence_wave();
  total = uni(total);
  uint32_t left = total;
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_setprio(2);
  // one burst per iteration, the documents in turn; a single copy of the
  // burst code serves them all (the document is a runtime index)
  for (int t = 0; live; t = (t + 1 == g) ? 0 : t + 1) {
    if (!(live & (1u << t))) continue;
    const int doc = (int)a.pair_docs[(uint32_t)g * (uint32_t)pair + (uint32_t)t];
    DocRun D;
    const uint32_t k0 = hl[t].resume;
    if (run_from_lds(D, &hl[t], doc, a)) pass1_burst<K, S>(D, a, zlds);
    run_to_lds(D, &hl[t]);
    if (!D.running) live &= ~(1u << t);
    const uint32_t ran = uni(hl[t].resume - k0);
    left -= ran;
    // against the schedule of the previous run (a.eta ticks for the whole
    // pass; a first run's is estimated from the batch, mte_run): behind it ->
    // higher priority
    if (a.eta) {
      const unsigned long long el = __builtin_amdgcn_s_memrealtime() - t_start;
      const unsigned long long mine = (unsigned long long)(total - left) * a.eta;  // done/total vs el/eta
      const unsigned long long sched = el * total;
      const unsigned long long band = (unsigned long long)total * a.eta / 32;
      if (mine + band < sched) __builtin_amdgcn_s_setprio(3);
      else if (mine < sched) __builtin_amdgcn_s_setprio(2);
      else if (mine < sched + band) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
  }
  if (lane_id() == 0) {
    for (int t = 0; t < g; t++) {
      const int doc = (int)a.pair_docs[(uint32_t)g * (uint32_t)pair + (uint32_t)t];
      if (doc >= 0) a.hdr[doc] = hl[t];  // resume = the op cursor
    }
    if (a.wclock) a.wclock[2 * pair + 1] = __builtin_amdgcn_s_memrealtime();
  }
}

// pass 2: one document per wavefront, for the documents pass 1 escalated
template <int K, bool S>
__global__ __launch_bounds__(256) void big_kernel(ReplayArgs a) {
  __shared__ uint32_t zlds_all[kDocsPerBlock][kWave * 16];
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int doc = (int)blockIdx.x * kDocsPerBlock + w;
  if (doc >= (int)a.n_docs) return;
  DocRun D;
  run_init(D, a, doc, true);
  if (!D.running && !(a.hdr[doc].flags & kHdrNeedsEsc)) return;  // untouched doc: leave the header alone
  if (D.flags & kHdrRel) {  // relative positions: on to the streamed pass
    D.flags |= kHdrNeedsEsc;
    D.running = false;
  }
  uint32_t* zlds = zlds_all[w];
  while (D.running) {
    const int n = D.n;
    if (n + 2 > (int)a.cap) {
      D.status = MTE_E_CAPACITY;
      break;
    }
    if (n + 2 > 16 * kWave) {  // beyond the register tiers: continue in pass 3 (mte_stream.h)
      D.flags |= kHdrNeedsEsc;
      break;
    }
    if (n + 2 <= 4 * kWave) burst_run<4, K, S>(D, a, zlds, 4, 1u << 19);
    else if (n + 2 <= 8 * kWave) burst_run<8, K, S>(D, a, zlds, 4, 1u << 19);
    else burst_run<16, K, S>(D, a, zlds, 4, 1u << 19);
  }
  run_finish(D, a);
}

}  // namespace mte
