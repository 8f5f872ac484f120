// mte_step8.h — the per-op step of the register tiers E >= 8 (doc_step) and
// its all-plane shift.  Layer above mte_regdoc.h, beside mte_step1.h; included
// by mte_replay.h alone (burst_run picks the step by tier).
#pragma once

#include "mte_kernels.h"
#include "mte_docrun.h"
#include "mte_regdoc.h"

namespace mte {

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
