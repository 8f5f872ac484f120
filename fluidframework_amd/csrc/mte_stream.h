// mte_stream.h — pass 3: documents pass 2 escalated (> 1,022 segments) and
// new length-calc documents of remote clients with delta events, replayed
// one wavefront per document with the segment planes left in HBM and streamed
// per op in tiles of 128 slots (2 per lane, lane-major, coalesced; 2 per lane
// keeps the registers low enough for 5-8 waves per SIMD, which hide the
// per-op chain of L2 round trips better than wider tiles).
//
// Per op, the same algorithm as doc_step (mte_step8.h), restated over tiles:
//   A  scan tiles front to back: perspective lengths, running prefix, the
//      split / insert-slot lookups (stops once every target is found and the
//      prefix has passed the op's positions);
//   B  the split + insert shift as a back-to-front tiled move of every plane
//      (new[i] = old[i - d(i)], d(i) = (i > t1) + (i > t2)), then the split
//      patches and the new segment (single-lane stores);
//   C  for remove / annotate, a second front-to-back scan on the new layout
//      that marks the leaves with start <= P < end;
// and, when minSeq advances, a tiled stream compaction (zamboni).
// Loads bypass L1 (agent-scope relaxed atomics = sc1) and every phase ends
// with s_waitcnt vmcnt(0), so each phase reads what the previous one wrote.
// This path is bandwidth- and latency-bound by design (O(n) bytes per op); it
// exists so that no document size is refused below the ctx capacity.
#pragma once

#include "mte_passes.h"
#include "mte_docrun.h"
#include "mte_regdoc.h"
#include "mte_hbm.h"

namespace mte {

// One op of one HBM-resident document of remote clients (see the file
// comment).  Returns 0 or a negative MTE_E_*.  ev: its delta events
// (MTE_DOC_EVENTS docs).
template <int K, bool S>
__device__ int stream_step(DocRun& D, uint32_t (&st)[kNumStats], s8v& cur, const ReplayArgs& a, EvOut& ev) {
  constexpr int E = kTileE;
  const int l = lane_id();
  uint32_t* pl = a.planes + (uint64_t)D.doc * a.cap;
  const uint64_t sd = a.stride;
  const bool evd = (D.flags & MTE_DOC_EVENTS) != 0;
  ev.op = D.k;
  const int nplanes = kFieldPlanes + K;

  const s8v op = cur;
  const uint4* rec = D.recp + 2 * D.k;
  if (D.k + 1 < D.k1) cur = sload8(rec + 2);
  const uint32_t w3 = (uint32_t)op[3];
  const uint32_t type = w3 & 0xffu, c = (w3 >> 8) & 0xffu, flags = w3 >> 16;
  if (c >= MTE_MAX_CLIENTS) return MTE_E_CLIENT_RANGE;
  if (type == MTE_OP_RELPOS) {
    // the next record's positions, in its view (the engine checked that an
    // insert, remove or annotate of this document follows)
    if (D.k + 1 >= D.k1) return MTE_E_INVALID_ARG;
    const uint32_t nw3 = (uint32_t)cur[3];
    const uint32_t nt = nw3 & 0xffu, nc = (nw3 >> 8) & 0xffu;
    if (nt > MTE_OP_ANNOTATE || nc >= MTE_MAX_CLIENTS || ((nw3 >> 16) & MTE_F_LOCAL)) return MTE_E_INVALID_ARG;
    const bool newcalc = (D.flags & MTE_DOC_NEW_LENGTH_CALC) != 0;
    const uint32_t key = (uint32_t)op[6];
    if (flags & MTE_RP_POS1) {
      int32_t p = stream_marker_pos<K>(pl, sd, D.n, key, (uint32_t)op[4], cur[1], nc, D.min_seq, newcalc);
      if (p >= 0) p = (flags & MTE_RP_BEFORE1) ? p - op[0] : p + 1 + op[0];
      else if (nt == MTE_OP_INSERT) return MTE_E_UNSUPPORTED;
      cur[4] = p;
    }
    if ((flags & MTE_RP_POS2) && nt != MTE_OP_INSERT) {
      int32_t p = stream_marker_pos<K>(pl, sd, D.n, key, (uint32_t)op[5], cur[1], nc, D.min_seq, newcalc);
      if (p >= 0) p = (flags & MTE_RP_BEFORE2) ? p - op[1] : p + 1 + op[1];
      cur[5] = p;
    }
    D.k++;
    return 0;
  }
  // local ops, acks, rollbacks, regenerations and references belong to a
  // local client's document (the HBM tree pass)
  if (type == MTE_OP_REF || (flags & MTE_F_LOCAL) || type >= MTE_OP_ACK) return MTE_E_UNSUPPORTED;
  MTE_STAT(st[kStOps]++;)
  MTE_STAT(st[kStMaxSegs] = (uint32_t)D.n > st[kStMaxSegs] ? (uint32_t)D.n : st[kStMaxSegs];)
  const int32_t s = op[0], r = op[1], msn = op[2];
  const int32_t pos1 = op[4], pos2 = op[5];
  const bool ins = type == MTE_OP_INSERT;
  const bool marker = ins && (flags & MTE_F_MARKER) != 0;
  const int32_t nlen = marker ? 1 : pos2;  // insert: length of the new segment
  const bool rng = type == MTE_OP_REMOVE || type == MTE_OP_ANNOTATE;
  const bool newcalc = (D.flags & MTE_DOC_NEW_LENGTH_CALC) != 0;
  int n = D.n;

  if (ins || rng) {
    MTE_STAT(st[kStScanned] += (uint32_t)n;)
    // ---- A: scan -----------------------------------------------------------
    const int32_t b1 = ins ? pos1 : (pos1 < pos2 ? pos1 : pos2);
    const int32_t b2 = ins ? pos1 : (pos1 < pos2 ? pos2 : pos1);
    int xa = -1, xb = -1, gs = -1;  // split at b1, split at b2 (range only), first defined leaf with P >= pos
    int32_t oa = 0, ob = 0, lena = 0, lenb = 0;
    uint32_t toffa = 0, toffb = 0;
    int32_t carry = 0;
    bool complete = true;  // the scan reached the end of the document
    for (int tb = 0; tb < n; tb += kTile) {
      Regs<E, K> R;
      tile_load_hot<K>(R, pl, sd, tb, n);
      int32_t L[E], P[E];
      leaf_lengths<E, K>(R, r, c + 1, (int)c, D.min_seq, newcalc, L);
      const int32_t tot = prefix<E>(L, P);
#pragma unroll
      for (int j = 0; j < E; j++) P[j] += carry;
      if (xa < 0) {
        int32_t o = 0;
        const int x = find_split<E>(L, P, b1, &o);
        if (x >= 0) {
          xa = tb + x;
          oa = o;
          lena = bcast<E>(R.len, x);
          toffa = bcast<E>(R.toff, x);
        }
      }
      if (rng && b2 != b1 && xb < 0) {
        int32_t o = 0;
        const int x = find_split<E>(L, P, b2, &o);
        if (x >= 0) {
          xb = tb + x;
          ob = o;
          lenb = bcast<E>(R.len, x);
          toffb = bcast<E>(R.toff, x);
        }
      }
      if (ins && gs < 0) {
        const int x = find_slot<E>(L, P, pos1);
        if (x >= 0) gs = tb + x;
      }
      carry += tot;
      // every later leaf has P >= carry > both positions: nothing more to find
      if (carry > b2 && (!ins || gs >= 0 || xa >= 0) && tb + kTile < n) {
        complete = false;
        break;
      }
    }
    // ---- decisions (as doc_step) --------------------------------------------
    int t1 = INT32_MAX, t2 = INT32_MAX, g = -1;
    SplitPatch pa{-1, -1, 0, 0, 0u, 0}, pb{-1, -1, 0, 0, 0u, 0};
    if (ins) {
      if (xa >= 0) {
        pa = SplitPatch{xa, nlen > 0 ? xa + 2 : xa + 1, oa, lena, toffa, pos1};
        t1 = xa;
        if (nlen > 0) {
          t2 = xa + 1;
          g = xa + 1;
        }
        MTE_STAT(st[kStWritten] += nlen > 0 ? 3 : 2;)
        n += 1;
      } else if (nlen > 0) {
        g = gs;
        if (g < 0) {
          if (complete && pos1 > carry) return MTE_E_INSERT_FAILED;  // mergeTree.ts:1666-1672
          g = n;
        }
        t1 = g - 1;
        MTE_STAT(st[kStWritten] += 1;)
      }
      if (nlen > 0) n += 1;
    } else {
      int x1 = xa, x2 = xb;
      int32_t o1 = oa, o2 = ob, l1 = lena, l2 = lenb, bb1 = b1;
      uint32_t f1 = toffa, f2 = toffb;
      if (x1 < 0) {
        x1 = x2;
        o1 = o2;
        l1 = l2;
        f1 = f2;
        bb1 = b2;
        x2 = -1;
      }
      if (x1 >= 0) {
        pa = SplitPatch{x1, x1 + 1, o1, l1, f1, bb1};
        t1 = x1;
        n += 1;
        MTE_STAT(st[kStWritten] += 2;)
        if (x2 >= 0) {
          const bool same = x2 == x1;
          pb = SplitPatch{x2 + 1, x2 + 2, same ? o2 - o1 : o2, same ? l1 - o1 : l2, same ? f1 + (uint32_t)o1 : f2, b2};
          t2 = x2 + 1;
          n += 1;
          MTE_STAT(st[kStWritten] += 2;)
        }
      }
    }
    if (n + 2 > (int)a.cap) return MTE_E_CAPACITY;
    // ---- B: shift back to front, then patches and the new segment --------------
    if (t1 != INT32_MAX) {
      const int lo = t1 + 1;
      // back to front: a tile's sources lie in it or the tile below, which is
      // moved later, so a tile's planes move kPlaneGroup at a time: their loads
      // all in flight at once, then their stores
      for (int tb = ((n - 1) / kTile) * kTile; tb + kTile > lo; tb -= kTile) {
        const int base = tb + l * E;
#pragma nounroll
        for (int p0 = 0; p0 < nplanes; p0 += kPlaneGroup) {
          uint32_t v[kPlaneGroup][E];
#pragma unroll
          for (int g = 0; g < kPlaneGroup; g++) {
            // unconditional loads from a valid plane and slot, selected after
            const int pg = p0 + g < nplanes ? p0 + g : nplanes - 1;
            const uint32_t pb = (uint32_t)((uint64_t)pg * sd);
#pragma unroll
            for (int j = 0; j < E; j++) {
              const int i = base + j;
              const int src = i - ((i > t1 ? 1 : 0) + (i > t2 ? 1 : 0));
              // src is -1 only for the new segment's slot 0 (t1 == -1), which the
              // new-segment stores below overwrite: never read before the doc
              const bool ok = p0 + g < nplanes && i < n && i >= lo && MTE_SLOT_OK(src, a.cap);
              const uint32_t x = ld_l2o(pl, pb + (uint32_t)(ok ? src : 0));
              v[g][j] = ok ? x : 0u;
            }
          }
#pragma unroll
          for (int g = 0; g < kPlaneGroup; g++) {
            const uint32_t pb = (uint32_t)((uint64_t)(p0 + g) * sd);
#pragma unroll
            for (int j = 0; j < E; j++) {
              const int i = base + j;
              if (p0 + g < nplanes && i < n && i >= lo && MTE_SLOT_OK(i, a.cap)) pl[pb + (uint32_t)i] = v[g][j];
            }
          }
        }
      }
      vm_drain();
    }
    if ((pa.h >= 0 && !(MTE_SLOT_OK(pa.h, a.cap) && MTE_SLOT_OK(pa.tl, a.cap))) ||
        (pb.h >= 0 && !(MTE_SLOT_OK(pb.h, a.cap) && MTE_SLOT_OK(pb.tl, a.cap))) || (g >= 0 && !MTE_SLOT_OK(g, a.cap)))
      return MTE_E_STATE;
    if (l == 0) {
#pragma unroll
      for (int pi = 0; pi < 2; pi++) {
        const SplitPatch& p = pi == 0 ? pa : pb;
        if (p.h >= 0) {
          pl[p.h] = (uint32_t)p.o;
          pl[p.tl] = (uint32_t)(p.len - p.o);
          pl[5 * sd + p.tl] = p.toff + (uint32_t)p.o;
        }
      }
      if (g >= 0) {
        pl[g] = (uint32_t)nlen;
        pl[sd + g] = (uint32_t)s;
        pl[2 * sd + g] = (uint32_t)kNone;
        pl[3 * sd + g] = 0u;
        pl[4 * sd + g] = (c + 1u) | (marker ? (1u + (uint32_t)pos2) << 8 : 0u);
        pl[5 * sd + g] = marker ? 0u : a.text_base + (uint32_t)op[6];
      }
    }
    if (g >= 0) {
      uint32_t pr[K > 0 ? K : 1][1];
      const bool one[1] = {true};
#pragma unroll
      for (int kk = 0; kk < (K > 0 ? K : 1); kk++) pr[kk][0] = 0;
      const uint32_t psi = (uint32_t)op[7];
      if (K > 0 && psi != MTE_NO_PROPS) {
        const s8v q2 = sload_props(a, psi);
        apply_props<1, K>(pr, one, (uint32_t)q2[0], (uint32_t)q2[1], (uint32_t)q2[2], psi, a);
        MTE_STAT(st[kStPwrites] += (uint32_t)q2[3];)
      }
      if (l == 0) {
#pragma unroll
        for (int kk = 0; kk < K; kk++) pl[(kFieldPlanes + kk) * sd + g] = pr[kk][0];
      }
      MTE_STAT(if (!marker) st[kStUnits] += (uint32_t)pos2;)
    }
    vm_drain();
    if (evd && ins) {  // insertSegments' delta callback (mergeTree.ts:1409-1416)
      if (g >= 0) ev_one(ev, MTE_OP_INSERT, own_prefix(pl, sd, g), nlen);
      else if (nlen <= 0) ev_one(ev, MTE_OP_INSERT, -1, 0);  // a zero-length segment is never linked
    }
    // ---- C: mark [start, end) on the new layout ---------------------------------
    if (rng && pos2 > pos1) {
      s8v q2 = {0, 0, 0, 0, 0, 0, 0, 0};
      if (type == MTE_OP_ANNOTATE) q2 = sload_props(a, (uint32_t)op[6]);
      const bool rem = type == MTE_OP_REMOVE;
      int32_t cy = 0, ocy = 0;  // ocy: the own view's prefix after the op (events)
      uint32_t cnt_all = 0;
      for (int tb = 0; tb < n && cy < pos2; tb += kTile) {
        Regs<E, K> R;
        tile_load_hot<K>(R, pl, sd, tb, n);
        int32_t L[E], P[E];
        leaf_lengths<E, K>(R, r, c + 1, (int)c, D.min_seq, newcalc, L);
        const int32_t tot = prefix<E>(L, P);
        bool in[E];
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < E; j++) {
          P[j] += cy;
          in[j] = L[j] > 0 && P[j] >= pos1 && P[j] < pos2;
          cnt += (uint32_t)__popcll(__ballot(in[j]));
        }
        cy += tot;
        if (evd) {
          // markRangeRemoved reports the segments it newly removes, annotateRange
          // every one it visits (mergeTree.ts:1954-1959, 1893-1900), at their
          // positions in the own view after the op, in document order
          const bool rem0 = type == MTE_OP_REMOVE;
          bool evf[E];
          int32_t OL[E], OP[E];
#pragma unroll
          for (int j = 0; j < E; j++) {
            evf[j] = in[j] && (!rem0 || R.rseq[j] == kNone);
            const bool gone = rem0 && in[j];
            OL[j] = (R.rseq[j] == kNone && !gone) ? R.len[j] : 0;
          }
          const int32_t otot = prefix<E>(OL, OP);
          uint32_t ecnt = 0;
#pragma unroll
          for (int j = 0; j < E; j++) ecnt += evf[j] ? 1u : 0u;
          const int32_t eincl = wave_incl_scan((int32_t)ecnt);
          uint32_t e = ev.n + (uint32_t)(eincl - (int32_t)ecnt);
#pragma unroll
          for (int j = 0; j < E; j++) {
            if (evf[j]) {
              if (e < ev.cap) ev.p[e] = mte_delta{ev.op, type, ocy + OP[j], R.len[j], OL[j] == 0 ? 1u : 0u};
              e++;
            }
          }
          ev.n += (uint32_t)rdlane(eincl, kWave - 1);
          ocy += otot;
        }
        if (cnt == 0) continue;
        cnt_all += cnt;
        const int base = tb + l * E;
        if (rem) {
          // markRemoved (mergeTree.ts:1924-1962)
#pragma unroll
          for (int j = 0; j < E; j++) {
            if (in[j]) {
              // an earlier removedSeq stays; the remover joins the mask
              pl[2 * sd + base + j] = (uint32_t)(R.rseq[j] == kNone ? s : R.rseq[j]);
              pl[3 * sd + base + j] = R.rmask[j] | (1u << c);
            }
          }
        } else if (K > 0) {
          // PropertiesManager.addProperties (segmentPropertiesManager.ts:63-151)
          // loads unconditional (padding reads slot 0), padding selected away
          // after: no branch per load
          uint32_t pr[K > 0 ? K : 1][E];
#pragma unroll
          for (int kk = 0; kk < K; kk++)
#pragma unroll
            for (int j = 0; j < E; j++) {
              const int i = base + j;
              const uint32_t o = ld_l2(pl + (kFieldPlanes + kk) * sd + (i < n ? i : 0));
              pr[kk][j] = ((flags & MTE_F_REWRITE) && in[j]) ? 0u : (i < n ? o : 0u);
            }
          apply_props<E, K>(pr, in, (uint32_t)q2[0], (uint32_t)q2[1], (uint32_t)q2[2], (uint32_t)op[6], a);
#pragma unroll
          for (int kk = 0; kk < K; kk++)
#pragma unroll
            for (int j = 0; j < E; j++)
              if (in[j]) pl[(kFieldPlanes + kk) * sd + base + j] = pr[kk][j];
        }
      }
      MTE_STAT(st[kStWritten] += cnt_all;)
      if (type == MTE_OP_ANNOTATE) st[kStPwrites] += cnt_all * (uint32_t)q2[3];
      vm_drain();
    }
  }
  D.n = n;
  D.k++;

  if (type != MTE_OP_NOOP) {  // Client.completeAndLogOp (client.ts:525-528)
    if (!(D.cur_seq < s)) return MTE_E_SEQ_ORDER;
    if (!(D.min_seq <= msn)) return MTE_E_MSN_ORDER;
  }
  if (flags & MTE_F_MSG_END) {
    // updateSeqNumbers (client.ts:937-945) -> setMinSeq (mergeTree.ts:1077-1093)
    if (!(D.cur_seq <= s)) return MTE_E_SEQ_ORDER;
    D.cur_seq = s;
    if (!(msn <= s)) return MTE_E_MSN_GT_SEQ;
    if (!(D.min_seq <= msn)) return MTE_E_MSN_ORDER;
    if (msn > D.min_seq) {
      D.min_seq = msn;
      // zamboni as a tiled stream compaction, front to back (dst <= src)
      int32_t w = 0;
      for (int tb = 0; tb < n; tb += kTile) {
        const int base = tb + l * E;
        bool keep[E];
        int32_t cntl = 0;
#pragma unroll
        for (int j = 0; j < E; j++) {
          const int i = base + j;
          const int32_t rs = (int32_t)ld_l2(pl + 2 * sd + (i < n ? i : 0));  // unconditional, selected after
          keep[j] = i < n && rs > msn;
          cntl += keep[j] ? 1 : 0;
        }
        const int32_t incl = wave_incl_scan(cntl);
        const int32_t tot = rdlane(incl, kWave - 1);
        if (tot != kTile || w != tb) {
          int32_t dst = w + incl - cntl;
          // kPlaneGroup planes' loads in flight at once, then their stores (dst
          // <= src: a tile's stores land at or below it, after its own loads)
  #pragma nounroll
        for (int p0 = 0; p0 < nplanes; p0 += kPlaneGroup) {
            uint32_t v[kPlaneGroup][E];
#pragma unroll
            for (int g = 0; g < kPlaneGroup; g++) {
              const int pg = p0 + g < nplanes ? p0 + g : nplanes - 1;
              const uint32_t pb = (uint32_t)((uint64_t)pg * sd);
#pragma unroll
              for (int j = 0; j < E; j++) {
                const bool ok = p0 + g < nplanes && keep[j];  // keep implies base + j < n
                const uint32_t x = ld_l2o(pl, pb + (uint32_t)(ok ? base + j : 0));
                v[g][j] = ok ? x : 0u;
              }
            }
#pragma unroll
            for (int g = 0; g < kPlaneGroup; g++) {
              const uint32_t pb = (uint32_t)((uint64_t)(p0 + g) * sd);
              int32_t d0 = dst;
#pragma unroll
              for (int j = 0; j < E; j++) {
                if (p0 + g < nplanes && keep[j] && MTE_SLOT_OK(d0, a.cap)) pl[pb + (uint32_t)d0] = v[g][j];
                d0 += keep[j] ? 1 : 0;
              }
            }
          }
          vm_drain();
        }
        w += tot;
      }
      D.n = w;
    }
  }
  return 0;
}

// pass 3: documents pass 2 escalated (more than 1,022 segments)
template <int K, bool S>
__global__ __launch_bounds__(256) void stream_kernel(ReplayArgs a) {
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int idx = (int)blockIdx.x * kDocsPerBlock + w;
  if (idx >= (int)a.n_docs) return;
  // longest batch first (a.sorder): the long local-client chains start first
  const int doc = a.sorder ? (int)__builtin_amdgcn_readfirstlane((int)a.sorder[idx]) : idx;
  // documents pass 2 escalated, and the new length-calc documents with delta
  // events and no local client (a local client's go to the HBM tree pass)
  const uint32_t hf = a.hdr[doc].flags;
  // These two are doc_owner(hf) == kOwnHtree and == kOwnStream (mte_kernels.h)
  // spelled out: through the function the compiler allocates this kernel's
  // scalar registers otherwise (other SGPR spill counts).  The HBM tree pass's
  // legacy documents with delta events pass the first test and leave at the
  // third: nothing sets kHdrNeedsEsc on a document that pass 1 and
  // rel_route_kernel do not own.  A change of the routing rule changes these.
  if (hf & (MTE_DOC_LOCAL_CLIENT | MTE_DOC_TREE)) return;  // the HBM tree pass's
  const bool own = (hf & (MTE_DOC_EVENTS | MTE_DOC_NEW_LENGTH_CALC)) == (MTE_DOC_EVENTS | MTE_DOC_NEW_LENGTH_CALC);
  if (!(hf & kHdrNeedsEsc) && !own) return;  // untouched doc: leave the header alone
  DocRun D;
  run_init(D, a, doc, !own);
  uint32_t st[kNumStats] = {};
  EvOut ev{nullptr, 0, 0u, 0u};
  if ((hf & MTE_DOC_EVENTS) && a.dl_off) {
    ev.p = a.dl + a.dl_off[doc];
    ev.cap = a.dl_off[doc + 1] - a.dl_off[doc];
  }
  if (D.running) {
    s8v cur = sload8(D.recp + 2 * D.k);
    while (D.running) {
      const int rc = stream_step<K, S>(D, st, cur, a, ev);
      if (rc < 0) {
        D.status = rc;
        D.running = false;
      } else if (D.k >= D.k1) {
        D.running = false;
      } else if (S && st[kStOps] >= (1u << 20)) {
        run_flush_stats(D, st, a);
      }
    }
    if constexpr (S) run_flush_stats(D, st, a);
  }
  if ((hf & MTE_DOC_EVENTS) && a.dl_n && lane_id() == 0) a.dl_n[doc] = ev.n;
  run_finish(D, a);
}

}  // namespace mte
