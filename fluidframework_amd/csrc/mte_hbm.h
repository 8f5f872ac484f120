// mte_hbm.h — documents whose planes stay in HBM: the L1-bypassing loads and
// vm_drain, the local-client plane constants, delta events and the local
// references (slides, stream_ref, stream_marker_pos).  Layer above
// mte_docrun.h; included by pass 3 (mte_stream.h) and the HBM tree pass (mte_htree.h).
#pragma once

#include "mte_kernels.h"
#include "mte_passes.h"
#include "mte_docrun.h"

namespace mte {

constexpr int kTileE = 2;
constexpr int kTile = kWave * kTileE;  // slots per tile

__device__ __forceinline__ uint32_t ld_l2(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// plane p, slot i of a doc's planes as a 32-bit offset from the doc's base
// (global_load saddr + voffset: no 64-bit address per lane and plane)
__device__ __forceinline__ uint32_t ld_l2o(const uint32_t* pl, uint32_t off) {
  return __hip_atomic_load(pl + off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Every slot index this path computes is checked against the doc's capacity
// before it touches memory; a violation (an engine bug) stops the document
// with MTE_E_STATE instead of faulting the device.
#define MTE_SLOT_OK(i, cap) ((unsigned)(i) < (unsigned)(cap))

// hot planes (len seq rseq rmask meta toff) of tile [tb, tb + kTile); slots >= n are padding
template <int K>
__device__ __forceinline__ void tile_load_hot(Regs<kTileE, K>& R, const uint32_t* pl, uint64_t st, int tb, int n) {
  const int base = tb + lane_id() * kTileE;
#pragma unroll
  for (int j = 0; j < kTileE; j++) {
    const int i = base + j;
    const bool v = i < n;
    // unconditional loads (slot 0 stands in for padding), selected after:
    // no branch around each load
    const uint32_t x = (uint32_t)(v ? i : 0);
    const uint32_t l0 = ld_l2(pl + x), l1 = ld_l2(pl + st + x), l2 = ld_l2(pl + 2 * st + x);
    const uint32_t l3 = ld_l2(pl + 3 * st + x), l4 = ld_l2(pl + 4 * st + x), l5 = ld_l2(pl + 5 * st + x);
    R.len[j] = v ? (int32_t)l0 : 0;
    R.seq[j] = v ? (int32_t)l1 : 0;
    R.rseq[j] = v ? (int32_t)l2 : kPad;
    R.rmask[j] = v ? l3 : 0u;
    R.meta[j] = v ? l4 : 0u;
    R.toff[j] = v ? l5 : 0u;
  }
}

// ---- documents with a local client (MTE_DOC_LOCAL_CLIENT, include/mte.h) ----
// They replay on the HBM tree pass (mte_htree.h); the plane layout and the
// event / reference helpers below are shared with it.  Pending seqs are kLocalBase + localSeq (UnassignedSequenceNumber, normalised
// above every sequenced seq as breakTie / nodeLength do, mergeTree.ts:1009-1016,
// 1713-1714).  K more planes after the property planes hold, per slot and key,
// the localSeq of the last pending local annotate that set the key (0 = none):
// the pendingKeyUpdateCount of segmentPropertiesManager.ts:94-135 (acks come in
// order, so "count > 0" is "last pending localSeq not yet acked").  One more
// plane after them holds the mask of the pending annotate segment groups the
// slot belongs to (MTE_ANNOTATE_SLOTS, include/mte.h).
constexpr int32_t kLocalBase = MTE_LOCAL_SEQ_BASE;
template <int K>
constexpr int kAnnPlane = kFieldPlanes + 2 * K;
constexpr int kPlaneGroup = 5;  // planes moved per batch of loads (all in flight, then the stores)

// ---- delta events (MTE_DOC_EVENTS, include/mte.h) ----------------------------
// The doc's own view: removed -> 0, else the length (Client.getPosition,
// client.ts:345-350, through nodeLength for the local client).
struct EvOut {
  mte_delta* p;   // the doc's region
  uint64_t cap;   // its size
  uint32_t n;     // events so far (may pass cap: overflow)
  uint32_t op;    // the record being applied
};
__device__ __forceinline__ void ev_one(EvOut& ev, uint32_t kind, int32_t pos, int32_t len) {
  if (lane_id() == 0 && ev.n < ev.cap) ev.p[ev.n] = mte_delta{ev.op, kind, pos, len, 0u};
  ev.n++;
}
// the own view's length of slots [0, g)
__device__ __forceinline__ int32_t own_prefix(const uint32_t* pl, uint64_t sd, int g) {
  int32_t acc = 0;
  for (int tb = 0; tb < g; tb += kTile) {
#pragma unroll
    for (int j = 0; j < kTileE; j++) {
      const int i = tb + lane_id() * kTileE + j;
      const int ic = i < g ? i : 0;  // unconditional loads, selected after
      const int32_t rs = (int32_t)ld_l2(pl + 2 * sd + ic), ln = (int32_t)ld_l2(pl + ic);
      acc += (i < g && rs == kNone) ? ln : 0;
    }
  }
  return rdlane(wave_incl_scan(acc), kWave - 1);
}

// ---- local references (MTE_DOC_REFS, include/mte.h) -------------------------
// (the reference words kRefLive ... kRefTransOff: mte_passes.h)

// a segment references may slide to (_getSlideToSegment, mergeTree.ts:893-913):
// not a pending insert and not removed-and-acked (a pending removal is fine)
__device__ __forceinline__ bool slide_ok(int32_t sq, int32_t rs) { return sq < kLocalBase && rs >= kLocalBase; }

// the first slot a reference may slide to after x (dir > 0) or before it
// (dir < 0), or -1; x is wave-uniform.  grp != 0: the removals of one ack
// (removedSeq grp) are acked segment by segment in group order (gp: the
// group-order plane), so the ones after `cur` in it are still pending when x's
// references slide (ackPendingSegment, mergeTree.ts:1285-1304)
// tw (the tree words, or nullptr): a merged leaf's items are one segment, so
// the search starts past x's leaf (its kTCont continuations / its head)
// gm / gid: a group member's word in plane gm is gid (its localSeq)
__device__ __forceinline__ int find_slide_target(const uint32_t* pl, uint64_t sd, int n, int x, int dir,
                                                 int32_t grp = 0, const uint32_t* gp = nullptr, uint32_t cur = 0,
                                                 const uint32_t* tw = nullptr, const uint32_t* gm = nullptr,
                                                 uint32_t gid = 0) {
  const int l = lane_id();
  if (dir > 0) {
    int b0 = x + 1;
    if (tw)
      while (b0 < n && (uni(ld_l2(tw + b0)) & kTCont)) b0++;
    for (int b = b0; b < n; b += kWave) {
      const int i = b + l;
      const int ic = i < n ? i : 0;  // unconditional loads, selected after
      const int32_t sq = (int32_t)ld_l2(pl + sd + ic), rs = (int32_t)ld_l2(pl + 2 * sd + ic);
      const bool pend = grp != 0 && rs == grp && sq < kLocalBase && ld_l2(gp + ic) > cur && ld_l2(gm + ic) == gid;
      const uint64_t m = __ballot(i < n && (slide_ok(sq, rs) || pend));
      if (m) return b + __ffsll((long long)m) - 1;
    }
  } else {
    int e0 = x;
    if (tw)
      while (e0 > 0 && (uni(ld_l2(tw + e0)) & kTCont)) e0--;
    for (int e = e0; e > 0; e -= kWave) {  // slots [e - 64, e)
      const int i = e - kWave + l;
      const int ic = i >= 0 ? i : 0;
      const int32_t sq = (int32_t)ld_l2(pl + sd + ic), rs = (int32_t)ld_l2(pl + 2 * sd + ic);
      const bool pend = grp != 0 && rs == grp && sq < kLocalBase && ld_l2(gp + ic) > cur && ld_l2(gm + ic) == gid;
      const uint64_t m = __ballot(i >= 0 && (slide_ok(sq, rs) || pend));
      if (m) return e - kWave + (63 - __builtin_clzll(m));
    }
  }
  return -1;
}

// slideAckedRemovedSegmentReferences (mergeTree.ts:921-950) for every segment
// the op of seq s made removed-and-acked -- its removedSeq is now s: a remote
// remove's new removals and the pending ones it overtook (:1936-1938,
// 1986-1993), or the local removals an ack sequenced (:1302-1304).  Each such
// segment's SlideOnRemove references move to offset 0 of the first following
// segment they may slide to (addBeforeTombstones), else to the last offset of
// the last preceding one (addAfterTombstones), else come off the segment's list
// (kRefOff); Simple references detach, or come off the list when there is no
// segment to slide to (localReference.ts:422-485).  Slots [0, rhi) of the table rt.
// ev (MTE_DOC_EVENTS documents): one MTE_DELTA_SLIDE record per reference that
// slid or came off its segment -- the reference calls its beforeSlide /
// afterSlide callbacks there (mergeTree.ts:936-942, localReference.ts:436-447,
// 471-480), which an interval collection turns into "changeInterval" events
// mid-op (intervalCollection.ts:1042-1053): pos = the own-view position of the
// removed segment it sat on, len = the unit it left (mte_htree.h
// ht_slide_keys makes it the unit's order key), removed = its slot,
// kind = MTE_DELTA_SLIDE | 1 if
// it moved to a segment | 2 if to the end of a preceding one | its offset in
// the removed segment << 16 (clamped):
// the host orders one segment's references as its LocalReferenceCollection
// iterates them.
enum { kSlideAll = 0, kSlideAck = 1, kSlideOverlap = 2, kSlideNew = 3 };
// one removed segment x's references (grp / gp / cur: find_slide_target)
__device__ __forceinline__ void slide_segment(const uint32_t* pl, uint64_t sd, int n, uint2* rt, uint32_t rhi, int x,
                                              EvOut* ev, int32_t grp, const uint32_t* gp, uint32_t cur,
                                              const uint32_t* tw, const uint32_t* gm = nullptr, uint32_t gid = 0) {
  const int l = lane_id();
  const uint32_t toff = uni(ld_l2(pl + 5 * sd + x)), len = uni(ld_l2(pl + x));
  // an item continuing a merged leaf is one segment with the items before it:
  // offsets count from the leaf's first unit
  uint32_t lead = 0;
  if (tw)
    for (int y = x; y > 0 && (uni(ld_l2(tw + y)) & kTCont); y--) lead += uni(ld_l2(pl + y - 1));
  int t = find_slide_target(pl, sd, n, x, 1, grp, gp, cur, tw, gm, gid);
  bool after = false;
  if (t < 0) {
    t = find_slide_target(pl, sd, n, x, -1, grp, gp, cur, tw, gm, gid);
    after = t >= 0;
  }
  uint32_t to = 0;
  if (t >= 0) {
    const uint32_t tt = uni(ld_l2(pl + 5 * sd + t)), tl = uni(ld_l2(pl + t));
    to = after ? tt + tl - 1u : tt;
  }
  const int32_t xpos = ev ? own_prefix(pl, sd, x) : 0;
  for (uint32_t rb = 0; rb < rhi; rb += kWave) {
    const uint32_t r = rb + (uint32_t)l;
    const uint32_t rc = r < rhi ? r : 0u;  // unconditional loads, selected after
    const uint32_t anc = ld_l2(&rt[rc].x), st = ld_l2(&rt[rc].y);
    const bool hit = r < rhi && (st & kRefLive) && !(st & (kRefDetached | MTE_REF_STAY_ON_REMOVE)) && anc - toff < len;
    const bool moves = (st & MTE_REF_SLIDE_ON_REMOVE) && t >= 0;
    if (hit) {
      if (moves) rt[r].x = to;
      else rt[r].y = st | kRefDetached | (t < 0 ? kRefOff : 0u);
    }
    if (ev) {
      const uint64_t hm = __ballot(hit);
      if (hm) {
        const uint32_t idx = ev->n + __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u));
        const uint32_t off = lead + (anc - toff) < 0xffffu ? lead + (anc - toff) : 0xffffu;
        if (hit && idx < ev->cap)
          ev->p[idx] = mte_delta{ev->op, MTE_DELTA_SLIDE | (moves ? 1u : 0u) | (moves && after ? 2u : 0u) | (off << 16), xpos,
                                 (int32_t)anc, r};
        ev->n += (uint32_t)__popcll(hm);
      }
    }
  }
  vm_drain();
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
    v = w < v ? w : v;
  }
  return v;
}

// mode: kSlideAll every such segment; kSlideAck the removals of one localSeq's
// group (gm / gid: its members hold gid there) in group order (gp: the
// group-order plane), each slid while the later ones are still pending (a reference can slide again from a later one: one record per
// slide); kSlideOverlap / kSlideNew a remote remove's segments that the local
// client had removed already (lrp: the local-removal plane, non-zero) -- slid
// before the delta callback -- then the newly removed ones, after it
// (mergeTree.ts:1970-1993).  lrp: the local-removal plane (overlap modes) or
// the group-order plane (kSlideAck).
__device__ __forceinline__ void stream_slide(const uint32_t* pl, uint64_t sd, int n, uint2* rt, uint32_t rhi, int32_t s,
                                             EvOut* ev = nullptr, int mode = kSlideAll,
                                             const uint32_t* lrp = nullptr, const uint32_t* tw = nullptr,
                                             const uint32_t* gm = nullptr, uint32_t gid = 0) {
  const int l = lane_id();
  if (mode == kSlideAck) {
    const uint32_t* gp = lrp;
    uint32_t cur = 0;
    for (bool first = true;; first = false) {
      // the group's next segment: the lowest order above cur among removedSeq s
      uint32_t best = 0xffffffffu;
      int bx = -1;
      for (int tb = 0; tb < n; tb += kWave) {
        const int i = tb + l;
        const int ic = i < n ? i : 0;
        const int32_t rs = (int32_t)ld_l2(pl + 2 * sd + ic);
        const uint32_t g = ld_l2(gp + ic);
        const bool c = i < n && rs == s && ld_l2(gm + ic) == gid && (first || g > cur);
        const uint32_t mn = wave_min_u32(c ? g : 0xffffffffu);
        const uint64_t at = __ballot(c && g == mn);
        if (at && (bx < 0 || mn < best)) {
          best = mn;
          bx = tb + __ffsll((long long)at) - 1;
        }
      }
      if (bx < 0) return;
      cur = best;
      slide_segment(pl, sd, n, rt, rhi, bx, ev, s, gp, cur, tw, gm, gid);
    }
  }
  for (int tb = 0; tb < n; tb += kWave) {
    const int i = tb + l;
    const int ic = i < n ? i : 0;
    const int32_t rs = (int32_t)ld_l2(pl + 2 * sd + ic);
    const bool lr = mode >= kSlideOverlap && ld_l2(lrp + ic) != 0u;
    uint64_t m = __ballot(i < n && rs == s && (mode < kSlideOverlap || lr == (mode == kSlideOverlap)));
    while (m) {
      const int x = tb + __ffsll((long long)m) - 1;
      m &= m - 1;
      slide_segment(pl, sd, n, rt, rhi, x, ev, 0, nullptr, 0u, tw);
    }
  }
}

// the anchor a reference on slot x moves to when x is removed and acked
// (_getSlideToSegment, mergeTree.ts:893-913; Client.getSlideToSegment's offset,
// client.ts:1117-1130), or false when there is none; x is wave-uniform
__device__ __forceinline__ bool slide_anchor(const uint32_t* pl, uint64_t sd, int n, int x, uint32_t& to) {
  int t = find_slide_target(pl, sd, n, x, 1);
  bool after = false;
  if (t < 0) {
    t = find_slide_target(pl, sd, n, x, -1);
    after = true;
  }
  if (t < 0) return false;
  const uint32_t tt = uni(ld_l2(pl + 5 * sd + t)), tl = uni(ld_l2(pl + t));
  to = after ? tt + tl - 1u : tt;
  return true;
}

// MTE_OP_REF (include/mte.h):
//   b = 0: createLocalReferencePosition on the segment and offset
//     getContainingSegment(pos1) finds in the local view (client.ts:360-364,
//     1107-1110; mergeTree.ts:872-885, 2124-2143);
//   b = 1: removeLocalReferencePosition (mergeTree.ts:2113-2123);
//   b = 2: a reference a sequenced op creates (createPositionReference with an
//     op, intervalCollection.ts:639-658): getContainingSegment in the op's
//     perspective (ref_seq, client), then getSlideToSegment; no segment: detached;
//   b = 3: the reference becomes SlideOnRemove (a = its new type) and slides if
//     its segment is removed and acked (ackInterval, :1805-1902).
// rhi: slots in use so far.
template <int K>
__device__ __forceinline__ int stream_ref(const uint32_t* pl, uint64_t sd, int n, uint2* rt, uint32_t& rhi, const s8v& op,
                          int32_t m, bool newcalc) {
  const uint32_t slot = (uint32_t)op[5], b = (uint32_t)op[7], typ = (uint32_t)op[6];
  const int l = lane_id();
  if (b == 1u) {
    if (l == 0) rt[slot] = make_uint2(0u, 0u);
    vm_drain();
    return 0;
  }
  if (typ & MTE_REF_TRANSIENT) return MTE_E_UNSUPPORTED;
  if ((typ & MTE_REF_SLIDE_ON_REMOVE) && (typ & MTE_REF_STAY_ON_REMOVE)) return MTE_E_INVALID_ARG;
  if (b == 3u) {
    const uint32_t st0 = ld_l2(&rt[slot].y), anc = ld_l2(&rt[slot].x);
    if (!(st0 & kRefLive)) return MTE_E_INVALID_ARG;
    uint32_t st = (st0 & (kRefLive | kRefDetached | kRefOff)) | (typ & 0xffffu), to = anc;
    if (!(st & kRefDetached) && (st & MTE_REF_SLIDE_ON_REMOVE)) {
      // the slot holding the reference's unit
      for (int tb = 0; tb < n; tb += kWave) {
        const int i = tb + l;
        const int ic = i < n ? i : 0;  // unconditional loads, selected after
        const uint32_t tf = ld_l2(pl + 5 * sd + ic), ln = ld_l2(pl + ic);
        const uint64_t mk = __ballot(i < n && anc - tf < ln);
        if (mk) {
          const int x = tb + __ffsll((long long)mk) - 1;
          const int32_t rs = (int32_t)uni(ld_l2(pl + 2 * sd + x));
          if (rs != kNone && rs < kLocalBase && !slide_anchor(pl, sd, n, x, to)) st |= kRefDetached;
          break;
        }
      }
    }
    if (l == 0) rt[slot] = make_uint2(to, st);
    vm_drain();
    return 0;
  }
  const bool remote = b == 2u;
  const int32_t pos = op[4], r = op[1];
  const uint32_t c = ((uint32_t)op[3] >> 8) & 0xffu;
  int32_t carry = 0;
  for (int tb = 0; tb < n; tb += kTile) {
    Regs<kTileE, K> R;
    tile_load_hot<K>(R, pl, sd, tb, n);
    int32_t L[kTileE], P[kTileE];
    if (remote) {
      leaf_lengths<kTileE, K>(R, r, c + 1, (int)c, m, newcalc, L);
    } else {
#pragma unroll
      for (int j = 0; j < kTileE; j++) L[j] = R.rseq[j] == kNone ? R.len[j] : 0;  // the local view: removed -> 0
    }
#pragma unroll
    for (int j = 0; j < kTileE; j++) L[j] = L[j] > 0 ? L[j] : 0;  // padding / undefined: nothing
    const int32_t tot = prefix<kTileE>(L, P);
    bool hit = false;
    uint32_t anc = 0;
    int jx = 0;
#pragma unroll
    for (int j = 0; j < kTileE; j++) {
      const bool h = L[j] > 0 && pos >= carry + P[j] && pos < carry + P[j] + L[j];
      anc = h ? R.toff[j] + (uint32_t)(pos - carry - P[j]) : anc;
      jx = h ? j : jx;
      hit = hit || h;
    }
    const uint64_t mk = __ballot(hit);
    if (mk) {
      const int ls = __ffsll((long long)mk) - 1;
      uint32_t a0 = rdlane(anc, ls), st = kRefLive | (typ & 0xffffu);
      if (remote) {
        const int x = tb + ls * kTileE + rdlane(jx, ls);
        const int32_t rs = (int32_t)uni(ld_l2(pl + 2 * sd + x));
        if (rs != kNone && rs < kLocalBase && !slide_anchor(pl, sd, n, x, a0)) st |= kRefDetached;
      }
      if (l == 0) rt[slot] = make_uint2(a0, st);
      vm_drain();
      if (slot + 1 > rhi) rhi = slot + 1;
      return 0;
    }
    carry += tot;
  }
  if (!remote) return MTE_E_INVALID_ARG;  // no segment holds pos in the local view
  if (l == 0) rt[slot] = make_uint2(0u, kRefLive | kRefDetached | (typ & 0xffffu));  // detached
  vm_drain();
  if (slot + 1 > rhi) rhi = slot + 1;
  return 0;
}

// MTE_OP_RELPOS (include/mte.h): the position of the first marker whose key
// plane `key` holds `vid`, in the view (r, c) -- getPosition (mergeTree.ts:
// 853-870) sums the lengths of everything before it; undefined leaves count 0
// -- or -1 when no held marker carries the id (posFromRelativePos,
// mergeTree.ts:1369-1392).  One front-to-back tile scan with early exit.
template <int K>
__device__ int32_t stream_marker_pos(const uint32_t* pl, uint64_t sd, int n, uint32_t key, uint32_t vid, int32_t r,
                                     uint32_t c, int32_t m, bool newcalc) {
  if (key >= (uint32_t)K || vid == 0u) return -1;
  constexpr int E = kTileE;
  const uint32_t* kp = pl + (uint64_t)(kFieldPlanes + key) * sd;
  int32_t carry = 0;
  for (int tb = 0; tb < n; tb += kTile) {
    Regs<E, K> R;
    tile_load_hot<K>(R, pl, sd, tb, n);
    int32_t L[E], P[E];
    leaf_lengths<E, K>(R, r, c + 1, (int)c, m, newcalc, L);
    const int32_t tot = prefix<E>(L, P);
    int jsel = E;
#pragma unroll
    for (int j = E - 1; j >= 0; j--) {
      const int i = tb + lane_id() * E + j;
      const uint32_t v = ld_l2(kp + (i < n ? i : 0));  // unconditional, selected after
      jsel = (i < n && (R.meta[j] >> 8) != 0u && v == vid) ? j : jsel;
    }
    const uint64_t msk = __ballot(jsel < E);
    if (msk) {
      const int ls = __ffsll((long long)msk) - 1;
      int32_t pv = P[0];
#pragma unroll
      for (int j = 1; j < E; j++) pv = jsel == j ? P[j] : pv;
      return carry + (int32_t)rdlane(pv, ls);
    }
    carry += tot;
  }
  return -1;
}

}  // namespace mte
