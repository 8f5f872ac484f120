// mte_step1.h — the per-op step of the pass-1 register tiers (E <= 4 slots
// per lane, documents of <= 254 segments: nearly every op of a conflict-farm
// batch).
//
// Same semantics as doc_step (mte_step8.h, which cites the reference for
// every rule), but the split / insert decisions stay per slot instead of
// going through scalar lookups: a slot learns "I am after the split leaf"
// from the popcount of the candidate ballot in the lanes below (v_mbcnt) plus
// its own lane's earlier slots, "I am right after it" from its neighbour's
// flag, and every piece of a split leaf is rebuilt from the values the slot
// pulled in the shift.  The scalar unit — one per CU, shared by four SIMDs —
// then only decodes the op and branches on the op type and on "is there a
// split"; the rest is VALU work on each SIMD.
//
// What depends on the records alone is done 64 records at a time (block_run,
// the tiers E <= kBlockEmax): lane i loads record D.k + i whole, the wave
// decodes it, checks client and type and runs the whole collab window as a
// prefix computation (running maxima of the ENDs' seq and min_seq), and the op
// loop reads a record with v_readlane at a scalar lane index and tests one bit
// for "minSeq advances here"; the words only some ops use (minSeq, the text
// offset, the property sets) are read where they are used (LaneWords).  The
// shift itself goes through the LDS crossbar at E = 1 (one ds_bpermute per
// plane) and at E = 2 (two, and two selects), plane by plane through DPP at
// E = 4 (shift_v).  E = 4 keeps the per-op fetch and window of
// doc_step_v.  On the kPack4 layout a property set is applied as the (keep,
// val) pair props_kernel folded it into (mte_kernels.h), whatever its size.
#pragma once

#include "mte_kernels.h"
#include "mte_docrun.h"
#include "mte_regdoc.h"

namespace mte {

// MTE_PASS1_UNIT is defined by mte_pass_pair.hip alone.  The step is shared
// with pass 2 (big_kernel runs doc_step_v at E = 4) and the chunk pass, whose
// units are compiled as before; what is written for pass 1's own compile
// (its unit leaves wave-uniform branches unstructurized, Makefile) is under
// this constant, so the other units' device code does not move with it.
#ifdef MTE_PASS1_UNIT
constexpr bool kPass1Unit = true;
#else
constexpr bool kPass1Unit = false;
#endif

// ---- per-slot flags ----------------------------------------------------------
// A per-slot flag is one bit of an integer held per lane: bit j of the word is
// the flag of slot j.  Flags are combined with integer VALU ops; a lane mask
// (v_cmp into an SGPR pair) is made only where a select consumes one.  As
// bools every && / || / ! between flags is a 64-bit scalar instruction per
// slot, on the one scalar unit the CU's four SIMDs share.  The words pass
// through an empty asm (as in pick(), mte_kernels.h): without it the compiler
// folds the integer logic back into lane-mask logic.
__device__ __forceinline__ uint32_t vpin(uint32_t x) {
  asm("" : "+v"(x));
  return x;
}

template <int E>
constexpr uint32_t kAllSlots = (1u << E) - 1u;

// the word with bit j set where c holds
__device__ __forceinline__ uint32_t fbit(bool c, int j) { return vpin(c ? (1u << j) : 0u); }
// flag of slot j (w pinned)
__device__ __forceinline__ bool fget(uint32_t w, int j) { return ((w >> j) & 1u) != 0; }

template <int E>
__device__ __forceinline__ void funpack(uint32_t w, bool (&b)[E]) {
#pragma unroll
  for (int j = 0; j < E; j++) b[j] = fget(w, j);
}

// bit j = some flagged slot lies before slot j (in this lane or a lower one)
template <int E>
__device__ __forceinline__ uint32_t after_flag(uint32_t F) {
  const uint32_t below = lanes_below(__ballot(F != 0));
  uint32_t pe = 0;  // flags of this lane's earlier slots, or-ed
  if constexpr (E > 1) {
    pe = F << 1;
#pragma unroll
    for (int sh = 1; sh < E - 1; sh <<= 1) pe |= pe << sh;
    pe &= kAllSlots<E>;
  }
  return vpin(pe | (below ? kAllSlots<E> : 0u));
}

// bit j of F1 / F2 = the flag of the slot 1 / 2 positions before slot j
template <int E>
__device__ __forceinline__ void prev_flags(uint32_t F, uint32_t& F1, uint32_t& F2) {
  // the previous lane's flags below this lane's (lane 0 gets 0)
  const uint32_t cat = (F << E) | (uint32_t)lane_prev((int32_t)F);
  F1 = vpin((cat >> (E - 1)) & kAllSlots<E>);
  if constexpr (E >= 2) F2 = vpin((cat >> (E >= 2 ? E - 2 : 0)) & kAllSlots<E>);
  else F2 = vpin((uint32_t)lane_prev((int32_t)F1));
}

template <typename T>
__device__ __forceinline__ T perm1(T v, int addr) {
  return (T)__builtin_amdgcn_ds_bpermute(addr, (int32_t)v);
}

template <int E, typename T>
__device__ __forceinline__ void perm_plane(T (&F)[E], int addr) {
  F[0] = perm1(F[0], addr);
}

// one plane of shift_v at E = 4: its two cross-lane moves, then its selects.  The E = 4
// tier shifts plane by plane: moving all 13 planes' neighbours first needs 52
// temporaries on top of 40 state registers, which spilled the whole pass-1
// kernel (its register budget is that of its largest tier)
template <int E, typename T>
__device__ __forceinline__ void shift_plane(T (&F)[E], const bool (&g1)[E], const bool (&g2)[E]) {
  const T p1 = (T)lane_prev((int32_t)F[E - 1]);
  const T p2 = (T)lane_prev((int32_t)F[E >= 2 ? E - 2 : 0]);
#pragma unroll
  for (int j = E - 1; j >= 0; j--) {
    const T m1 = (j >= 1) ? F[j >= 1 ? j - 1 : 0] : p1;
    const T m2 = (j >= 2) ? F[j >= 2 ? j - 2 : 0] : ((j == 1) ? p1 : p2);
    F[j] = g2[j] ? m2 : (g1[j] ? m1 : F[j]);
  }
}

// one plane of shift_v at E = 2: slot 0 pulled through a0, slot 1 through a1
// (byte addresses of the source lanes), then one select per slot: slot 0 takes
// the slot-1 pull where it moves by one (once0), slot 1 its own lane's old
// slot 0 where it moves by one (once1)
template <typename T>
__device__ __forceinline__ void pull_plane2(T (&F)[2], int a0, int a1, bool once0, bool once1) {
  const T b0 = perm1(F[0], a0), b1 = perm1(F[1], a1);
  F[1] = once1 ? F[0] : b1;
  F[0] = once0 ? b1 : b0;
}

// new[i] = old[i - d(i)], d = g1 + g2 (g2 implies g1; flag words), for every
// plane and the NX extra per-slot values X.  E == 1: lane l pulls lane l - d(l)
// through the LDS crossbar (ds_bpermute: one LDS-pipe instruction per plane
// instead of two DPP moves and two selects on the VALU).  E == 2: two pulls and
// two selects per plane (below).  E == 4: two DPP moves and the selects, plane
// by plane (shift_plane).
template <int E, int K, int NX>
__device__ __forceinline__ void shift_v(Regs<E, K>& R, int32_t (&X)[NX > 0 ? NX : 1][E], uint32_t g1w,
                                        uint32_t g2w) {
  if constexpr (E == 2) {
    // Slot j of lane l is global index 2l + j, and d is non-decreasing in i and
    // never jumps by two, so a lane's (d0, d1) is one of (0,0), (0,1), (1,1),
    // (1,2), (2,2).  Slot 0 wants lane l's slot 0 (d0 = 0), lane l-1's slot 1
    // (d0 = 1) or lane l-1's slot 0 (d0 = 2); slot 1 wants lane l's slot 1
    // (d1 = 0), lane l's slot 0 (d1 = 1) or lane l-1's slot 1 (d1 = 2).  So the
    // slot-0 plane is pulled from lane l - (d0 == 2) and the slot-1 plane from
    // lane l - (d0 >= 1): at (1,2) both slots want that one value, at (1,1)
    // slot 1 takes its own lane's slot 0 and the pull serves slot 0 alone, and
    // d1 = 2 implies d0 >= 1.  The crossbar wraps modulo 64, so lane 0 must not
    // pull from lane -1 into a slot that is kept: its slot 1 (i = 1) never moves
    // by two, and its slot 0 moves only for an insert before the first segment,
    // which then overwrites the slot whole (put_new_v).
    const uint32_t once = vpin(g1w & ~g2w);  // bit j: d_j == 1
    const int self = lane_id() << 2;
    const int a0 = self - (int)((g2w & 1u) << 2), a1 = self - (int)((g1w & 1u) << 2);
    const bool o0 = fget(once, 0), o1 = fget(once, 1);
    // what the caller's piece arithmetic reads first goes first
#pragma unroll
    for (int x = 0; x < NX; x++) pull_plane2(X[x], a0, a1, o0, o1);
    pull_plane2(R.len, a0, a1, o0, o1);
    pull_plane2(R.toff, a0, a1, o0, o1);
    pull_plane2(R.seq, a0, a1, o0, o1);
    pull_plane2(R.rseq, a0, a1, o0, o1);
    pull_plane2(R.rmask, a0, a1, o0, o1);
    pull_plane2(R.meta, a0, a1, o0, o1);
#pragma unroll
    for (int k = 0; k < kRegPlanes<K>; k++) pull_plane2(R.pr[k], a0, a1, o0, o1);
  } else if constexpr (E == 1) {
    const int addr = (lane_id() - (int)g1w - (int)g2w) << 2;
    perm_plane<E>(R.len, addr);
    perm_plane<E>(R.seq, addr);
    perm_plane<E>(R.rseq, addr);
    perm_plane<E>(R.rmask, addr);
    perm_plane<E>(R.meta, addr);
    perm_plane<E>(R.toff, addr);
#pragma unroll
    for (int k = 0; k < kRegPlanes<K>; k++) perm_plane<E>(R.pr[k], addr);
#pragma unroll
    for (int x = 0; x < NX; x++) perm_plane<E>(X[x], addr);
  } else {
    bool g1[E], g2[E];
    funpack<E>(g1w, g1);
    funpack<E>(g2w, g2);
    shift_plane<E>(R.len, g1, g2);
    shift_plane<E>(R.seq, g1, g2);
    shift_plane<E>(R.rseq, g1, g2);
    shift_plane<E>(R.rmask, g1, g2);
    shift_plane<E>(R.meta, g1, g2);
    shift_plane<E>(R.toff, g1, g2);
#pragma unroll
    for (int k = 0; k < kRegPlanes<K>; k++) shift_plane<E>(R.pr[k], g1, g2);
#pragma unroll
    for (int x = 0; x < NX; x++) shift_plane<E>(X[x], g1, g2);
  }
}

// the inserted segment at the slots flagged in `atw` (mergeTree.ts:1599-1611,
// textSegment.ts:40-48, mergeTreeNodes.ts:602-609)
template <int E, int K, bool S, typename LW>
__device__ __forceinline__ void put_new_v(Regs<E, K>& R, uint32_t atw, const s8v& op, const LW& late, uint32_t c,
                                          uint32_t flags, const ReplayArgs& a, uint32_t (&st)[kNumStats]) {
  const int32_t s = op[0], pos2 = op[5];
  const bool marker = (flags & MTE_F_MARKER) != 0;
  const int32_t nlen = marker ? 1 : pos2;
  const uint32_t meta = (c + 1u) | (marker ? (1u + (uint32_t)pos2) << 8 : 0u);
  uint32_t toff = marker ? 0u : a.text_base + (uint32_t)late.w6();
  const uint32_t psi = (uint32_t)late.w7();
  uint32_t pr[kRP<K>][1];
  const bool one[1] = {true};
#pragma unroll
  for (int kk = 0; kk < kRP<K>; kk++) pr[kk][0] = 0;
  if (kKeys<K> > 0 && psi != MTE_NO_PROPS) {
    const s8v q2 = sload_props(a, psi);
    if constexpr (K == kPack4) {
      // the set folded by props_kernel: the packed bytes, and a marker's
      // side-key value, which goes to its toff register (ReplayArgs::side_key)
      pr[0][0] = (uint32_t)q2[5];
      toff = (marker && q2[7]) ? (uint32_t)q2[6] : toff;
    } else {
      apply_props<1, K>(pr, one, (uint32_t)q2[0], (uint32_t)q2[1], (uint32_t)q2[2], psi, a);
    }
    MTE_STAT(st[kStPwrites] += (uint32_t)q2[3];)
  }
  MTE_STAT(if (!marker) st[kStUnits] += (uint32_t)pos2;)
  bool at[E];
  funpack<E>(atw, at);
#pragma unroll
  for (int j = 0; j < E; j++) {
    R.len[j] = at[j] ? nlen : R.len[j];
    R.seq[j] = at[j] ? s : R.seq[j];
    R.rseq[j] = at[j] ? kNone : R.rseq[j];
    R.rmask[j] = at[j] ? 0u : R.rmask[j];
    R.meta[j] = at[j] ? meta : R.meta[j];
    R.toff[j] = at[j] ? toff : R.toff[j];
#pragma unroll
    for (int kk = 0; kk < kRegPlanes<K>; kk++) R.pr[kk][j] = at[j] ? pr[kk][0] : R.pr[kk][j];
  }
}

// chunk pass (mte_chunk.h): the insert slot lies in a later chunk
constexpr int kNextChunk = 2;

// The segment part of one insert / remove / annotate on a register-resident
// run of segments — a whole document (doc_step_v) or one chunk of a big one
// (mte_chunk.h, CH = true).  Returns 0, MTE_E_INSERT_FAILED or (CH, insert
// only, unless `last`) kNextChunk with the registers untouched.  With CH the
// op's positions are taken relative to `off`, the chunk's first position in
// the op's perspective; *tot is the chunk's length in that perspective before
// the op and *dlen its change (+ inserted units, - units the remover saw).
//
// Words 6 and 7 of the record come through `late` (w6(), w7()): only an insert
// reads word 7 (its property set) and only a text insert or an annotate that
// marks something reads word 6, so a caller that holds the records in lanes
// (block_run) reads them there and not for every op.
template <int E, int K, bool S, bool CH, typename LW>
__device__ __forceinline__ int seg_op_v(Regs<E, K>& R, int& n, const s8v& op, const LW& late, uint32_t type,
                                        uint32_t c, uint32_t flags, int32_t m, bool newcalc, int32_t off, bool last,
                                        int32_t& tot, int32_t& dlen, const ReplayArgs& a,
                                        uint32_t (&st)[kNumStats]) {
  const int base = lane_id() * E;
  const int32_t s = op[0], r = op[1];
  const int32_t pos1 = op[4] - (CH ? off : 0);
  const int32_t pos2 = (CH && type != MTE_OP_INSERT) ? op[5] - off : op[5];
  int32_t L[E], P[E];
  leaf_lengths<E, K, true>(R, r, c + 1, (int)c, m, newcalc, L);
  const int32_t total = prefix<E>(L, P);
  if constexpr (CH) {
    tot = total;
    dlen = 0;
  }
  // split candidate at b: the visible leaf with P < b < P + L
  uint32_t slim[E];
#pragma unroll
  for (int j = 0; j < E; j++) slim[j] = L[j] > 1 ? (uint32_t)(L[j] - 1) : 0u;

  if (type == MTE_OP_INSERT) {
    // applyInsertOp -> insertSegments (client.ts:470-505, mergeTree.ts:1394-1422)
    const bool marker = (flags & MTE_F_MARKER) != 0;
    const int32_t nlen = marker ? 1 : pos2;
    int32_t X[1][E];  // split offset, meaningful at the split leaf
    uint32_t sp = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
      X[0][j] = pos1 - P[j];
      sp |= fbit(((uint32_t)X[0][j] - 1u) < slim[j], j);
    }
    sp = vpin(sp);
    uint32_t at = 0;
    if (__ballot(sp != 0)) {
      // ensureIntervalBoundary: [head][new][tail], the tail a copy of the leaf
      const uint32_t ins = uni(nlen > 0 ? ~0u : 0u);  // wave-uniform, an integer operand of the flag logic
      const uint32_t A = after_flag<E>(sp);
      uint32_t nb, nb2;
      prev_flags<E>(sp, nb, nb2);
      const uint32_t g2 = vpin(A & ~nb & ins);
      shift_v<E, K, 1>(R, X, A, g2);
      const uint32_t tail = vpin((nb2 & ins) | (nb & ~ins));
#pragma unroll
      for (int j = 0; j < E; j++) {
        const bool own = fget(sp, j), tl = fget(tail, j);
        if constexpr (!kPass1Unit) {
          R.len[j] = own ? X[0][j] : (tl ? R.len[j] - X[0][j] : R.len[j]);
          R.toff[j] = tl ? R.toff[j] + (uint32_t)X[0][j] : R.toff[j];
        } else {
          // pass 1: the same selects with both arms in locals.  A ternary with
          // arithmetic in an arm is emitted as a branch, and at E >= 2 those
          // lane-divergent branches stayed branches, which put the whole insert
          // path through the CFG structurizer and its flow blocks' copies of the
          // planes (DESIGN §6 "Uniform branches left unstructurized")
          const int32_t x = X[0][j], len = R.len[j], rest = len - x;
          const uint32_t off = R.toff[j], moved = off + (uint32_t)x;
          const int32_t kept = tl ? rest : len;
          R.len[j] = own ? x : kept;
          R.toff[j] = tl ? moved : off;
        }
      }
      at = nb & ins;
      n += nlen > 0 ? 2 : 1;
      MTE_STAT(st[kStWritten] += nlen > 0 ? 3u : 2u;)
    } else if (nlen > 0) {
      // insertingWalk: before the first defined leaf with P >= pos
      uint32_t cand = 0;
#pragma unroll
      for (int j = 0; j < E; j++) {
        const uint32_t def = fbit(L[j] >= 0, j);
        cand |= vpin(P[j] >= pos1 ? def : 0u);
      }
      cand = vpin(cand);
      if (__ballot(cand != 0)) {
        const uint32_t A = after_flag<E>(cand);
        at = cand & ~A;
        int32_t none[1][E];
        shift_v<E, K, 0>(R, none, vpin(A | cand), 0u);
      } else {
        if (CH && !last) return kNextChunk;  // the slot is in a later chunk
        if (pos1 > total) return MTE_E_INSERT_FAILED;  // mergeTree.ts:1666-1672
        const uint32_t d = (uint32_t)(n - base);  // append: the slot is padding
        at = d < (uint32_t)E ? 1u << (d & 31u) : 0u;
      }
      n += 1;
      MTE_STAT(st[kStWritten] += 1;)
    }
    at = vpin(at);
    if (nlen > 0) put_new_v<E, K, S>(R, at, op, late, c, flags, a, st);
    if constexpr (CH) dlen = nlen > 0 ? nlen : 0;
  } else {
    // markRangeRemoved / annotateRange: ensureIntervalBoundary at both ends
    // (ordered by position), then mark start <= P < end
    const int32_t b1 = pos1 < pos2 ? pos1 : pos2, b2 = pos1 < pos2 ? pos2 : pos1;
    uint32_t s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
      s1 |= fbit(((uint32_t)(b1 - P[j]) - 1u) < slim[j], j);
      s2 |= fbit(((uint32_t)(b2 - P[j]) - 1u) < slim[j], j);
    }
    s1 = vpin(s1);
    s2 = vpin(b2 != b1 ? s2 : 0u);
    uint64_t m1 = __ballot(s1 != 0), m2 = __ballot(s2 != 0);
    int32_t bA = b1;
    if (!m1) {  // only the end splits: it acts as the first split
      s1 = s2;
      s2 = 0;
      m1 = m2;
      m2 = 0;
      bA = b2;
    }
    if (m1) {
      const uint32_t A = after_flag<E>(s1);
      uint32_t B = 0;  // after the second split leaf's head (no second split: no slot)
      if (m2) {
        uint32_t nbB, nbB2;
        prev_flags<E>(s2, nbB, nbB2);
        B = vpin(after_flag<E>(s2) & ~nbB);
      }
      int32_t X[3][E];  // L, P and the split flags travel with the slot
#pragma unroll
      for (int j = 0; j < E; j++) {
        X[0][j] = L[j];
        X[1][j] = P[j];
        X[2][j] = (int32_t)(((s1 >> j) & 1u) | (((s2 >> j) & 1u) << 1));
      }
      shift_v<E, K, 3>(R, X, A, B);
#pragma unroll
      for (int j = 0; j < E; j++) {
        // which piece of its source leaf slot j now holds: piece kp of 1 + h1 +
        // h2, cut at cutA and (both ends in the leaf) at oB; every select below
        // is on one integer compare
        const int32_t hh = (int32_t)vpin((uint32_t)X[2][j]);
        const int32_t h1 = hh & 1, h2 = hh >> 1;
        const int32_t d = (int32_t)(((A >> j) & 1u) + ((B >> j) & 1u));
        const int32_t oA = bA - X[1][j], oB = b2 - X[1][j];
        const int32_t kp = hh ? d - 1 + h1 : 0;  // an unsplit leaf is its own only piece
        const int32_t cutA = h1 ? oA : oB;
        const int32_t mid = kp == 1 ? cutA : oB;
        const int32_t st0 = kp < 1 ? 0 : mid;
        const int32_t cut = kp == 0 ? cutA : oB;
        const int32_t en = kp >= h1 + h2 ? R.len[j] : cut;
        const int32_t nl = en - st0;
        L[j] = hh ? nl : X[0][j];
        P[j] = X[1][j] + st0;
        R.len[j] = nl;
        R.toff[j] += (uint32_t)st0;
      }
      n += m2 ? 2 : 1;
      MTE_STAT(st[kStWritten] += m2 ? 4u : 2u;)
    }
    if (pos2 != pos1) {
      // nodeMap (mergeTree.ts:2274-2330): no visible leaf straddles a boundary.
      // pos1 <= P < pos2 as one unsigned compare (an empty range when pos2 < pos1)
      const uint32_t span = pos2 > pos1 ? (uint32_t)pos2 - (uint32_t)pos1 : 0u;
      uint32_t inw = 0;
#pragma unroll
      for (int j = 0; j < E; j++) {
        const uint32_t vis = fbit(L[j] > 0, j);
        inw |= vpin(((uint32_t)P[j] - (uint32_t)pos1) < span ? vis : 0u);
      }
      inw = vpin(inw);
      bool in[E];
      funpack<E>(inw, in);
      uint32_t cnt = 0;  // marked slots (S), else only whether there is one
      if constexpr (S) {
#pragma unroll
        for (int j = 0; j < E; j++) cnt += (uint32_t)__popcll(__ballot(in[j]));
      } else {
        cnt = __ballot(inw != 0) ? 1u : 0u;
      }
      MTE_STAT(st[kStWritten] += cnt;)
      if (type == MTE_OP_REMOVE) {
        // markRemoved (mergeTree.ts:1924-1962)
        const uint32_t bit = 1u << c;
#pragma unroll
        for (int j = 0; j < E; j++) {
          const int32_t first = (int32_t)vpin((uint32_t)(R.rseq[j] == kNone ? s : R.rseq[j]));
          R.rseq[j] = in[j] ? first : R.rseq[j];
          R.rmask[j] = in[j] ? (R.rmask[j] | bit) : R.rmask[j];
        }
        if constexpr (CH) {  // the remover's own view loses the marked units
          int32_t rl = 0;
#pragma unroll
          for (int j = 0; j < E; j++) rl += in[j] ? L[j] : 0;
          dlen = -rdlane(wave_incl_scan(rl), kWave - 1);
        }
      } else if (cnt > 0) {
        // PropertiesManager.addProperties (segmentPropertiesManager.ts:63-151)
        const uint32_t psi = (uint32_t)late.w6();
        const s8v q2 = sload_props(a, psi);
        if constexpr (K == kPack4) {
          // the set folded by props_kernel into (keep, val); a rewrite keeps nothing
          const bool rw = (flags & MTE_F_REWRITE) != 0;
          const uint32_t keep = rw ? 0u : (uint32_t)q2[4], val = (uint32_t)q2[5];
          // the side key's value of a marker is in its toff register (put_new_v)
          if (rw && a.side_key < 4u) {
#pragma unroll
            for (int j = 0; j < E; j++) {
              const uint32_t cleared = vpin((R.meta[j] >> 8) ? 0u : R.toff[j]);
              R.toff[j] = in[j] ? cleared : R.toff[j];
            }
          }
#pragma unroll
          for (int j = 0; j < E; j++) R.pr[0][j] = in[j] ? ((R.pr[0][j] & keep) | val) : R.pr[0][j];
        } else {
          if (flags & MTE_F_REWRITE) {
#pragma unroll
            for (int kk = 0; kk < kRegPlanes<K>; kk++)
#pragma unroll
              for (int j = 0; j < E; j++) R.pr[kk][j] = in[j] ? 0u : R.pr[kk][j];
          }
          apply_props<E, K>(R.pr, in, (uint32_t)q2[0], (uint32_t)q2[1], (uint32_t)q2[2], psi, a);
        }
        MTE_STAT(st[kStPwrites] += cnt * (uint32_t)q2[3];)
      }
    }
  }
  return 0;
}

// words 6 and 7 of a record that is already in scalars
struct OpWords {
  const s8v& op;
  __device__ __forceinline__ int32_t w6() const { return op[6]; }
  __device__ __forceinline__ int32_t w7() const { return op[7]; }
};

template <int E, int K, bool S, bool CH>
__device__ __forceinline__ int seg_op_v(Regs<E, K>& R, int& n, const s8v& op, uint32_t type, uint32_t c,
                                        uint32_t flags, int32_t m, bool newcalc, int32_t off, bool last,
                                        int32_t& tot, int32_t& dlen, const ReplayArgs& a,
                                        uint32_t (&st)[kNumStats]) {
  return seg_op_v<E, K, S, CH>(R, n, op, OpWords{op}, type, c, flags, m, newcalc, off, last, tot, dlen, a, st);
}

// zamboni of a pass-1 tier after minSeq rose to msn: drop the tombstones with
// removedSeq <= msn (padding included), set D.n.  Returns true when the
// document now fits a smaller register tier (the burst ends).
template <int E, int K>
__device__ __forceinline__ bool zamboni_v(Regs<E, K>& R, DocRun& D, int n, int32_t msn, uint32_t* zlds, int emin) {
  if constexpr (E == 1) {
    // each kept slot pushes its fields to its compacted lane (ds_permute)
    const bool keep = R.rseq[0] > msn;
    const uint64_t mk = __ballot(keep);
    const int n_new = __popcll(mk);
    if (n_new != n) {
      const int addr = (keep ? (int)lanes_below(mk) : kWave - 1) << 2;
      R.len[0] = __builtin_amdgcn_ds_permute(addr, R.len[0]);
      R.seq[0] = __builtin_amdgcn_ds_permute(addr, R.seq[0]);
      R.rseq[0] = __builtin_amdgcn_ds_permute(addr, R.rseq[0]);
      R.rmask[0] = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int32_t)R.rmask[0]);
      R.meta[0] = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int32_t)R.meta[0]);
      R.toff[0] = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int32_t)R.toff[0]);
#pragma unroll
      for (int kk = 0; kk < kRegPlanes<K>; kk++)
        R.pr[kk][0] = (uint32_t)__builtin_amdgcn_ds_permute(addr, (int32_t)R.pr[kk][0]);
      const bool pad = lane_id() >= n_new;
      R.rseq[0] = pad ? kPad : R.rseq[0];
      R.len[0] = pad ? 0 : R.len[0];
      D.n = n_new;
    }
  } else {
    const int n_new = zamboni_lds<E, K>(R, n, msn, zlds);
    if (n_new != n) {
      D.n = n_new;
      // drop to a smaller register tier once the doc fits in half of it
      if (E > emin && n_new + 2 + 16 <= 32 * E) return true;
    }
  }
  return false;
}

template <int E, int K, bool S>
__device__ __forceinline__ int doc_step_v(Regs<E, K>& R, DocRun& D, uint32_t (&st)[kNumStats], uint32_t& cur,
                                          const uint32_t*& vrec, const ReplayArgs& a, uint32_t* zlds, int emin) {
  const int lim = kWave * E < (int)a.cap ? kWave * E : (int)a.cap;
  if (D.n + 2 > lim) return 1;
  if constexpr (S) {
    if (st[kStOps] >= (1u << 20)) return 1;
  }

  // ---- op record (prefetched into `cur`; see doc_step) ----------------------
  s8v op;
#pragma unroll
  for (int i = 0; i < 8; i++) op[i] = (int32_t)rdlane(cur, i);
  // the next record (zeroed pad after the last); vrec is this lane's running
  // pointer into the records, so no address is formed per op
  vrec += 8;
  cur = *vrec;
  const uint32_t w3 = (uint32_t)op[3];
  const uint32_t type = w3 & 0xffu, c = (w3 >> 8) & 0xffu, flags = w3 >> 16;
  if (c >= MTE_MAX_CLIENTS) return MTE_E_CLIENT_RANGE;
  MTE_STAT(st[kStOps]++;)
  MTE_STAT(st[kStMaxSegs] = (uint32_t)D.n > st[kStMaxSegs] ? (uint32_t)D.n : st[kStMaxSegs];)
  const int32_t s = op[0];
  const int32_t msn = op[2];
  int n = D.n;

  if (type <= MTE_OP_ANNOTATE) {
    MTE_STAT(st[kStScanned] += (uint32_t)n;)
    int32_t tot, dlen;
    const int rc = seg_op_v<E, K, S, false>(R, n, op, type, c, flags, D.min_seq, (D.flags & MTE_DOC_NEW_LENGTH_CALC) != 0,
                                            0, true, tot, dlen, a, st);
    if (rc) return rc;
  } else if (type != MTE_OP_NOOP) {
    return MTE_E_INVALID_ARG;
  }
  D.n = n;
  D.k++;

  // collab window (see doc_step)
  const bool live = type != MTE_OP_NOOP, end = (flags & MTE_F_MSG_END) != 0;
  const bool bad = (live & (s <= D.cur_seq)) | (end & (s < D.cur_seq)) | ((live | end) & (msn < D.min_seq)) |
                   (end & (msn > s));
  if (bad) return window_error(D, live, end, s, msn);
  if (end) {
    D.cur_seq = s;
    if (msn > D.min_seq) {
      D.min_seq = msn;
      if (zamboni_v<E, K>(R, D, n, msn, zlds, emin)) return 1;
    }
  }
  return 0;
}

// ---- block decode ------------------------------------------------------------
// The tiers E <= kBlockEmax take their records 64 at a time: lane i holds
// record D.k + i whole, and what depends on the records alone -- the field
// decode, the client / type checks and the whole collab window, a prefix
// computation over the records -- is done once per block with vector
// instructions.  The op loop then reads a record's words with v_readlane at a
// scalar lane index (no load, no wait per op) and its window work is one bit
// test.  E = 4 keeps doc_step_v's per-op fetch: it has no registers to spare.
constexpr int kBlockEmax = 2;

template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ int32_t dpp_or(int32_t old, int32_t v) {
  // disabled / out-of-range source lanes produce `old`
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWMASK, 0xf, false);
}

// Record i's words 2, 6 and 7 out of the block's lanes, read where an op needs
// them.  A v_readlane has no side effect, so the compiler would hoist it to
// the top of the op loop beside the other words, one VALU instruction per word
// and op; the lane index passes through a volatile asm at each use, which
// stays under the branch it is written in.
struct LaneWords {
  uint32_t v2, v6, v7;  // the words of record D.k + lane
  uint32_t i;           // the record's lane, wave-uniform
  __device__ __forceinline__ int32_t at(uint32_t v) const {
    uint32_t l = i;
    asm volatile("" : "+s"(l));
    return (int32_t)rdlane(v, (int)l);
  }
  __device__ __forceinline__ int32_t w2() const { return at(v2); }
  __device__ __forceinline__ int32_t w6() const { return at(v6); }
  __device__ __forceinline__ int32_t w7() const { return at(v7); }
};

// inclusive running maximum over the 64 lanes (wave_incl_scan's shape); lo =
// INT32_MIN, the identity of max, in a register of the caller's
__device__ __forceinline__ int32_t wave_incl_max(int32_t v, int32_t lo) {
  int32_t t;
  t = dpp_or<kRowShr1>(lo, v), v = v > t ? v : t;
  t = dpp_or<kRowShr2>(lo, v), v = v > t ? v : t;
  t = dpp_or<kRowShr4>(lo, v), v = v > t ? v : t;
  t = dpp_or<kRowShr8>(lo, v), v = v > t ? v : t;
  t = dpp_or<kRowBcast15, 0xa>(lo, v), v = v > t ? v : t;
  t = dpp_or<kRowBcast31, 0xc>(lo, v), v = v > t ? v : t;
  return v;
}

// Up to kend - D.k records of one document, block by block.  Returns like
// doc_step_v: 0 (all applied), 1 (re-pick the tier) or a negative MTE_E_*; D is
// then exactly what doc_step_v leaves record after record, so the next burst
// decodes afresh from D.k.
template <int E, int K, bool S>
__device__ __forceinline__ int block_run(Regs<E, K>& R, DocRun& D, uint32_t (&st)[kNumStats], const ReplayArgs& a,
                                         uint32_t* zlds, int emin, uint32_t kend) {
  const int lim = kWave * E < (int)a.cap ? kWave * E : (int)a.cap;
  while (D.k < kend) {
    const uint32_t nb = kend - D.k < (uint32_t)kWave ? kend - D.k : (uint32_t)kWave;
    // ---- the block: record D.k + lane, zero past its end ----------------------
    // the lane index and the scans' identity are made here, per block, behind
    // an asm: as loop invariants they are hoisted out of the kernel's burst
    // loop and then live (and spill) across the E = 4 tier's code
    uint32_t lane = (uint32_t)lane_id();
    int32_t lo32 = INT32_MIN;
    asm volatile("" : "+v"(lane), "+v"(lo32));
    const bool valid = lane < nb;
    const uint4* rp = D.recp + 2 * (D.k + (valid ? lane : 0u));
    const uint4 lo = rp[0], hi = rp[1];
    uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = valid ? w[i] : 0u;
    const uint32_t vtype = w[3] & 0xffu, vc = (w[3] >> 8) & 0xffu;
    const bool vlive = vtype != MTE_OP_NOOP, vend = ((w[3] >> 16) & MTE_F_MSG_END) != 0;
    const int32_t vs = (int32_t)w[0], vmsn = (int32_t)w[2];
    // the window before each record: on the valid prefix the running maximum of
    // the ENDs' seq is "the last END's seq" and that of their min_seq is minSeq
    // (a lower value there is itself an error); behind the first bad record
    // nothing is read
    const int32_t cur_raw = wave_incl_max(vend ? vs : lo32, lo32);
    const int32_t min_raw = wave_incl_max(vend ? vmsn : lo32, lo32);
    int32_t cur_b = dpp_or<kWaveShr1>(lo32, cur_raw), min_b = dpp_or<kWaveShr1>(lo32, min_raw);
    cur_b = cur_b > D.cur_seq ? cur_b : D.cur_seq;
    min_b = min_b > D.min_seq ? min_b : D.min_seq;
    const int32_t cur_after = cur_raw > D.cur_seq ? cur_raw : D.cur_seq;  // lane i: cur_seq after record i
    const bool bad_pre = vc >= MTE_MAX_CLIENTS || (vtype > MTE_OP_ANNOTATE && vtype != MTE_OP_NOOP);
    const bool bad_win = (vlive & (vs <= cur_b)) | (vend & (vs < cur_b)) | ((vlive | vend) & (vmsn < min_b)) |
                         (vend & (vmsn > vs));
    const uint64_t mpre = __ballot(valid && bad_pre), mbad = mpre | __ballot(valid && bad_win);
    const uint32_t stop = mbad ? (uint32_t)__builtin_ctzll(mbad) : nb;  // the first bad record
    const bool stop_pre = mbad && ((mpre >> stop) & 1ull);
    // where the window advances and the zamboni runs (below the stop record)
    const uint64_t zam = __ballot(valid && vend && vmsn > min_b) & (stop < 64u ? (1ull << stop) - 1ull : ~0ull);
    // a record that only violates the window is applied before its error shows
    const uint32_t nrun = stop + ((mbad && !stop_pre) ? 1u : 0u);

    uint32_t i = 0;
    int rc = 0;
    for (; i < nrun; i++) {
      if (D.n + 2 > lim) {
        rc = 1;
        break;
      }
      if constexpr (S) {
        if (st[kStOps] >= (1u << 20)) {
          rc = 1;
          break;
        }
      }
      // words 0, 1, 3, 4, 5 of record i for every op; 2 (minSeq), 6 and 7 where
      // they are used (LaneWords)
      s8v op = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 6; j++)
        if (j != 2) op[j] = (int32_t)rdlane(w[j], (int)i);
      const LaneWords late{w[2], w[6], w[7], i};
      const uint32_t w3 = (uint32_t)op[3];
      const uint32_t type = w3 & 0xffu, c = (w3 >> 8) & 0xffu, flags = w3 >> 16;
      MTE_STAT(st[kStOps]++;)
      MTE_STAT(st[kStMaxSegs] = (uint32_t)D.n > st[kStMaxSegs] ? (uint32_t)D.n : st[kStMaxSegs];)
      int n = D.n;
      if (type <= MTE_OP_ANNOTATE) {
        MTE_STAT(st[kStScanned] += (uint32_t)n;)
        int32_t tot, dlen;
        rc = seg_op_v<E, K, S, false>(R, n, op, late, type, c, flags, D.min_seq,
                                      (D.flags & MTE_DOC_NEW_LENGTH_CALC) != 0, 0, true, tot, dlen, a, st);
        if (rc) break;
      }
      D.n = n;
      D.k++;
      if ((zam >> i) & 1ull) {
        const int32_t msn = late.w2();
        D.min_seq = msn;
        if (zamboni_v<E, K>(R, D, n, msn, zlds, emin)) {
          i++;
          rc = 1;
          break;
        }
      }
    }
    // i records of the block are applied: cur_seq is the last END's seq among
    // them.  A stop record that was applied is not counted: window_error sets
    // cur_seq itself where the reference does
    const bool stopped = rc == 0 && mbad;  // the loop reached the stop record
    const uint32_t done = (stopped && !stop_pre) ? stop : i;
    if (done) D.cur_seq = rdlane(cur_after, (int)done - 1);
    if (rc) return rc;
    if (stopped) {
      const uint32_t w3 = rdlane(w[3], (int)stop);
      const uint32_t type = w3 & 0xffu, c = (w3 >> 8) & 0xffu, flags = w3 >> 16;
      if (stop_pre) {  // nothing of the record is applied
        if (D.n + 2 > lim) return 1;
        if constexpr (S) {
          if (st[kStOps] >= (1u << 20)) return 1;
        }
        if (c >= MTE_MAX_CLIENTS) return MTE_E_CLIENT_RANGE;
        MTE_STAT(st[kStOps]++;)
        MTE_STAT(st[kStMaxSegs] = (uint32_t)D.n > st[kStMaxSegs] ? (uint32_t)D.n : st[kStMaxSegs];)
        return MTE_E_INVALID_ARG;
      }
      return window_error(D, type != MTE_OP_NOOP, (flags & MTE_F_MSG_END) != 0, (int32_t)rdlane(w[0], (int)stop),
                          (int32_t)rdlane(w[2], (int)stop));
    }
  }
  return 0;
}

}  // namespace mte
