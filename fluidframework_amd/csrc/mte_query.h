// mte_query.h — batched read-only queries over the resident segment planes.
//
// find_tiles_kernel answers mte_find_tiles (include/mte.h): for each query the
// nearest visible ReferenceType.Tile marker carrying a label, before or after
// a position of the document's own view -- MergeTree.findTile
// (mergeTree.ts:1135-1163; the forward search with recordTileStart / tileShift,
// :182-218, 1165-1215, and backwardSearch, :1217-1261), stated flat:
//
//   preceding: the last matching segment whose position P <= pos
//   following: the first matching segment whose position P >= pos
//
// where a segment matches when it is visible (rseq == kNone: not removed in
// the own view, no tree-pass placeholder), a marker whose refType has the Tile
// bit, and its value id in the query's key plane is one of the query's ids
// (the values of "referenceTileLabels" whose array holds the label; the host
// picks them).  A following hit at P >= pos is a visible unit at or after pos,
// so pos < length holds for every hit and needs no length pass; at
// pos >= length nothing is found (the reference may return a
// removed marker at pos == length).
//
// One wave per query, four queries per workgroup, as digest_kernel walks a
// document: 64 slots a step with coalesced loads of rseq, len, meta and the one
// property plane, a wave prefix sum of the visible lengths, a ballot.  Reads
// only; the one write is the query's own answer.  A document of a million
// segments is 16k steps of one wave: correct, slow; a tile-parallel variant
// (as dg_*_kernel is of the digest) is not built.
//
// text_count_kernel and text_gather_kernel answer mte_read_texts:
// MergeTreeTextHelper.getText (MergeTreeTextHelper.ts:20-74) stated flat, the
// units at own-view positions start <= p < min(end, length), a visible marker
// position contributing nothing or one 0x0020 (MTE_TEXT_PLACEHOLDERS).  The
// count walks the whole document (it also gives getLength) over rseq, len and
// meta; the host turns the counts into offsets; the gather runs the same walk
// up to `end` and copies unit-parallel: per 64-slot step each lane's clipped
// contribution is scanned, (exclusive sum, source) staged in the wave's own
// 512 B of LDS, and lane j of each round of 64 output units finds its slot by a
// 6-step search and copies one unit, so consecutive lanes write consecutive
// units whether the step is one segment of thousands of units or 64 segments
// of one.  props_at_kernel answers mte_props_at (Client.getPropertiesAtPosition,
// client.ts:1133-1141): the visible segment with P <= pos < P + L.  All three
// have find_tiles_kernel's shape (one wave per query, four per workgroup), and
// like it serve big contexts over the flat planes with one wave per document:
// correct, slow for a document of a million segments; no tile-parallel variant
// is built.  The four waves of a workgroup walk different documents: nothing
// block-wide sits in any loop.
//
// ref_positions_kernel answers mte_read_ref_positions: read_refs_view and
// mte_read_ref_order (mte_engine.hip) for any number of documents, both views
// and the order key from one walk.  One wave takes one (query, block of 64
// reference slots): lane r holds slot first + 64 b + r of the document's
// reference table.  The wave walks the document 64 segments a step as
// props_at_kernel does (len, rseq, toff coalesced; the tree word only where the
// block holds a Transient slot; one scan for the visible lengths, one for all
// lengths when the order is asked for), then broadcasts the step's segments one
// after the other with v_readlane at a uniform index (toff and len; the leaf
// id and the head bit, a ballot, only where the block holds a Transient slot)
// while every lane still looking tests its own reference and keeps the index of
// the first segment in document order that holds its unit.  After the step each
// lane pulls that segment's prefixes and removed flag across the wave
// (ds_bpermute), so the inner loop carries two broadcasts and a compare.  The
// wave leaves the walk when a ballot shows no lane looking; the wave of slot
// block 0 walks on without the inner loop, for getLength.
//
// The (query, block) of a wave comes from a task table the host uploads with
// the queries (16 B a wave: query, block, where the block's answers start),
// rather than from a search of a block-prefix array: the host sums the counts
// anyway for the offsets, the table is at most a quarter of the answers it
// describes, and a wave starts with one load where the search would take
// log2(n) dependent ones before its first useful load.
// 256 threads, no LDS (the pulls use the crossbar only), 24 VGPRs and no scratch
// as the gfx950 -O3 build reports.  One wave walks a whole document per
// 64 slots: correct, slow for a document of a million segments; no
// tile-parallel variant is built.
//
// segs_count_kernel and segs_gather_kernel answer mte_read_segment_lists: the
// list mte_read_segments returns (MTE_SEGS_RAW) for any number of documents, or
// that list dropped and coalesced as SnapshotV1.extractSegment
// (snapshotV1.ts:189-265, MTE_SEGS_V1) and SnapshotLegacy.extractSync
// (snapshotlegacy.ts:153-211, MTE_SEGS_LEGACY) reduce it at a minSeq.  One wave
// per query, four per workgroup; both kernels run segs_walk, 64 slots a step:
// rseq, seq, len, meta, toff coalesced, the tree word only where doc_has_tree,
// the property planes and one arena unit a lane (the slot's last) only in the
// coalescing modes.  A kTCont slot takes the class of its head, a kept slot
// pulls the class, last unit and property row of the kept slot before it
// (ballot, lane-mask count, ds_bpermute), and the one sequential condition of
// TextSegment.canAppend is taken in closed form over a scan of the kept
// lengths: inside a chain joined by every other condition, slot i starts a new
// row exactly when len(i) > 256 and the kept units since the chain's head
// exceed 256.  What crosses a step is wave-uniform: the last kept slot's class,
// last unit and property row, the units since the chain's head, the counts, the
// open row's length.  The count writes the counts; the host turns them into
// offsets; the gather repeats the walk, each row's start lane writes its fields
// and property row, a row's len is written when its run closes (in the step, at
// a later step's first start, or at the document's end), and the text is copied
// unit-parallel as text_gather_kernel does it (per-wave LDS staging, the 6-step
// search).  Reads of engine state only; plain vector stores of the answers.
// 256 threads; count: 37 VGPRs, no LDS, no scratch; gather: 53 VGPRs, 2 KiB of
// LDS a workgroup, no scratch, as the gfx950 -O3 build reports.  One wave walks
// a whole document: correct, slow for a document of a million segments; no
// tile-parallel variant is built.
#pragma once

#include "mte_kernels.h"
#include "mte_passes.h"

namespace mte {

constexpr int kQueriesPerBlock = 4;

__global__ __launch_bounds__(256) void find_tiles_kernel(TileArgs a) {
  const int w = threadIdx.x / kWave;
  const int l = lane_id();
  const uint32_t qi = blockIdx.x * kQueriesPerBlock + (uint32_t)w;
  if (qi >= a.n) return;
  const mte_tile_query q = a.q[qi];
  const uint32_t doc = uni(q.doc);
  const int32_t pos = uni(q.pos);
  const uint32_t first = uni(q.first), count = uni(q.count);
  const bool preceding = (uni(q.flags) & MTE_TILE_PRECEDING) != 0;
  const int32_t status = a.hdr[doc].status;
  int n = status == MTE_OK ? a.hdr[doc].nseg : 0;  // a stopped document answers -1
  n = n < 0 ? 0 : (n > (int)a.cap ? (int)a.cap : n);
  if (count == 0) n = 0;
  const uint64_t db = (uint64_t)doc * a.cap;
  const uint32_t* plane = a.soa.props + (uint64_t)q.key * a.soa.plane_stride + db;
  // the slice's first 64 ids, one per lane; a longer slice reads the rest from memory
  const uint32_t sv = (uint32_t)l < count ? a.values[first + l] : 0u;
  const int ns = count < (uint32_t)kWave ? (int)count : kWave;

  int32_t hit_pos = -1, hit_slot = -1, carry = 0;
  uint32_t hit_kind = 0;
  for (int c0 = 0; c0 < n; c0 += kWave) {
    if (preceding && carry > pos) break;  // the chunk starts beyond pos: every P > pos from here on
    const int i = c0 + l;
    const bool vis = i < n && a.soa.rseq[db + i] == kNone;
    const int32_t L = vis ? a.soa.len[db + i] : 0;
    const uint32_t kind = vis ? a.soa.meta[db + i] >> 8 : 0u;
    const uint32_t vid = vis ? plane[i] : 0u;
    const int32_t incl = wave_incl_scan(L);
    const int32_t P = carry + incl - L;
    bool member = false;
    for (int j = 0; j < ns; j++) member |= vid == rdlane(sv, j);
    for (uint32_t j = kWave; j < count; j++) member |= vid == a.values[first + j];
    const bool match = L > 0 && kind != 0 && ((kind - 1) & 1u) && vid != 0 && member;
    const unsigned long long b = __ballot(match && (preceding ? P <= pos : P >= pos));
    if (b) {
      const int s = preceding ? 63 - __builtin_clzll(b) : __builtin_ctzll(b);
      hit_pos = rdlane(P, s);
      hit_kind = rdlane(kind, s);
      hit_slot = c0 + s;
      if (!preceding) break;
    }
    carry += rdlane(incl, kWave - 1);
  }
  if (l == 0) {
    mte_tile_hit h;
    h.pos = hit_pos;
    h.status = status;
    h.ref_type = hit_slot >= 0 ? hit_kind - 1 : 0u;
    h.reserved = 0;
    a.out[qi] = h;
  }
  if (a.out_props && (uint32_t)l < a.n_keys)
    a.out_props[(uint64_t)qi * a.n_keys + l] =
        hit_slot >= 0 ? a.soa.props[(uint64_t)l * a.soa.plane_stride + db + hit_slot] : 0u;
}

// what slot [P, P + L) of kind `kind` gives a query [start, end): its clipped
// span's first position and its units (a marker's only with placeholders)
__device__ __forceinline__ int32_t text_clip(int32_t P, int32_t L, uint32_t kind, int32_t start, int32_t end,
                                             bool placeholders, int32_t* lo) {
  *lo = P > start ? P : start;
  const int32_t hi = P + L < end ? P + L : end;
  return (hi > *lo && (kind == 0 || placeholders)) ? hi - *lo : 0;
}

__global__ __launch_bounds__(256) void text_count_kernel(TextArgs a) {
  const int w = threadIdx.x / kWave;
  const int l = lane_id();
  const uint32_t qi = blockIdx.x * kQueriesPerBlock + (uint32_t)w;
  if (qi >= a.n) return;
  const mte_text_query q = a.q[qi];
  const uint32_t doc = uni(q.doc);
  const int32_t start = uni(q.start), end = uni(q.end);
  const bool ph = (uni(q.flags) & MTE_TEXT_PLACEHOLDERS) != 0;
  const DocHdr h = a.hdr[doc];
  int n = h.status == MTE_OK ? h.nseg : 0;  // a stopped document answers length = n_units = 0
  n = n < 0 ? 0 : (n > (int)a.cap ? (int)a.cap : n);
  const uint64_t db = (uint64_t)doc * a.cap;

  int32_t carry = 0, mine = 0;
  for (int c0 = 0; c0 < n; c0 += kWave) {
    const int i = c0 + l;
    const bool vis = i < n && a.soa.rseq[db + i] == kNone;
    const int32_t L = vis ? a.soa.len[db + i] : 0;
    const uint32_t kind = vis ? a.soa.meta[db + i] >> 8 : 0u;
    const int32_t incl = wave_incl_scan(L);
    int32_t lo;
    mine += text_clip(carry + incl - L, L, kind, start, end, ph, &lo);
    carry += rdlane(incl, kWave - 1);
  }
  const int32_t units = rdlane(wave_incl_scan(mine), kWave - 1);
  if (l == 0) {
    mte_text_info* o = a.info + qi;  // offset is the host's
    o->status = h.status;
    o->cur_seq = h.cur_seq;
    o->min_seq = h.min_seq;
    o->length = (uint32_t)carry;
    o->n_units = (uint32_t)units;
    o->reserved = 0;
  }
}

// the wave's LDS writes before, its reads after (no other wave shares the slice)
__device__ __forceinline__ void query_fence_wave() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

constexpr uint32_t kTextMarker = 0x80000000u;  // staged exclusive sum: the slot is a marker

__global__ __launch_bounds__(256) void text_gather_kernel(TextArgs a) {
  __shared__ uint2 stage[kQueriesPerBlock][kWave];  // (exclusive sum | kTextMarker, arena offset)
  const int w = threadIdx.x / kWave;
  const int l = lane_id();
  const uint32_t qi = blockIdx.x * kQueriesPerBlock + (uint32_t)w;
  if (qi >= a.n) return;
  const mte_text_query q = a.q[qi];
  const uint32_t doc = uni(q.doc);
  const int32_t start = uni(q.start), end = uni(q.end);
  const bool ph = (uni(q.flags) & MTE_TEXT_PLACEHOLDERS) != 0;
  int n = a.hdr[doc].status == MTE_OK ? a.hdr[doc].nseg : 0;
  n = n < 0 ? 0 : (n > (int)a.cap ? (int)a.cap : n);
  const uint64_t db = (uint64_t)doc * a.cap;
  uint16_t* out = a.text + uni64(a.offset[qi]);
  uint2* st = stage[w];

  int32_t carry = 0;
  for (int c0 = 0; c0 < n; c0 += kWave) {
    if (carry >= end) break;  // the step starts at or beyond end
    const int i = c0 + l;
    const bool vis = i < n && a.soa.rseq[db + i] == kNone;
    const int32_t L = vis ? a.soa.len[db + i] : 0;
    const uint32_t kind = vis ? a.soa.meta[db + i] >> 8 : 0u;
    const int32_t incl = wave_incl_scan(L);
    const int32_t P = carry + incl - L;
    int32_t lo;
    const int32_t c = text_clip(P, L, kind, start, end, ph, &lo);
    const int32_t cincl = wave_incl_scan(c);
    const int32_t T = rdlane(cincl, kWave - 1);  // units this step gives: below 2^31, as length is
    if (T > 0) {
      const uint32_t src = (c > 0 && kind == 0) ? a.soa.toff[db + i] + (uint32_t)(lo - P) : 0u;
      st[l] = make_uint2((uint32_t)(cincl - c) | (kind != 0 ? kTextMarker : 0u), src);
      query_fence_wave();
      for (int32_t j = l; j < T; j += kWave) {
        // the last slot whose exclusive sum is <= j: slots that give nothing
        // share theirs with the next giving one, so this is the giving one
        int s = 0;
#pragma unroll
        for (int b = kWave / 2; b > 0; b >>= 1)
          if ((int32_t)(st[s + b].x & ~kTextMarker) <= j) s += b;
        const uint2 e = st[s];
        out[j] = (e.x & kTextMarker) ? (uint16_t)0x0020 : a.arena[e.y + (uint32_t)(j - (int32_t)(e.x & ~kTextMarker))];
      }
      query_fence_wave();  // the next step overwrites the slice
      out += T;
    }
    carry += rdlane(incl, kWave - 1);
  }
}

__global__ __launch_bounds__(256) void props_at_kernel(PosArgs a) {
  const int w = threadIdx.x / kWave;
  const int l = lane_id();
  const uint32_t qi = blockIdx.x * kQueriesPerBlock + (uint32_t)w;
  if (qi >= a.n) return;
  const mte_pos_query q = a.q[qi];
  const uint32_t doc = uni(q.doc);
  const int32_t pos = uni(q.pos);
  const int32_t status = a.hdr[doc].status;
  int n = status == MTE_OK ? a.hdr[doc].nseg : 0;
  n = n < 0 ? 0 : (n > (int)a.cap ? (int)a.cap : n);
  const uint64_t db = (uint64_t)doc * a.cap;

  int32_t hit_slot = -1, carry = 0;
  uint32_t hit_kind = 0;
  for (int c0 = 0; c0 < n; c0 += kWave) {
    if (carry > pos) break;
    const int i = c0 + l;
    const bool vis = i < n && a.soa.rseq[db + i] == kNone;
    const int32_t L = vis ? a.soa.len[db + i] : 0;
    const uint32_t kind = vis ? a.soa.meta[db + i] >> 8 : 0u;
    const int32_t incl = wave_incl_scan(L);
    const int32_t P = carry + incl - L;
    const unsigned long long b = __ballot(L > 0 && P <= pos && pos < P + L);
    if (b) {
      const int s = __builtin_ctzll(b);
      hit_kind = rdlane(kind, s);
      hit_slot = c0 + s;
      break;
    }
    carry += rdlane(incl, kWave - 1);
  }
  if (l == 0) {
    mte_pos_hit h;
    h.status = status;
    h.found = hit_slot >= 0;
    h.kind = hit_kind;
    h.reserved = 0;
    a.out[qi] = h;
  }
  if (a.out_props && (uint32_t)l < a.n_keys)
    a.out_props[(uint64_t)qi * a.n_keys + l] =
        hit_slot >= 0 ? a.soa.props[(uint64_t)l * a.soa.plane_stride + db + hit_slot] : 0u;
}

__global__ __launch_bounds__(256) void ref_positions_kernel(RefArgs a) {
  const int w = threadIdx.x / kWave;
  const int l = lane_id();
  const uint32_t ti = blockIdx.x * kQueriesPerBlock + (uint32_t)w;
  if (ti >= a.n_tasks) return;
  const uint4 t = a.tasks[ti];
  const uint32_t qi = uni(t.x), blk = uni(t.y);
  const uint64_t out0 = uni64((uint64_t)t.z | ((uint64_t)t.w << 32));
  const mte_ref_query q = a.q[qi];
  const uint32_t doc = uni(q.doc), count = uni(q.count);
  const bool transient = (uni(q.flags) & MTE_REFS_TRANSIENT) != 0;
  const DocHdr h = a.hdr[doc];
  int n = h.status == MTE_OK ? h.nseg : 0;  // a stopped document answers -1 (and length 0)
  n = n < 0 ? 0 : (n > (int)a.cap ? (int)a.cap : n);
  const uint64_t db = (uint64_t)doc * a.cap;
  const bool want_pos = a.pos != nullptr, want_order = a.order != nullptr;

  const uint32_t s = blk * (uint32_t)kWave + (uint32_t)l;  // < count <= ref_cap - first
  const bool mine = s < count;
  const uint2 rt = mine ? a.refs[(uint64_t)doc * a.ref_cap + uni(q.first) + s] : make_uint2(0u, 0u);
  const bool live = (rt.y & kRefLive) != 0;
  const bool trans = live && (rt.y & kRefTrans);
  // what the lane still looks for (want): bit 0 the segment holding its unit,
  // for the position (up), the order key (uo) or both; bit 1 its Transient
  // slot's leaf
  const bool up = want_pos && live && !trans && !((rt.y & kRefDetached) && !(transient && (rt.y & kRefOff)));
  const bool uo = want_order && live && !((rt.y & kRefDetached) && !(rt.y & kRefOff));
  uint32_t want = ((up || uo) ? 1u : 0u) | ((want_pos && trans) ? 2u : 0u);
  const bool any_trans = __ballot(want & 2u) != 0;
  // the tree words, for the leaf ids: zeros for a document without them, as the host reads them
  const bool tree = doc_has_tree(h.flags) && any_trans;
  const bool lead = blk == 0;  // this wave also answers info, so it walks to the end

  int32_t pos = -1, carry = 0;
  int64_t key = -1, ocarry = 0;
  for (int c0 = 0; c0 < n; c0 += kWave) {
    const bool look = __ballot(want != 0) != 0;
    if (!look && !lead) break;
    const int i = c0 + l;
    const bool in = i < n;
    const int32_t rs = in ? a.soa.rseq[db + i] : kNone;
    const int32_t L = in ? a.soa.len[db + i] : 0;
    const int32_t V = rs == kNone ? L : 0;
    const int32_t vincl = wave_incl_scan(V);
    if (look) {
      const uint32_t to = in ? a.soa.toff[db + i] : 0u;
      const uint32_t tw = (in && tree) ? a.tree[db + i] : 0u;
      const int32_t P = carry + vincl - V;
      const int32_t O = want_order ? wave_incl_scan(L) - L : 0;  // below 2^31: the units are distinct arena units
      const unsigned long long head = __ballot(!(tw & (kTCont | kTEmpty)));
      const uint32_t id = (tw >> 8) & (kIdLimit - 1u);
      const int m = n - c0 < kWave ? n - c0 : kWave;
      // the step's segments, broadcast in document order: the first that holds
      // the lane's unit (ju), the head of its leaf (jt)
      int ju = -1, jt = -1;
      for (int j = 0; j < m; j++) {
        if (__ballot(want != 0) == 0) break;
        const uint32_t d = rt.x - rdlane(to, j);
        const bool hu = ((want & 1u) != 0) & (d < (uint32_t)rdlane(L, j));  // & not &&: no branch round a compare
        ju = hu ? j : ju;
        want = hu ? want & ~1u : want;
        if (any_trans) {
          const bool ht = ((want & 2u) != 0) & (((head >> j) & 1ull) != 0) & (rdlane(id, j) == rt.x);
          jt = ht ? j : jt;
          want = ht ? want & ~2u : want;
        }
      }
      // each lane pulls its segment's words (every lane takes part in the pull)
      const int pu = (ju < 0 ? 0 : ju) << 2;
      const uint32_t d = rt.x - (uint32_t)__builtin_amdgcn_ds_bpermute(pu, (int32_t)to);
      const int32_t Pu = __builtin_amdgcn_ds_bpermute(pu, P);
      const bool gone_u = __builtin_amdgcn_ds_bpermute(pu, rs) != kNone;
      if (ju >= 0 && up) pos = Pu + (gone_u ? 0 : (int32_t)d);
      if (want_order) {
        const int32_t Ou = __builtin_amdgcn_ds_bpermute(pu, O);
        if (ju >= 0 && uo) key = ocarry + (int64_t)Ou + (int64_t)d;
        ocarry += (int64_t)rdlane(O + L, kWave - 1);
      }
      if (any_trans) {
        const int pt = (jt < 0 ? 0 : jt) << 2;
        const int32_t Pt = __builtin_amdgcn_ds_bpermute(pt, P);
        const bool gone_t = __builtin_amdgcn_ds_bpermute(pt, rs) != kNone;
        if (jt >= 0) pos = Pt + (gone_t ? 0 : (int32_t)(rt.y & kRefTransOff));
      }
    }
    carry += rdlane(vincl, kWave - 1);
  }
  if (mine) {
    if (want_pos) a.pos[out0 + l] = pos;
    if (want_order) a.order[out0 + l] = key;
  }
  if (lead && l == 0) {
    mte_ref_info* o = a.info + qi;
    o->status = h.status;
    o->cur_seq = h.cur_seq;
    o->min_seq = h.min_seq;
    o->length = (uint32_t)carry;
    o->offset = out0;
  }
}

// ---- mte_read_segment_lists ---------------------------------------------------
constexpr int32_t kSegGranularity = 256;  // TextSegmentGranularity (textSegment.ts)

__device__ __forceinline__ int top_lane(unsigned long long b) { return 63 - __builtin_clzll(b); }
__device__ __forceinline__ uint32_t pull(int lane, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(lane << 2, (int32_t)v);
}

// The walk both kernels run, so they agree slot for slot.  Per 64-slot step a
// slot is valid (it gives something to the raw list), a head (it opens a raw
// segment) or a follower (a kTCont slot behind a head), kept (the mode keeps its
// raw segment) and, a kept head, the start of an output row or joined to the row
// before it.  The class word w of a lane: bit 0 kept, bit 1 eligible, bits 2..
// the kind; a follower takes its head's.
template <bool GATHER>
__device__ __forceinline__ void segs_walk(const SegsArgs& a, uint32_t qi, int l, uint2* st) {
  const mte_segs_query q = a.q[qi];
  const uint32_t doc = uni(q.doc), mode = uni(q.mode);
  const DocHdr h = a.hdr[doc];
  const int32_t dmin = uni(h.min_seq);
  const int32_t m = (uni(q.flags) & MTE_SEGS_DOC_MIN_SEQ) ? dmin : uni(q.min_seq);
  const uint32_t hflags = uni(h.flags);
  int n = h.status == MTE_OK ? h.nseg : 0;
  n = uni(n < 0 ? 0 : (n > (int)a.cap ? (int)a.cap : n));
  uint64_t so = 0, to = 0;
  if constexpr (GATHER) {
    const mte_segs_info* o = a.info + qi;
    if (uni(o->status) != MTE_OK || uni(o->n_segs) == 0u) return;  // the count refused it, or nothing to write
    so = uni64(o->seg_offset);
    to = uni64(o->text_offset);
  }
  const uint64_t db = (uint64_t)doc * a.cap;
  const bool tree = doc_has_tree(hflags);
  const bool rmhi = (hflags & (MTE_DOC_LOCAL_CLIENT | MTE_DOC_TREE)) != 0 && a.rm_hi != nullptr;
  const bool lazy = a.lazy != 0 && !tree;
  const bool coal = mode != MTE_SEGS_RAW, legacy = mode == MTE_SEGS_LEGACY;
  const int nk = (int)a.n_keys;
  const unsigned long long me = 1ull << l, lt = me - 1;

  // carried from step to step, wave-uniform
  bool any = false;     // a raw segment was opened
  bool keep_a = false;  // the open raw segment is kept
  uint32_t bw = 0, blast = 0, bp[MTE_MAX_KEYS] = {};  // the last kept slot: class word, last unit, property row
  int32_t run = 0;       // kept units since the head of the soft run
  uint32_t nrows = 0, ntext = 0;
  int32_t open_len = 0;  // units of row nrows - 1 so far
  bool bad = false;

  for (int c0 = 0; c0 < n; c0 += kWave) {
    const int i = c0 + l;
    const bool in = i < n;
    const uint32_t tw = (in && tree) ? a.tree[db + i] : 0u;
    const int32_t rs = in ? a.soa.rseq[db + i] : kNone;
    const int32_t sq = in ? a.soa.seq[db + i] : 0;
    const int32_t L = in ? a.soa.len[db + i] : 0;
    const uint32_t meta = in ? a.soa.meta[db + i] : 0u;
    const uint32_t toff = in ? a.soa.toff[db + i] : 0u;
    if constexpr (!GATHER)
      if (rmhi) bad |= in && a.rm_hi[db + i] != 0u && !(tw & kTEmpty) && rs != kNone;
    const bool valid = in && !(tw & kTEmpty) && !(lazy && rs != kNone && rs <= dmin);
    const unsigned long long bv = __ballot(valid);
    const bool head = valid && (!(tw & kTCont) || (!any && (bv & lt) == 0));
    const unsigned long long bh = __ballot(head);
    const uint32_t kind = meta >> 8;
    bool keep = true, elig = false;
    if (coal) {
      keep = legacy ? (sq <= m && rs > m) : !(rs != kNone && rs <= m);
      elig = legacy ? keep : (rs == kNone && sq <= m);
    }
    uint32_t w = (keep ? 1u : 0u) | (elig ? 2u : 0u) | (kind << 2);
    uint32_t p[MTE_MAX_KEYS];
#pragma unroll
    for (int k = 0; k < MTE_MAX_KEYS; k++)
      p[k] = (k < nk && head && (coal || GATHER)) ? a.soa.props[(uint64_t)k * a.soa.plane_stride + db + i] : 0u;

    // a raw segment's units past this step (its kTCont slots there): the length rule asks for all of them
    int32_t ext = 0;
    if (coal && tree && bh) {
      for (int c1 = c0 + kWave; c1 < n; c1 += kWave) {
        const int j = c1 + l;
        const uint32_t t2 = j < n ? a.tree[db + j] : kTEmpty;
        const int32_t l2 = j < n ? a.soa.len[db + j] : 0;
        const bool v2 = !(t2 & kTEmpty);
        const unsigned long long stop = __ballot(v2 && !(t2 & kTCont));
        const unsigned long long before = stop ? ((stop & (~stop + 1ull)) - 1ull) : ~0ull;
        ext += rdlane(wave_incl_scan((v2 && (before & me)) ? l2 : 0), kWave - 1);
        if (stop) break;
      }
    }

    // a follower takes its head's class (and, where rows are compared, its property row)
    const bool follower = valid && !head;
    {
      const unsigned long long hb = bh & lt;
      const int hl = hb ? top_lane(hb) : 0;
      const uint32_t wh = pull(hl, w);
      if (follower) w = hb ? wh : (keep_a ? bw : 0u);
      if (coal) {
#pragma unroll
        for (int k = 0; k < MTE_MAX_KEYS; k++)
          if (k < nk) {
            const uint32_t ph = pull(hl, p[k]);
            if (follower) p[k] = hb ? ph : bp[k];
          }
      }
    }
    const bool kept = valid && (w & 1u);
    const bool e = (w & 2u) != 0;
    const uint32_t ekind = w >> 2;
    const unsigned long long bk = __ballot(kept);
    const bool gives = kept && (head ? kind == 0 : true);  // units for `text`
    uint32_t last = 0;
    if (coal && kept && ekind == 0 && L > 0) last = a.arena[toff + (uint32_t)(L - 1)];

    // the kept slot before this one: soft = joined to it by every condition but the length one
    bool soft = false;
    if (coal) {
      const unsigned long long kb = bk & lt;
      const int pl = kb ? top_lane(kb) : 0;
      uint32_t pw = pull(pl, w), plast = pull(pl, last);
      if (!kb) pw = bw, plast = blast;
      bool same = true, uneq = false;
#pragma unroll
      for (int k = 0; k < MTE_MAX_KEYS; k++)
        if (k < nk) {
          const uint32_t pk = pull(pl, p[k]);
          same = same && (kb ? pk : bp[k]) == p[k];
          uneq = uneq || (p[k] & MTE_VALUE_UNEQUAL);
        }
      soft = kept && head && e && (pw & 3u) == 3u && ekind == 0 && (pw >> 2) == 0 && plast != 0x0Au && same && !uneq;
    }
    const int32_t KL = kept ? L : 0;
    const int32_t kin = wave_incl_scan(KL);
    const int32_t S = kin - KL;
    const int32_t total = rdlane(kin, kWave - 1);
    const bool rh = kept && head && !soft;  // the head of a soft run
    const unsigned long long brh = __ballot(rh);
    bool brk = false;
    if (coal) {
      // the raw segment's length: to the next head, or past the step's end
      int32_t rawlen = L;
      if (tree) {
        const int32_t VL = valid ? L : 0;
        const int32_t vin = wave_incl_scan(VL);
        const unsigned long long ha = bh & ~(lt | me);
        const int32_t vnh = (int32_t)pull(ha ? __builtin_ctzll(ha) : 0, (uint32_t)(vin - VL));
        rawlen = (ha ? vnh : rdlane(vin, kWave - 1) + ext) - (vin - VL);
      }
      const unsigned long long rb = brh & (lt | me);
      const int32_t Sh = (int32_t)pull(rb ? top_lane(rb) : 0, (uint32_t)S);
      const int32_t d = rb ? S - Sh : run + S;  // S(i) - S(h)
      brk = soft && rawlen > kSegGranularity && d > kSegGranularity;
    }
    const bool start = kept && head && (!soft || brk);
    const unsigned long long bs = __ballot(start);
    const int32_t TL = gives ? L : 0;
    const int32_t tin = wave_incl_scan(TL);
    const int32_t T = rdlane(tin, kWave - 1);

    if constexpr (GATHER) {
      const uint32_t rmask = (start && rs != kNone) ? a.soa.rmask[db + i] : 0u;
      const unsigned long long sa = bs & ~(lt | me);
      const int32_t Snx = (int32_t)pull(sa ? __builtin_ctzll(sa) : 0, (uint32_t)S);
      if (start) {
        const uint64_t r = so + nrows + (uint32_t)__builtin_popcountll(bs & lt);
        mte_seg* row = a.segs + r;
        const bool info_kept = !coal || (!e && sq > m);  // seq and client stay
        row->text_off = kind == 0 ? ntext + (uint32_t)(tin - TL) : 0u;
        if (sa) row->len = (uint32_t)(Snx - S);
        row->seq = info_kept ? sq : 0;
        row->removed_seq = e ? MTE_NOT_REMOVED : rs;  // kNone is MTE_NOT_REMOVED
        row->removers = e ? 0u : rmask;
        row->client = info_kept ? (int32_t)(meta & 0xffu) - 1 : -1;
        row->kind = kind;
        row->propset = MTE_NO_PROPS;
#pragma unroll
        for (int k = 0; k < MTE_MAX_KEYS; k++)
          if (k < nk) a.props[r * (uint64_t)nk + k] = p[k];
      }
      // the row open since an earlier step closes at this step's first start
      if (bs && nrows > 0 && (bs & lt) == 0 && start) a.segs[so + nrows - 1].len = (uint32_t)(open_len + S);
      if (T > 0) {
        uint16_t* out = a.text + to + ntext;
        st[l] = make_uint2((uint32_t)(tin - TL), toff);
        query_fence_wave();
        for (int32_t j = l; j < T; j += kWave) {
          int s = 0;  // the last slot whose exclusive sum is <= j: the giving one (text_gather_kernel)
#pragma unroll
          for (int b = kWave / 2; b > 0; b >>= 1)
            if ((int32_t)st[s + b].x <= j) s += b;
          const uint2 x = st[s];
          out[j] = a.arena[x.y + (uint32_t)(j - (int32_t)x.x)];
        }
        query_fence_wave();  // the next step overwrites the slice
      }
    }

    if (bs) open_len = total - rdlane(S, top_lane(bs));
    else open_len += total;
    nrows += (uint32_t)__builtin_popcountll(bs);
    ntext += (uint32_t)T;
    if (brh) run = total - rdlane(S, top_lane(brh));
    else run += total;
    if (bk) {
      const int lk = top_lane(bk);
      bw = rdlane(w, lk);
      blast = rdlane(last, lk);
      if (coal) {
#pragma unroll
        for (int k = 0; k < MTE_MAX_KEYS; k++)
          if (k < nk) bp[k] = rdlane(p[k], lk);
      }
    }
    if (bv) {
      keep_a = (rdlane(w, top_lane(bv)) & 1u) != 0;
      any = true;
    }
  }
  if constexpr (GATHER) {
    if (nrows > 0 && l == 0) a.segs[so + nrows - 1].len = (uint32_t)open_len;
  } else {
    const bool refused = __ballot(bad) != 0;  // mte_read_segments refuses the document
    if (l == 0) {
      mte_segs_info* o = a.info + qi;  // the offsets are the host's
      o->status = refused ? MTE_E_UNSUPPORTED : h.status;
      o->cur_seq = h.cur_seq;
      o->min_seq = h.min_seq;
      o->n_segs = refused ? 0u : nrows;
      o->n_text = refused ? 0u : ntext;
      o->reserved = 0;
    }
  }
}

__global__ __launch_bounds__(256) void segs_count_kernel(SegsArgs a) {
  const uint32_t qi = blockIdx.x * kQueriesPerBlock + threadIdx.x / kWave;
  if (qi >= a.n) return;
  segs_walk<false>(a, qi, lane_id(), nullptr);
}

__global__ __launch_bounds__(256) void segs_gather_kernel(SegsArgs a) {
  __shared__ uint2 stage[kQueriesPerBlock][kWave];  // (exclusive sum, arena offset)
  const uint32_t qi = blockIdx.x * kQueriesPerBlock + threadIdx.x / kWave;
  if (qi >= a.n) return;
  segs_walk<true>(a, qi, lane_id(), stage[threadIdx.x / kWave]);
}

}  // namespace mte
