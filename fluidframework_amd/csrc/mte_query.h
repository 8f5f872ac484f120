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

}  // namespace mte
