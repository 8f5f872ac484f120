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

}  // namespace mte
