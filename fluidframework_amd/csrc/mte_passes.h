// mte_passes.h — the host-device contract of the replay passes: their host
// launchers, the argument structs the launchers take and the layout constants
// both sides use.  Each pass lives in its own translation unit
// (mte_pass_tree.hip, mte_pass_htree.hip, mte_pass_flat.hip,
// mte_pass_chunk.hip) so the passes compile in parallel and one can be rebuilt
// alone; mte_engine.hip drives them (launch_replay) and includes no kernel
// header.  The pass headers include this one for the declarations below.  The
// batched read-only queries (mte_query.h, mte_query.hip) follow the same rule.
// Which pass replays a document is doc_owner() (mte_kernels.h), the one place
// where the routing rule lives; nothing here restates it.
#pragma once

#include <hip/hip_runtime.h>

#include "mte_kernels.h"

namespace mte {

// ---- the chunked pass (mte_chunk.h) -----------------------------------------
constexpr uint32_t kChunkMinCap = 8192;  // ctxs with a smaller capacity use pass 3 = stream_kernel
constexpr int kChE = 4;                  // slots per lane
constexpr int kChSlots = kWave * kChE;   // 256 slots per chunk
constexpr int kChFill = 128;             // segments per chunk after a re-layout
constexpr int kChGroup = 64;             // chunks per summary group
constexpr int kChWaves = 8;              // one document per 512-thread workgroup
constexpr uint32_t kChMaxGroups = 500;   // G in LDS: 32 x 500 x 4 B

struct ChunkArgs {
  uint32_t* arena;   // plane p, doc d, chunk i, slot j: arena[p * astride + (d * nch_cap + i) * 256 + j]
  uint64_t astride;
  uint32_t nch_cap;  // chunks per doc
  uint32_t ng_cap;   // groups per doc (<= kChMaxGroups)
  uint32_t* cnt;     // [doc][nch_cap] segments per chunk
  uint32_t* kc;      // [doc][nch_cap] re-layout scratch
  int32_t* sum;      // [doc][MTE_MAX_CLIENTS][nch_cap]
  // round phases (mte_round.h): with a plan, chunk_kernel replays only the
  // documents the plan sends op after op, up to their run's end
  const uint4* plan;      // [doc] x mode, y k0, z k1, w M (null: every escalated doc to its end)
  const uint32_t* rflag;  // [doc] non-zero: the round phases left the run to this pass
};

// the workgroup's control block, after the G columns in the launch's dynamic LDS
struct ChCtl {
  int32_t req, arg_c, arg_r;
  int32_t n;        // segments of the doc
  int32_t nch;      // chunks in use
  int32_t min_seq;  // for the re-layout's zamboni and the rebuilds
  int32_t status;
  int32_t part[kChWaves];
  int32_t rr[MTE_MAX_CLIENTS];  // refSeq each summary column is valid for
  int32_t pf_k;     // wave 0's current op (the prefetch wave runs ahead of it)
  int32_t pf_stop;  // wave 0 left its op loop
};

// ---- the tree pass (mte_tree.h) ---------------------------------------------
constexpr int kTreeHeapCap = 255;  // entries per document (+ the unused index 0)
constexpr uint32_t kHdrTreeEsc = 0x40000000u;  // tree pass: the document is TIER 1's (E = 4)
constexpr uint32_t kHdrTreeBig = 0x20000000u;  // tree pass: the document is TIER 2's (E = 8, 16)
constexpr uint32_t kHdrTreeHbmFlag = 0x10000000u;  // past TIER 2: the HBM tree pass (mte_htree.h kHdrTreeHbm)
// the tree word's bits (mte_tree.h describes the word)
constexpr uint32_t kTH = 0x7u, kTCont = 0x8u, kTNsShift = 4, kTNs = 0x30u, kTPo = 0x40u, kTEmpty = 0x80u;
constexpr uint32_t kTNl = 0x80000000u;
constexpr uint16_t kRecNl = 0x8000u;  // op record flag (engine-internal): the insert's text holds a '\n'
constexpr uint32_t kIdLimit = 1u << 23;

struct TreeArgs {
  uint32_t* tree;        // tree word of slot x of doc d: tree[d * cap + x]
  uint2* heap;           // doc d: heap[d * (kTreeHeapCap + 1) + k], k = 1 .. size
  const uint32_t* docs;  // the legacy documents
  uint32_t n_docs;
  const uint16_t* arena; // text (an append-merge looks at the last unit of a leaf)
  uint32_t final_round;  // TIER 1: keep documents that shrink (no return to TIER 0)
  uint32_t k_cap;        // this round's op cursor limit (TIER 0 / 1): documents advance together
};

// ---- the HBM tree pass (mte_htree.h) ----------------------------------------
constexpr int kHtState = 8;            // state words per document

// state words (HtreeArgs::st)
enum HtSt { kHsDepth = 0, kHsNextId, kHsHeapN, kHsLseq, kHsRhi, kHsEntered, kHsWin };

constexpr int kHtProf = 8;  // phase clocks of an MTE_HTREE_PROF build (mte_htree.h)

struct HtreeArgs {
  uint32_t* tree;        // tree words: tree[doc * cap + i]
  const uint2* rheap;    // the register tiers' heaps (kTreeHeapCap + 1 per doc): an escalating doc's
  uint2* heap;           // HBM tree heaps: heap[doc * (hcap + 1) + k], k = 1 .. hn
  uint32_t hcap;
  uint32_t lcap;         // items a document may hold in LDS (0: none; the launch's dynamic LDS)
  uint32_t* st;          // kHtState words per document
  int32_t* scr;          // L at scr[doc * 2 cap + i], P at scr[doc * 2 cap + cap + i]
  const uint32_t* docs;  // the documents this pass may replay
  uint32_t n_docs;
  const uint16_t* arena;
  unsigned long long* prof;  // kHtProf phase clocks (MTE_HTREE_PROF builds), or nullptr
  uint32_t maint;        // some document records maintenance (the htree_kernel<K, S, true> build)
};

// planes of a local-client / MTE_DOC_TREE document (mte_htree.h names them); the
// last is the removers of short ids 32 .. 63 (kRmHiPlane there).  As functions
// of K for the host, which has it at run time.
constexpr int local_planes(int K) { return kFieldPlanes + 3 * K + 6; }
constexpr int rm_hi_plane(int K) { return local_planes(K) - 1; }
template <int K> constexpr int kLocalPlanes = local_planes(K);

// ---- local references (MTE_DOC_REFS, include/mte.h; mte_hbm.h) --------------
// A reference is kept as the text unit it sits on -- its arena offset (a
// marker's is its reserved unit): splits never copy text, so the unit names the
// same place in whatever segment holds it, which is what LocalReferenceCollection
// keeps as (segment, offset) and moves on split (localReference.ts:391-416).
// kRefOff (with kRefDetached): a reference slideAckedRemovedSegmentReferences
// took off its segment's list for want of a segment to slide to
// (mergeTree.ts:935-942, removeLocalRef keeps the segment): detached for
// every read but mte_read_refs_transient, which still finds its segment.
constexpr uint32_t kRefLive = 0x80000000u, kRefDetached = 0x40000000u, kRefOff = 0x20000000u;
// a Transient reference (localReference.ts:263: never on its segment's list, so
// nothing moves or slides it): kRefLive | kRefDetached | kRefTrans | its offset
// in its segment, x = that segment's leaf id (mte_htree.h ht_ref_transient;
// titems.c REF_TRANS): read as its segment's position + the offset, the offset
// dropped once the segment is removed, -1 once the segment is gone
constexpr uint32_t kRefTrans = 0x10000000u, kRefTransOff = 0x0fffffffu;

// round phases of the chunked pass (mte_round.h)
constexpr int kRB = 62;              // sub-ops per chunk and run: 128 + 2 x 62 slots <= 254
constexpr uint32_t kRoundMin = 256;  // the shortest run the round phases take
constexpr int kMaxPhases = 16;       // phases per launch before the rest runs op after op
// a document's chunks stay laid out from one run to the next (rnd_live) while
// no chunk holds more than this many segments; a run whose sub-ops would not
// fit a carried chunk (count + 2 per sub-op > kChSlots) is re-laid out and run
// again in the next phase
constexpr uint32_t kLiveFull = 192;
struct RoundArgs {
  uint4* plan;      // [doc] x mode, y k0, z k1, w M
  uint32_t* rcnt;   // [doc][nch_cap] sub-ops per chunk
  uint2* rbuf;      // [doc][nch_cap][kRB] (op index - k0, chunk start in the op's perspective)
  uint4* rrec;      // [doc][nch_cap][kRB][2] the sub-op's record, copied there by the resolve (rnd_emit)
  uint32_t* rflag;  // [doc] non-zero: the run replays op after op
  uint32_t* nch;    // [doc] chunks after the re-layout
  uint32_t* nnew;   // [doc] segments after the re-layout
  uint32_t* count;  // [0] round docs, [1] op-after-op docs, [2] active docs
  uint2* rchain;    // [doc][MTE_MAX_CLIENTS] (list offset, entries) of each client chain
  // [doc] where the document's segments are: 0 the flat planes; 1 the chunk
  // arena, carried from the previous run (the flat planes are stale); 2 the
  // arena, re-laid out for this run
  uint32_t* live;
  uint32_t* gfl;    // [doc] 1: this launch gathers the arena back into the flat planes
  uint32_t last;    // this phase sends every active document op after op
  uint32_t col_cap; // chunks a resolve column holds (the phase's largest document, rounded to 64: rnd_plan's count[3])
  uint32_t d0, nd;  // the documents [d0, d0 + nd) one launch_round_run covers
  // [doc] the bytes the round phases of the last mte_run had to read and write
  // (their algorithmic bytes: records, planes re-laid out / applied /
  // gathered, sub-op lists), added per document and phase; planes = the
  // segment planes a move carries (kFieldPlanes + K)
  unsigned long long* acct;
  uint32_t planes;
};
// the round phases fit a context whose per-wave column (nch_cap + ng_cap
// entries, mte_round.h rnd_resolve_kernel) fits this much LDS
constexpr uint32_t kRoundLdsMax = 150u * 1024u;
// the documents leaving the arena (their next run is not a round, a chunk is
// full, or final: every one) gathered back into the flat planes
template <int K>
hipError_t launch_round_gather(const ReplayArgs& a, const ChunkArgs& ch, const RoundArgs& rd, int final,
                               hipStream_t s);
inline uint64_t rnd_resolve_lds(uint32_t nch_cap, uint32_t ng_cap) {
  return (uint64_t)(nch_cap + 2 * ((ng_cap + 63) / 64 * 64) + 64 + 1024) * 4u;  // + GD rows, the staging ring (kRing)
}

// the tree pass over the legacy documents (mte_tree.h): `rounds` of TIER 0
// (E <= 2) / TIER 1 (E = 4), then TIER 2 (E = 8, 16)
template <int K, bool S>
hipError_t launch_tree(const ReplayArgs& a, const TreeArgs& t, uint32_t blocks, hipStream_t s, int rounds,
                       uint32_t per_round);
// the HBM tree pass (mte_htree.h): one wavefront per candidate document
template <int K, bool S>
hipError_t launch_htree(const ReplayArgs& a, const HtreeArgs& t, hipStream_t s);
// pass 1 (one workgroup per pool of ReplayArgs::pools, `blocks` = n_pools) and
// pass 2 (one document per wavefront); pass1_waves(K, S) = the waves per SIMD
// that instantiation of pass 1 is built for, 5 or 6 (K as launch_pair takes it,
// kPack4 included): the host lays the pools out for it (pool_layout.h), so the
// batch is resident at once
template <int K, bool S>
hipError_t launch_pair(const ReplayArgs& a, uint32_t blocks, hipStream_t s);
int pass1_waves(int K, bool S);
constexpr int kPass1WavesMin = 5, kPass1WavesMax = 6;
template <int K, bool S>
hipError_t launch_big(const ReplayArgs& a, uint32_t blocks, hipStream_t s);
// pass 3: HBM-streamed (mte_stream.h) or chunked (mte_chunk.h)
template <int K, bool S>
hipError_t launch_stream(const ReplayArgs& a, uint32_t blocks, hipStream_t s);
template <int K, bool S>
hipError_t launch_chunk(const ReplayArgs& a, const ChunkArgs& ch, uint32_t n_docs, size_t lds, hipStream_t s);
// the round phases: plan, then (scatter, resolve, apply, gather) for the
// documents the plan gives a run
hipError_t launch_round_plan(const ReplayArgs& a, const ChunkArgs& ch, const RoundArgs& rd, uint32_t n_docs,
                             hipStream_t s);
template <int K>
hipError_t launch_round_run(const ReplayArgs& a, const ChunkArgs& ch, const RoundArgs& rd, uint32_t n_docs,
                            hipStream_t s);

// ---- batched queries (mte_query.h) ------------------------------------------
struct TileArgs {
  const DocHdr* hdr;
  SegSoA soa;
  uint32_t cap;
  uint32_t n_keys;
  uint32_t n;                  // queries; one wave each
  const mte_tile_query* q;     // validated by the host (doc, key, first + count)
  const uint32_t* values;
  mte_tile_hit* out;           // [n]
  uint32_t* out_props;         // [n][n_keys], or null
};
hipError_t launch_find_tiles(const TileArgs& a, hipStream_t s);

// mte_read_texts: text_count_kernel fills info (all but offset), the host sums
// the counts into offsets, text_gather_kernel copies the units
struct TextArgs {
  const DocHdr* hdr;
  SegSoA soa;
  uint32_t cap;
  uint32_t n;                  // queries; one wave each
  const mte_text_query* q;     // validated by the host (doc, start, end, flags)
  mte_text_info* info;         // [n] (count)
  const uint64_t* offset;      // [n] where each query's units start in text (gather)
  const uint16_t* arena;       // (gather)
  uint16_t* text;              // (gather)
};
hipError_t launch_text_count(const TextArgs& a, hipStream_t s);
hipError_t launch_text_gather(const TextArgs& a, hipStream_t s);

struct PosArgs {
  const DocHdr* hdr;
  SegSoA soa;
  uint32_t cap;
  uint32_t n_keys;
  uint32_t n;                  // queries; one wave each
  const mte_pos_query* q;      // validated by the host (doc, pos)
  mte_pos_hit* out;            // [n]
  uint32_t* out_props;         // [n][n_keys], or null
};
hipError_t launch_props_at(const PosArgs& a, hipStream_t s);

// mte_read_ref_positions: one wave per task = (query, block of 64 slots)
struct RefArgs {
  const DocHdr* hdr;
  SegSoA soa;
  uint32_t cap;
  const uint32_t* tree;        // the tree words; null in a context without tree documents
  const uint2* refs;
  uint32_t ref_cap;
  uint32_t n_tasks;
  const mte_ref_query* q;      // validated by the host (doc, MTE_DOC_REFS, first + count, flags)
  const uint4* tasks;          // x query | y slot block | z, w where the block's answers start (64 bits)
  mte_ref_info* info;          // [queries], written by each query's block 0
  int32_t* pos;                // or null
  int64_t* order;              // or null
};
hipError_t launch_ref_positions(const RefArgs& a, hipStream_t s);

// mte_read_segment_lists: segs_count_kernel fills info (all but the offsets),
// the host sums the counts into offsets and sends info back, segs_gather_kernel
// repeats the walk and writes rows, property rows and units
struct SegsArgs {
  const DocHdr* hdr;
  SegSoA soa;
  uint32_t cap;
  uint32_t n_keys;
  uint32_t n;                  // queries; one wave each
  uint32_t lazy;               // docs.rounds_carried: a flat document may hold tombstones at or below its minSeq
  const uint32_t* tree;        // the tree words; null in a context without tree documents
  const uint32_t* rm_hi;       // the removers of short ids 32 .. 63 (rm_hi_plane); null without such documents
  const mte_segs_query* q;     // validated by the host (doc, mode, min_seq, flags)
  mte_segs_info* info;         // [n]: written by the count, read (status, offsets) by the gather
  const uint16_t* arena;
  mte_seg* segs;               // (gather)
  uint32_t* props;             // (gather) [row][n_keys]
  uint16_t* text;              // (gather)
};
hipError_t launch_segs_count(const SegsArgs& a, hipStream_t s);
hipError_t launch_segs_gather(const SegsArgs& a, hipStream_t s);

}  // namespace mte
