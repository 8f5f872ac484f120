// mte_docrun.h — the per-document run state every replay pass uses: DocRun and
// its load / write-back (run_init, run_finish), the scalar op fetch, the
// statistics switch and the collab-window error.  Layer above mte_kernels.h;
// included by every pass header (mte_regdoc.h, mte_hbm.h, mte_chunk.h, mte_htree.h ...).
#pragma once

#include "mte_kernels.h"

namespace mte {

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

// number of set bits of m in the lanes below this one
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
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

}  // namespace mte
