// mte_replay.h — the flat replay's register-tier kernels and the burst that
// drives a tier.  Top of the register layers (mte_docrun.h,
// mte_regdoc.h, the steps mte_step1.h and mte_step8.h); included by the units
// of pass 1 (mte_pass_pair.hip) and of passes 2 and 3 (mte_pass_flat.hip).
//
//   pair_kernel  — pass 1: a workgroup per pool of documents (one document per
//                  wave when the batch fits the chip that way), E <=
//                  MTE_PASS1_EMAX (<= 254 segments each at 4).  The workgroup's
//                  waves run the pool's documents one burst at a time, whichever
//                  wave is free, so all documents of a 10k-doc batch are
//                  resident on the chip at once (one wave per doc would need
//                  10k resident waves; the chip holds 8 per SIMD).
//   big_kernel   — pass 2: one document per wavefront, E in {4, 8, 16}
//                  (<= 1022 segments), for documents pass 1 escalated.
//   stream_kernel — pass 3 (mte_stream.h): larger documents, HBM-resident.
//
// The tiers E >= 8 run the per-op step doc_step (mte_step8.h) on a
// register-resident document: op records (32 B, mte_kernels.h) are read with
// scalar loads straight into SGPRs (the op index is wave-uniform), the next
// op's record in flight while the current op runs, and a vector load touches
// the records ahead so the scalar loads hit L2.  The tiers E <= 4 run the
// per-slot-flag step (mte_step1.h): E <= 2 takes its records 64 at a time, one
// per lane, and decodes and window-checks them vector-wide (block_run); E = 4
// fetches each op's record with a vector load (doc_step_v).
#pragma once

#include <type_traits>

#include "mte_kernels.h"
#include "mte_docrun.h"
#include "mte_regdoc.h"
#include "mte_step1.h"
#include "mte_step8.h"

// Build-time knobs (tools/variants.sh builds A/B variants; defaults are the product build).
#ifndef MTE_BURST
#define MTE_BURST 128
#endif
#ifndef MTE_PASS1_EMAX  // largest pass-1 register tier (4, or 2: documents over 126 segments go to pass 2)
#define MTE_PASS1_EMAX 4
#endif

namespace mte {

constexpr uint32_t kBurst = MTE_BURST;  // ops per burst in pass 1
constexpr int kStepVEmax = 4;           // tiers up to this E run the per-slot-flag step (doc_step_v), larger ones doc_step

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

// DocRun <-> a DocHdr image in LDS (pass 1 keeps the documents of a pool
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

// pass 1: one workgroup per pool of documents (pool_layout.h).  A batch that
// fits the chip at one document per wave runs that way (pool_max <= WPB: wave w
// owns document w of its pool and nothing is shared).  A larger batch has more
// documents in a pool than the workgroup has waves, and any wave runs any of
// them, one burst at a time, so a 10k-document batch is resident on the chip at
// once with the register budget of one document (E <= 4) per wave and every
// wave slot filled; W = waves per SIMD the register budget is sized for.
//
// Between bursts a document lives in HBM (store_regs / load_regs) and its
// header in the pool's LDS images `hl`, so nothing ties it to a wave.  A wave
// claims a document with a compare-and-swap on the document's claim word in
// LDS (lane 0, the result made uniform), runs one burst and releases it:
//   - a document is held by at most one wave at a time;
//   - no wave ever waits for another: the claim is one bounded scan over the
//     pool from the wave's cursor, and a wave that finds no free document
//     exits.  Every document with ops left is then held by a running wave,
//     which offers it again after its burst and scans again itself (its own
//     document last), so nothing is left behind;
//   - the hand-off through HBM is a workgroup-scope release / acquire (the
//     waves of a workgroup share their CU's L1): after store_regs and
//     run_flush_stats the releasing wave fences, waits for its stores
//     (s_waitcnt vmcnt(0) in asm: the fence's own wait can be dropped by the
//     compiler) and only then stores the claim word; the claiming wave fences
//     after its compare-and-swap succeeded and before load_regs.  The segment
//     planes and the statistics are read by vector loads only (never through
//     the scalar cache, which no fence of this scope refreshes);
//   - the wave whose burst ends a document's part of the pass (ops done, a
//     status, kHdrNeedsEsc, or nothing to run at all) writes its header to
//     HBM.  A kHdrRel document is never started and its header in HBM is
//     already what pass 1 leaves, so nobody writes it.
//
// Fair issue between the waves sharing a SIMD: the SIMD arbiter favours the
// oldest wave, so with equal work per wave the youngest starves, then runs
// alone (latency-bound) at the end: measured on config 3 the pass-1 waves
// ended in five steps by dispatch order, 14.9 ms to 26.3 ms (tools/
// wave_clock.py).  Before every burst the wave sets its priority (4 levels)
// from the claimed document's progress against the schedule of the previous
// run, which keeps the documents abreast, so they finish together.
constexpr uint32_t kClaimFree = 0, kClaimHeld = 1, kClaimDone = 2;

template <int K, bool S, int WPB, int W>
__global__ __launch_bounds__(WPB * kWave, W * 4 / WPB) void pair_kernel(ReplayArgs) {
  const ReplayArgs& a = args_in_place();
  __shared__ uint32_t zlds_all[WPB][kWave * 4];
  __shared__ DocHdr hl[kPoolMax];
  __shared__ uint32_t k0s[kPoolMax];    // the op cursor at the kernel's entry (for the issue priority)
  __shared__ uint32_t claim[kPoolMax];  // kClaim*
  const int w = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t wave = blockIdx.x * WPB + (uint32_t)w;
  if (a.wclock && lane_id() == 0) a.wclock[2 * wave] = __builtin_amdgcn_s_memrealtime();
  // (made uniform by hand: the table is read by vector loads, and the pointer
  // would otherwise sit in a VGPR pair across the op loop)
  const uint32_t first = uni(a.pools[blockIdx.x]);
  const uint32_t n = min(uni(a.pools[blockIdx.x + 1]) - first, (uint32_t)kPoolMax);
  uint64_t docs_at = reinterpret_cast<uint64_t>(a.pools + a.n_pools + 1 + first);
  asm("" : "+s"(docs_at));
  const uint32_t* const docs = reinterpret_cast<const uint32_t*>(docs_at);
  // the pool's headers into LDS, one thread per document
  if (threadIdx.x < n) {
    const uint32_t t = threadIdx.x;
    DocHdr h = a.hdr[docs[t]];
    const bool rel = (h.flags & kHdrRel) != 0;  // the streamed pass's this batch
    if (!rel) h.flags &= ~kHdrNeedsEsc;
    hl[t] = h;
    k0s[t] = h.resume;
    claim[t] = rel ? kClaimDone : kClaimFree;
  }
  __syncthreads();
  uint32_t* zlds = zlds_all[w];
  const bool owned = a.pool_max <= (uint32_t)WPB;  // one document per wave
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_setprio(2);
  // one burst per iteration; a single copy of the burst code serves every
  // document (the document is a runtime index)
  uint32_t t = (uint32_t)w < n ? (uint32_t)w : 0u;  // the cursor
  bool more = owned ? (uint32_t)w < n && claim[w] == kClaimFree : n != 0;
  while (more) {
    if (!owned) {
      uint32_t got = n;
      for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = t + i < n ? t + i : t + i - n;
        uint32_t seen = kClaimHeld;
        if (lane_id() == 0) {
          seen = kClaimFree;
          __hip_atomic_compare_exchange_strong(&claim[c], &seen, kClaimHeld, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (uni(seen) == kClaimFree) {
          got = c;
          break;
        }
      }
      if (got == n) break;  // every document is done or held by a running wave
      t = got;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    const int doc = uni((int32_t)docs[t]);
    DocRun D;
    if (run_from_lds(D, &hl[t], doc, a)) {
      // against the schedule of the previous run (a.eta ticks for the whole
      // pass; a first run's is estimated from the batch, mte_run): the
      // document behind it -> higher priority for its burst
      if (a.eta) {
        const uint32_t k0 = uni(k0s[t]);
        const unsigned long long total = D.k1 - k0;
        const unsigned long long el = __builtin_amdgcn_s_memrealtime() - t_start;
        const unsigned long long mine = (unsigned long long)(D.k - k0) * a.eta;  // done/total vs el/eta
        const unsigned long long sched = el * total;
        const unsigned long long band = total * a.eta / 32;
        if (mine + band < sched) __builtin_amdgcn_s_setprio(3);
        else if (mine < sched) __builtin_amdgcn_s_setprio(2);
        else if (mine < sched + band) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      pass1_burst<K, S>(D, a, zlds);
    }
    run_to_lds(D, &hl[t]);
    if (!D.running && lane_id() == 0) a.hdr[doc] = hl[t];  // resume = the op cursor
    if (owned) {
      more = D.running;
    } else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane_id() == 0)
        __hip_atomic_store(&claim[t], D.running ? kClaimFree : kClaimDone, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
      t = t + 1 == n ? 0 : t + 1;
    }
  }
  if (a.wclock && lane_id() == 0) a.wclock[2 * wave + 1] = __builtin_amdgcn_s_memrealtime();
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
