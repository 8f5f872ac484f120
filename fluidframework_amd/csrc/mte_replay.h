// mte_replay.h — the flat replay's register-tier kernels and the burst that
// drives a tier.  Top of the register layers (mte_docrun.h,
// mte_regdoc.h, the steps mte_step1.h and mte_step8.h); included by the units
// of pass 1 (mte_pass_pair.hip) and of passes 2 and 3 (mte_pass_flat.hip).
//
//   pair_kernel  — pass 1: `a.group` documents per wavefront (1 when the batch
//                  fits the chip at one per wave), E <= MTE_PASS1_EMAX (<= 254
//                  segments each at 4).  The wave runs its documents in turn,
//                  one burst each, so all documents of a 10k-doc batch are
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
#ifndef MTE_PAIR_WAVES  // pass-1 waves per SIMD the register budget is sized for (5: 96 VGPRs, 4: 128)
#define MTE_PAIR_WAVES 5
#endif
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

// DocRun <-> a DocHdr image in LDS (pass 1 keeps both documents of a pair
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

// pass 1: `a.group` documents per wavefront (1 when the batch fits the chip
// at one per wave), replayed in turn one burst each, so a 10k-document batch is
// resident on the chip at once with the register budget of one document
// (E <= 4); W = waves per SIMD the register budget is sized for.
//
// Fair issue between the waves sharing a SIMD: the SIMD arbiter favours the
// oldest wave, so with equal work per wave the youngest starves, then runs
// alone (latency-bound) at the end: measured on config 3 the pass-1 waves
// ended in five steps by dispatch order, 14.9 ms to 26.3 ms (tools/
// wave_clock.py).  After every burst the wave sets its priority (4 levels)
// from its progress against the schedule of the previous run, which keeps the
// waves of a SIMD abreast, so they finish together.
template <int K, bool S, int WPB, int W>
__global__ __launch_bounds__(WPB * kWave, W * 4 / WPB) void pair_kernel(ReplayArgs) {
  const ReplayArgs& a = args_in_place();
  __shared__ uint32_t zlds_all[WPB][kWave * 4];
  __shared__ DocHdr hl_all[WPB][kGroupMax];
  const int w = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int pair = (int)blockIdx.x * WPB + w;
  if (pair >= (int)a.n_pairs) return;
  if (a.wclock && lane_id() == 0) a.wclock[2 * pair] = __builtin_amdgcn_s_memrealtime();
  const int g = (int)a.group;
  DocHdr* hl = hl_all[w];
  uint32_t* zlds = zlds_all[w];
  uint32_t live = 0;  // bit t: document t still has ops to run in this pass
  uint32_t total = 0;  // ops of the group in this pass, and those left (for the issue priority)
  for (int t = 0; t < g; t++) {
    const int doc = (int)a.pair_docs[(uint32_t)g * (uint32_t)pair + (uint32_t)t];
    if (doc >= 0) {
      DocHdr h = a.hdr[doc];
      const bool rel = (h.flags & kHdrRel) != 0;  // the streamed pass's this batch
      if (!rel) h.flags &= ~kHdrNeedsEsc;
      if (lane_id() == 0) hl[t] = h;
      if (!rel) {
        live |= 1u << t;
        total += (uint32_t)(a.op_off[doc + 1] - a.op_off[doc]) - h.resume;
      }
    }
  }
  fence_wave();
  total = uni(total);
  uint32_t left = total;
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_setprio(2);
  // one burst per iteration, the documents in turn; a single copy of the
  // burst code serves them all (the document is a runtime index)
  for (int t = 0; live; t = (t + 1 == g) ? 0 : t + 1) {
    if (!(live & (1u << t))) continue;
    const int doc = (int)a.pair_docs[(uint32_t)g * (uint32_t)pair + (uint32_t)t];
    DocRun D;
    const uint32_t k0 = hl[t].resume;
    if (run_from_lds(D, &hl[t], doc, a)) pass1_burst<K, S>(D, a, zlds);
    run_to_lds(D, &hl[t]);
    if (!D.running) live &= ~(1u << t);
    const uint32_t ran = uni(hl[t].resume - k0);
    left -= ran;
    // against the schedule of the previous run (a.eta ticks for the whole
    // pass; a first run's is estimated from the batch, mte_run): behind it ->
    // higher priority
    if (a.eta) {
      const unsigned long long el = __builtin_amdgcn_s_memrealtime() - t_start;
      const unsigned long long mine = (unsigned long long)(total - left) * a.eta;  // done/total vs el/eta
      const unsigned long long sched = el * total;
      const unsigned long long band = (unsigned long long)total * a.eta / 32;
      if (mine + band < sched) __builtin_amdgcn_s_setprio(3);
      else if (mine < sched) __builtin_amdgcn_s_setprio(2);
      else if (mine < sched + band) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
  }
  if (lane_id() == 0) {
    for (int t = 0; t < g; t++) {
      const int doc = (int)a.pair_docs[(uint32_t)g * (uint32_t)pair + (uint32_t)t];
      if (doc >= 0) a.hdr[doc] = hl[t];  // resume = the op cursor
    }
    if (a.wclock) a.wclock[2 * pair + 1] = __builtin_amdgcn_s_memrealtime();
  }
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
