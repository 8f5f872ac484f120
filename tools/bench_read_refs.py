#!/usr/bin/env python3
"""Side measurement (not part of bench.py): every document's local reference
positions, Transient reads and order keys from one batched call against the
per-document read-outs.

State: `--docs` MTE_DOC_REFS documents (a local client each) loaded as `--segs`
segments of 1 .. 3 units, `--refs` live references a document (SlideOnRemove,
Simple and StayOnRemove by turns, spread over the text), then a few remote
removes a document, so that references slid, detached and sit on tombstones.
Three ways to the same answers:

  read_ref_positions      DeviceEngine.read_ref_positions(order=True) over two
                          queries a document (plain, Transient): one
                          mte_read_ref_positions call (one kernel, one
                          synchronisation) and the split into one array a query;
  read_ref_positions_raw  the device call alone, over query records packed
                          beforehand, the answers left as two flat arrays;
  per_document            what the engine offered before and still does:
                          read_refs, read_refs(transient=True) and read_ref_order
                          of each document (two synchronisations and the copies of
                          three planes, the tree words and the reference table a
                          call, the search on the host).

Each is warmed up, then timed `--repeats` times end to end on the host clock
(all end with the answers on the host); the median and the spread (min, max) are
reported, and the ratios of the medians.  The answers are asserted equal before
anything is timed.  Run it at --refs 64 and --refs 1024.  Prints one JSON line.

Usage: python3 tools/bench_read_refs.py [--docs 1000] [--segs 300] [--refs 64] [--repeats 15] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402

from fluidframework_amd.abi import (DOC_INIT_DTYPE, DOC_LOCAL_CLIENT, DOC_NEW_LENGTH_CALC, DOC_REFS,  # noqa: E402
                                    NO_PROPS, NOT_REMOVED, REF_QUERY_DTYPE, REF_SLIDE_ON_REMOVE, REF_STAY_ON_REMOVE,
                                    REFS_TRANSIENT, SEG_DTYPE)
from fluidframework_amd.engine import DeviceEngine  # noqa: E402
from fluidframework_amd.packing import BatchBuilder, DocClients, Interner  # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def build(n_docs, n_segs, n_refs):
    inits = np.zeros(n_docs, DOC_INIT_DTYPE)
    inits["flags"], inits["propset"] = DOC_NEW_LENGTH_CALC | DOC_LOCAL_CLIENT | DOC_REFS, NO_PROPS
    lens = 1 + np.arange(n_segs) % 3
    length = int(lens.sum())
    segs = np.zeros(n_docs * n_segs, SEG_DTYPE)
    segs["len"] = np.tile(lens, n_docs)
    segs["text_off"] = np.concatenate([[0], np.cumsum(segs["len"][:-1], dtype=np.uint64)]).astype(np.uint32)
    segs["removed_seq"], segs["client"], segs["propset"] = NOT_REMOVED, -1, NO_PROPS
    e = DeviceEngine(2)
    e.load_docs(inits, (0x100 + np.arange(n_docs * length) % 0x7000).astype(np.uint16))
    e.load_segments(np.arange(n_docs + 1, dtype=np.uint64) * n_segs, segs)
    it = Interner(2)
    types = (REF_SLIDE_ON_REMOVE, 0, REF_STAY_ON_REMOVE)
    bb = BatchBuilder(n_docs, it)
    for d in range(n_docs):
        cl = DocClients("A", local=True)
        for k in range(n_refs):
            bb.add_ref(d, cl, (k * 7919 + d) % length, types[k % 3])
        for s, p in enumerate(range(length - 30, 0, -length // 8)):  # eight remote removes, from the back
            bb.add_message(d, cl, {"clientId": "C", "sequenceNumber": s + 1, "referenceSequenceNumber": s,
                                   "minimumSequenceNumber": 0, "type": "op",
                                   "contents": {"type": 1, "pos1": p, "pos2": p + 12}})
    e.apply_batch(bb.build())
    assert (e.statuses() == 0).all()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--segs", type=int, default=300)
    ap.add_argument("--refs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    e = build(a.docs, a.segs, a.refs)
    docs, n = list(range(a.docs)), a.refs
    queries = [(d, 0, n, t) for d in docs for t in (False, True)]
    raw = np.array([(d, 0, n, REFS_TRANSIENT if t else 0) for d, _, _, t in queries], REF_QUERY_DTYPE)

    def read_ref_positions():
        return e.read_ref_positions(queries, order=True)

    def read_ref_positions_raw():
        return e.read_ref_positions_raw(raw, want_order=True)

    def per_document():
        return [(e.read_refs(d, n), e.read_refs(d, n, transient=True), e.read_ref_order(d, n)) for d in docs]

    pos, keys = read_ref_positions()
    want = per_document()
    for d in docs:
        assert (pos[2 * d] == want[d][0]).all() and (pos[2 * d + 1] == want[d][1]).all()
        assert (keys[2 * d] == want[d][2]).all() and (keys[2 * d + 1] == want[d][2]).all()
    flat = np.concatenate([w[0] for w in want])
    res = {"docs": a.docs, "segments_per_doc": int(len(e.read_segments(0)[0])), "refs_per_doc": n,
           "slots_read": int(raw["count"].sum()), "attached": int((flat >= 0).sum()), "detached": int((flat < 0).sum()),
           "read_ref_positions": timed(read_ref_positions, a.repeats, a.warmup),
           "read_ref_positions_raw": timed(read_ref_positions_raw, a.repeats, a.warmup),
           "per_document": timed(per_document, a.repeats, a.warmup)}
    res["per_document_over_read_ref_positions"] = \
        res["per_document"]["median_ms"] / res["read_ref_positions"]["median_ms"]
    res["per_document_over_read_ref_positions_raw"] = \
        res["per_document"]["median_ms"] / res["read_ref_positions_raw"]["median_ms"]
    print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
