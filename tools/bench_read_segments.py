#!/usr/bin/env python3
"""Side measurement (not part of bench.py): every document's V1 summary from one
batched segment-list read against the per-document summary writer.

State: config 3's op mix (inserts, removes, annotates, one marker in 16) over
1,000 documents with a collaboration window of 320 ops, 1,280 ops each, so a
document ends holding about 300 segments, most of them above its minSeq.  Four
ways over the same state:

  write_v1_all        snapshot.write_v1_all of every document: one
                      mte_read_segment_lists call (a count kernel, a gather
                      kernel, two synchronisations) and the blobs built from its
                      rows;
  write_v1_each       what the engine offered before: snapshot.write_v1 document
                      by document (mte_read_segments: a wait and a download of
                      every plane per document, then the drop-and-coalesce loop
                      in Python);
  segment_lists_raw   the device call alone, MTE_SEGS_RAW over query records
                      packed beforehand, rows, property rows and units left as
                      arrays;
  read_segments_each  read_segments of each document.

Each is warmed up, then timed `--repeats` times end to end on the host clock
(all end with their results on the host); the median and the spread (min, max)
are reported, and the ratios of the medians.  The blobs and the lists are
asserted equal before anything is timed.  Prints one JSON line.

Usage: python3 tools/bench_read_segments.py [--docs 1000] [--ops 1280] [--window 320] [--repeats 9] [--warmup 2]
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

from fluidframework_amd import gen, snapshot  # noqa: E402
from fluidframework_amd.abi import SEGS_DOC_MIN_SEQ, SEGS_QUERY_DTYPE, SEGS_RAW  # noqa: E402
from fluidframework_amd.engine import DeviceEngine  # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--ops", type=int, default=1280)
    ap.add_argument("--window", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    st = gen.generate(3, n_docs=a.docs, ops_per_doc=a.ops, round_ops=a.window)
    e = DeviceEngine(st["n_keys"])
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    docs = list(range(a.docs))
    raw = np.zeros(a.docs, SEGS_QUERY_DTYPE)
    raw["doc"], raw["mode"], raw["flags"] = docs, SEGS_RAW, SEGS_DOC_MIN_SEQ
    windows = [(v["min_seq"], v["cur_seq"]) for v in (e.read_doc(d) for d in docs)]

    def write_v1_all():
        return snapshot.write_v1_all(e, docs)

    def write_v1_each():
        return [snapshot.write_v1(e, d, *windows[d]) for d in docs]

    def segment_lists_raw():
        return e.read_segment_lists_raw(raw)

    def read_segments_each():
        return [e.read_segments(d) for d in docs]

    assert write_v1_all() == write_v1_each()
    info, segs, props, text = segment_lists_raw()
    each = read_segments_each()
    assert info["n_segs"].tolist() == [len(s) for s, _, _ in each]
    assert (segs == np.concatenate([s for s, _, _ in each])).all() and (text == np.concatenate([t for _, _, t in each])).all()
    rows_v1 = sum(len(s) for s, _, _ in e.read_segment_lists([(d, 1, None) for d in docs]))
    res = {"docs": a.docs, "ops_per_doc": a.ops, "window": a.window, "segments_held": int(len(segs)),
           "segments_held_per_doc_median": int(np.median(info["n_segs"])), "rows_v1": rows_v1, "units": int(len(text)),
           "write_v1_all": timed(write_v1_all, a.repeats, a.warmup),
           "write_v1_each": timed(write_v1_each, a.repeats, a.warmup),
           "segment_lists_raw": timed(segment_lists_raw, a.repeats, a.warmup),
           "read_segments_each": timed(read_segments_each, a.repeats, a.warmup)}
    res["write_v1_each_over_write_v1_all"] = res["write_v1_each"]["median_ms"] / res["write_v1_all"]["median_ms"]
    res["read_segments_each_over_segment_lists_raw"] = (res["read_segments_each"]["median_ms"]
                                                        / res["segment_lists_raw"]["median_ms"])
    print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
