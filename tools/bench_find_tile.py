#!/usr/bin/env python3
"""Side measurement (not part of bench.py): one batched find_tiles call against
the per-document path, for one findTile query per document.

State: BASELINE config 2's size (1,000 documents x 1,000 ops), with config 3's
markers (one insert in 16) labelled as the findTile vectors are
(tests/tile_streams.py).  Two ways to the same answers:

  batched       DeviceEngine.find_tiles: one upload, one kernel launch, one
                download for all documents (mte_find_tiles);
  per_document  what the engine offered before: read_doc of each document (its
                copies and a stream synchronisation per document) and the flat
                rule scanned on the host (tests/tile_model.py).

Each is warmed up, then timed `--repeats` times end to end on the host clock
(both end with the answers on the host); the median and the spread (min, max)
are reported, and the ratio of the medians.  `batched_raw` is the device call
alone, over query records packed beforehand; `read_docs_only` the per-document
read-outs alone, without decoding or scanning.  Prints one JSON line.

Usage: python3 tools/bench_find_tile.py [--docs 1000] [--ops 1000] [--repeats 15] [--warmup 3]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import tile_model  # noqa: E402
import tile_streams as ts  # noqa: E402
from fluidframework_amd.abi import TILE_PRECEDING, TILE_QUERY_DTYPE  # noqa: E402
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
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    S = {"config": 2, "n_docs": a.docs, "ops_per_doc": a.ops, "params": dict(marker_every=16)}
    st = ts.label_stream(ts.generate(S))
    it = ts.stream_interner(st)
    e = DeviceEngine(st["n_keys"])
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    rng = random.Random(1)
    lengths = [e.read_doc(d)["length"] for d in range(a.docs)]
    qs = [(d, rng.randint(0, max(lengths[d] - 1, 0)), "pg", rng.random() < 0.5) for d in range(a.docs)]

    def batched():
        return e.find_tiles(qs, it)

    key, ids = it.tile_values("pg")
    raw = np.zeros(len(qs), TILE_QUERY_DTYPE)
    for i, (d, p, _, pre) in enumerate(qs):
        raw[i] = (d, p, key, 0, len(ids), TILE_PRECEDING if pre else 0)

    def batched_raw():
        return e.find_tiles_raw(raw, ids)

    def per_document():
        out = []
        for d, p, label, pre in qs:
            h = tile_model.find_tile(tile_model.decoded_segs(e.read_doc(d), it), p, label, pre)
            out.append(None if h is None else {"pos": h[0], "refType": h[1], "props": h[2]})
        return out

    def read_docs_only():  # the per-document path's device part alone: no decoding, no scan
        return [e.read_doc(d)["length"] for d in range(a.docs)]

    assert batched() == per_document()
    res = {"docs": a.docs, "ops_per_doc": a.ops, "segments_held_max": int(e.stats()["max_segs"]),
           "found": sum(x is not None for x in batched()),
           "batched": timed(batched, a.repeats, a.warmup),
           "batched_raw": timed(batched_raw, a.repeats, a.warmup),
           "per_document": timed(per_document, a.repeats, a.warmup),
           "read_docs_only": timed(read_docs_only, a.repeats, a.warmup)}
    res["per_document_over_batched"] = res["per_document"]["median_ms"] / res["batched"]["median_ms"]
    print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
