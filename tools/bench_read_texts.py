#!/usr/bin/env python3
"""Side measurement (not part of bench.py): every document's text from one
batched read_texts call against the per-document read-out.

State: as tools/bench_find_tile.py -- BASELINE config 2's size (1,000 documents
x 1,000 ops), config 3's markers (one insert in 16), labelled as the findTile
vectors are (tests/tile_streams.py).  Three ways to the same texts:

  read_texts      DeviceEngine.read_texts of every document: one mte_read_texts
                  call (a count kernel, a gather kernel, two synchronisations)
                  and the decoding of the units into Python strings;
  read_texts_raw  the device call alone, over query records packed beforehand,
                  the units left as one uint16 array;
  per_document    what the engine offered before: read_doc of each document (its
                  copies and stream synchronisations per document).

Each is warmed up, then timed `--repeats` times end to end on the host clock
(all end with the texts on the host); the median and the spread (min, max) are
reported, and the ratios of the medians.  The texts are asserted equal before
anything is timed.  Run it at two document counts (--docs 1000, --docs 250): the
batched call's time must not grow by a synchronisation per document.  Prints one
JSON line.

Usage: python3 tools/bench_read_texts.py [--docs 1000] [--ops 1000] [--repeats 15] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import tile_streams as ts  # noqa: E402
from fluidframework_amd.abi import TEXT_QUERY_DTYPE, TEXT_TO_END  # noqa: E402
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
    e = DeviceEngine(st["n_keys"])
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    docs = list(range(a.docs))
    raw = np.zeros(a.docs, TEXT_QUERY_DTYPE)
    raw["doc"], raw["end"] = docs, TEXT_TO_END

    def read_texts():
        return e.read_texts(docs)

    def read_texts_raw():
        return e.read_texts_raw(raw)

    def per_document():
        return [e.read_doc(d)["text"] for d in docs]

    texts = read_texts()
    assert texts == per_document()
    info, units = read_texts_raw()
    assert int(info["n_units"].sum()) == len(units) == sum(len(t) for t in texts)
    res = {"docs": a.docs, "ops_per_doc": a.ops, "segments_held_max": int(e.stats()["max_segs"]),
           "units": len(units), "units_per_doc_max": int(info["n_units"].max()),
           "read_texts": timed(read_texts, a.repeats, a.warmup),
           "read_texts_raw": timed(read_texts_raw, a.repeats, a.warmup),
           "per_document": timed(per_document, a.repeats, a.warmup)}
    res["per_document_over_read_texts"] = res["per_document"]["median_ms"] / res["read_texts"]["median_ms"]
    res["per_document_over_read_texts_raw"] = res["per_document"]["median_ms"] / res["read_texts_raw"]["median_ms"]
    print(json.dumps(res))
    e.close()


if __name__ == "__main__":
    main()
