#!/usr/bin/env python3
"""Golden Client.findTile answers from the REFERENCE merge-tree itself
(tests/golden/tile_vectors.json.gz).

Seeded generated streams (regenerated from their parameters by the tests:
fluidframework_amd/gen.py is deterministic) get tile labels on their marker
inserts (tests/tile_streams.py) and are replayed by tests/golden/ref_tiles.js
through the reference Client.  At four checkpoints per document (after each
quarter of its messages, cut on message ends like gen.cut_ops) the file records
the document's length, getTextWithPlaceholders and, for the labels pg, li, zz
and both directions, findTile's position (-1: undefined) for every start
position, run-length encoded: preceding for p in [0, length] and length + 5,
following for p in [0, length).  Data only, no reference source.

A document on which the reference throws is recorded with its error and left
out of the tests; more than 10 % of a set left out fails the generation.

Usage: python3 tests/golden/make_tile_golden.py
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from fluidframework_amd.messages import stream_docs  # noqa: E402
import ref_util  # noqa: E402
import tile_streams  # noqa: E402

OUT = os.path.join(HERE, "tile_vectors.json.gz")
DRIVER = os.path.join(HERE, "ref_tiles.js")
MAX_LEFT_OUT = 0.10
# config 3's mix (insert / remove / annotate), a marker every 4th insert, documents kept above 160 units
SETS = [
    ("newcalc_rounds", 3, 40, 600, dict(length_mode=2, marker_every=4, min_length=160)),
    ("newcalc_lag16", 3, 40, 600, dict(length_mode=2, marker_every=4, min_length=160, max_lag=16)),
    ("newcalc_lag64", 3, 40, 600, dict(length_mode=2, marker_every=4, min_length=160, max_lag=64)),
    ("legacy_rounds", 3, 40, 500, dict(length_mode=1, marker_every=4, min_length=160)),
    ("legacy_lag16", 3, 40, 500, dict(length_mode=1, marker_every=4, min_length=160, max_lag=16)),
]


def ref_tiles(docs):
    ref_util.build_ref()
    p = subprocess.run(["node", "--max-old-space-size=8192", DRIVER, ref_util.REF_OUT],
                       input=json.dumps({"labels": tile_streams.LABELS, "docs": docs}),
                       capture_output=True, text=True, timeout=3600)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-4000:])
    return json.loads(p.stdout)["docs"]


def main():
    if not ref_util.ref_available():
        sys.exit("the reference sources are not in this container")
    out = {"generator": "fluidframework_amd/gen.py (mte_gen.cpp), seeded MT19937; tests/tile_streams.py labels; "
                        "tests/golden/ref_tiles.js", "labels": tile_streams.LABELS, "sets": []}
    for name, cfg, nd, nops, kw in SETS:
        S = {"name": name, "config": cfg, "n_docs": nd, "ops_per_doc": nops, "params": kw}
        st = tile_streams.generate(S)
        _, cuts = tile_streams.checkpoints(st)
        docs = stream_docs(st, 0, nd, segs=False)
        for d, doc in enumerate(docs):
            doc["msgs"] = tile_streams.labelled_msgs(st, d)
            doc["cuts"] = [int(x) for x in cuts[d]]
        res = ref_tiles(docs)
        bad = [d for d, r in enumerate(res) if r["error"]]
        print(name, "left out:", [(d, res[d]["error"]) for d in bad], flush=True)
        if len(bad) > MAX_LEFT_OUT * nd:
            sys.exit(f"{name}: the reference threw on {len(bad)} of {nd} documents (> 10 %): "
                     "change the set's parameters or seeds")
        S["docs"] = [{"error": r["error"], "cps": r["cps"]} for r in res]
        out["sets"].append(S)
        print(name, sum(len(c["hits"]) for r in res for c in r["cps"]), "distinct hits", flush=True)
    with gzip.open(OUT, "wt", encoding="utf-8") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
