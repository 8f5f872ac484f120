"""findTile through the Node host (fluidframework_amd/node): MergeTreeEngine.
findTiles, BatchClient.findTile and getTextWithPlaceholders against the
reference's answers (tests/golden/tile_vectors.json.gz, see
tests/test_find_tile.py), and the addon built over the CPU restatement, whose
library has no mte_find_tiles: it still loads and findTile throws
MTE_E_UNSUPPORTED."""
import json
import os
import shutil
import subprocess

import pytest

import tile_streams as ts
from fluidframework_amd.abi import MTE_E_UNSUPPORTED
from fluidframework_amd.messages import stream_docs
from test_find_tile import gold_set, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")
N_DOCS, SINGLE = 12, 2


@pytest.mark.gpu
def test_node_find_tiles_equal_reference():
    S = gold_set("newcalc_lag16")
    st = ts.generate(S)
    _, cuts = ts.checkpoints(st)
    docs = stream_docs(st, 0, N_DOCS, segs=False)
    for d, doc in enumerate(docs):
        doc["msgs"] = ts.labelled_msgs(st, d)
        doc["cuts"] = [int(x) for x in cuts[d]]
    r = subprocess.run([NODE, "tests/node/find_tile_gpu.js"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       input=json.dumps({"labels": golden()["labels"], "single": SINGLE, "docs": docs}))
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])["docs"]
    asked = 0
    for d in range(N_DOCS):
        assert not S["docs"][d]["error"]
        for k, (g, w) in enumerate(zip(got[d], S["docs"][d]["cps"])):
            assert g["length"] == w["length"] and g["text"] == w["text"] and g["sliceOk"], (d, k)
            want = {label: [ts.unrle(r) for r in w["q"][label]] for label in golden()["labels"]}
            assert g["q"] == want, (d, k)
            assert (g["single"] == want) if d < SINGLE else (g["single"] is None), (d, k)
            assert g["hits"] == [[p, pr, pr["markerId"], 1] for p, pr in w["hits"]], (d, k)
            asked += sum(len(x) for v in want.values() for x in v)
    assert asked > 10000


def test_restatement_addon_loads_and_find_tile_is_unsupported():
    js = """
const addon = require("./oracle/_build/mte_napi_oracle.node");
const { MergeTreeEngine } = require("./fluidframework_amd/node");
const eng = new MergeTreeEngine({ nKeys: 8, addon });
const c = eng.createClient("hello", { newLengthCalc: true });
c.applyMsg({ clientId: "B", sequenceNumber: 1, referenceSequenceNumber: 0, minimumSequenceNumber: 0, type: "op",
  contents: { type: 0, pos1: 2, seg: { marker: { refType: 1 }, props: { markerId: "x", referenceTileLabels: ["pg"] } } } });
const out = { text: c.getTextWithPlaceholders(), part: c.getTextWithPlaceholders(1, 4), plain: c.getText(),
  values: eng.interner.tileValues("pg"), code: null };
try { c.findTile(3, "pg"); } catch (e) { out.code = e.code; }
console.log(JSON.stringify(out));
eng.close();
"""
    r = subprocess.run([NODE, "-e", js], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout)
    assert out == {"text": "he llo", "part": "e l", "plain": "hello", "values": [1, [2]], "code": MTE_E_UNSUPPORTED}
