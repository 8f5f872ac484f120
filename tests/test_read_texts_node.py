"""The batched read-outs through the Node host (fluidframework_amd/node):
MergeTreeEngine.getTexts and getPropertiesAt over the golden replay fixtures
after their last round, against BatchClient.getText / getTextWithPlaceholders /
getPropertiesAtPosition document by document and against the fixtures' expected
texts; and the addon built over the CPU restatement, whose library has neither
call: it still loads and both throw MTE_E_UNSUPPORTED."""
import json
import os
import shutil
import subprocess

import pytest

from fixtures_util import load_fixtures
from fluidframework_amd.abi import MTE_E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.mark.gpu
def test_node_get_texts_and_properties_at_equal_batch_client():
    r = subprocess.run([NODE, "tests/node/read_texts_gpu.js"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    fx = load_fixtures()
    assert got["texts"] == got["expected"] == [f["rounds"][-1]["resultText"] for f in fx] and len(fx) == 30
    assert got["textMismatches"] == 0 and got["textQueries"] > 2000
    assert got["posMismatches"] == 0 and got["posQueries"] > 1000 and got["withProps"] > 100
    assert "not for a client of this engine" in got["foreignText"]
    assert "not for a client of this engine" in got["foreignPos"]
    assert got["own"] == ["bc"] and got["empty"] == [[], []]


def test_restatement_addon_loads_and_the_batched_read_outs_are_unsupported():
    js = """
const addon = require("./oracle/_build/mte_napi_oracle.node");
const { MergeTreeEngine } = require("./fluidframework_amd/node");
const eng = new MergeTreeEngine({ nKeys: 8, addon });
const c = eng.createClient("hello", { newLengthCalc: true });
const out = { plain: c.getText(), text: null, pos: null, listed: Object.keys(addon).filter((k) => /readTexts|propsAt/.test(k)),
  has: [typeof addon.readTexts, typeof addon.propsAt] };
try { eng.getTexts([{ client: c }]); } catch (e) { out.text = e.code; }
try { eng.getPropertiesAt([{ client: c, pos: 1 }]); } catch (e) { out.pos = e.code; }
console.log(JSON.stringify(out));
eng.close();
"""
    r = subprocess.run([NODE, "-e", js], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == {"plain": "hello", "text": MTE_E_UNSUPPORTED, "pos": MTE_E_UNSUPPORTED, "listed": [],
                                    "has": ["function", "function"]}
