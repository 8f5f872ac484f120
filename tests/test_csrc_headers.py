"""The device headers' layering (csrc/mte_*.h): every header compiles as a unit of
its own, and each translation unit reaches exactly the headers written out
below, so a new edge in the include graph is a decision made here, in sight.
Needs only hipcc (a syntax-only cross-compile for gfx950), no GPU."""
import glob
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidframework_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-std=c++17", "--offload-arch=gfx950"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")

# what every unit reaches (mte_kernels.h includes include/mte.h)
BASE = {"mte_kernels.h", "mte_passes.h"}
# the register layers: run state, register document, the two steps
REG = {"mte_docrun.h", "mte_regdoc.h"}
UNIT_HEADERS = {
    "mte_engine.hip": BASE,
    "mte_query.hip": BASE | {"mte_query.h"},
    # pass 1: the step of its tiers, and mte_step8.h for burst_run's doc_step
    "mte_pass_pair.hip": BASE | REG | {"mte_step1.h", "mte_step8.h", "mte_replay.h"},
    # passes 2 and 3: the same, and the HBM documents under stream_kernel
    "mte_pass_flat.hip": BASE | REG | {"mte_step1.h", "mte_step8.h", "mte_replay.h", "mte_hbm.h", "mte_stream.h"},
    # the chunk pass and the round phases share seg_op_v with pass 1; no flat kernel
    "mte_pass_chunk.hip": BASE | REG | {"mte_step1.h", "mte_chunk.h", "mte_round.h"},
    # the register tree: a register document and the tree word; no step, no flat kernel
    "mte_pass_tree.hip": BASE | REG | {"mte_treeword.h", "mte_tree.h"},
    # the HBM tree: run state, HBM documents, the tree word; no register document
    "mte_pass_htree.hip": BASE | {"mte_docrun.h", "mte_hbm.h", "mte_treeword.h", "mte_htree.h"},
}


def _pool(fn, items):
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(items, ex.map(fn, items)))


def test_every_header_compiles_alone(tmp_path):
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(CSRC, "mte_*.h")))
    assert len(headers) >= 15

    def alone(h):
        unit = tmp_path / (h + ".hip")
        unit.write_text('#include "%s"\n' % os.path.join(CSRC, h))
        r = subprocess.run([HIPCC, *FLAGS, "-fsyntax-only", str(unit)], capture_output=True, text=True)
        return r.stderr[-1500:] if r.returncode else ""

    failed = {h: err for h, err in _pool(alone, headers).items() if err}
    assert failed == {}


def test_units_reach_the_headers_listed_here():
    units = sorted(os.path.basename(u) for pat in ("mte_pass_*.hip", "mte_query.hip", "mte_engine.hip")
                   for u in glob.glob(os.path.join(CSRC, pat)))
    assert units == sorted(UNIT_HEADERS)

    def reached(u):
        out = subprocess.run([HIPCC, *FLAGS, "-MM", u], cwd=CSRC, capture_output=True, text=True, check=True).stdout
        deps = {os.path.basename(d) for d in re.split(r"[\s\\]+", out) if d.endswith(".h")}
        return {d for d in deps if d.startswith("mte_")}

    got = _pool(reached, units)
    assert got == {u: UNIT_HEADERS[u] for u in units}
