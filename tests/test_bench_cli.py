"""bench.py's command line: a plain run measures the headline alone, --full
adds the side blocks, --dump-outputs writes what the last timed step left for
its caller.  CPU: the dump's encoding, on the restatement (the engines share
read_doc / digest / statuses).  GPU: one small plain run and one small --full
run of the benchmark itself, the dumped digests checked against the
restatement's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fluidframework_amd import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DOCS, OPS = 64, 500


def _restatement():
    from oracle import OracleEngine
    s = gen.generate(3, n_docs=DOCS, ops_per_doc=OPS, n_threads=2, round_sync=True)
    o = OracleEngine(s["n_keys"], threads=2)
    gen.load_stream(o, s)
    o.apply_batch(s["batch"])
    return o


def _words(halves):
    """digests.npy (docs, 8) float64 halves -> (docs, 4) uint64."""
    h = halves.astype(np.uint64).reshape(len(halves), 4, 2)
    return h[:, :, 0] | (h[:, :, 1] << np.uint64(32))


def test_dump_outputs_encoding_is_exact(tmp_path):
    o = _restatement()
    d = tmp_path / "out"
    bench.dump_outputs(str(d), o, o.digest(), o.statuses())
    assert sorted(os.listdir(d)) == ["digests.npy", "statuses.npy", "text_sample.npy", "text_sample_docs.npy"]
    halves = np.load(d / "digests.npy")
    assert halves.dtype == np.float64 and halves.shape == (DOCS, 8)
    np.testing.assert_array_equal(_words(halves), o.digest())
    assert (o.digest() >> np.uint64(32)).any()  # the high halves carry data: a plain float64 cast would round
    np.testing.assert_array_equal(np.load(d / "statuses.npy"), o.statuses().astype(np.float64))
    docs, text = np.load(d / "text_sample_docs.npy"), np.load(d / "text_sample.npy")
    assert len(docs) == bench.DUMP_SAMPLE_DOCS == len(text) and len(set(docs.tolist())) == len(docs)
    for k, doc in enumerate(docs.astype(int)):
        want = np.frombuffer(o.read_doc(int(doc))["text"].encode("utf-16-le", errors="surrogatepass"), "<u2")
        np.testing.assert_array_equal(text[k, :len(want)], want)
        assert (text[k, len(want):] == -1).all()
    # the sample is fixed: a second dump picks the same documents
    bench.dump_outputs(str(tmp_path / "again"), o, o.digest(), o.statuses())
    np.testing.assert_array_equal(np.load(tmp_path / "again" / "text_sample_docs.npy"), docs)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--docs", str(DOCS), "--ops", str(OPS), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


SIDE_BLOCKS = ("roofline", "end_to_end", "end_to_end_node", "tree_placement", "local_client", "weak_scaling",
               "cpu_baseline", "cpu_baseline_reference", "parity_sample")


@pytest.mark.gpu
def test_gpu_plain_run_is_lean_and_dumps_the_timed_outputs(tmp_path):
    j = _bench("--dump-outputs", str(tmp_path))
    assert j["full"] is False and j["steps"] == 3 and j["warmup"] == 1
    assert all(j[k] is None for k in SIDE_BLOCKS), {k: j[k] for k in SIDE_BLOCKS if j[k] is not None}
    assert j["unit"] == "ops/s" and j["higher_is_better"] is True and j["dtype"] == "int32" and j["valid"] is True
    assert j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(j["config"]["ops_per_gpu"] / (j["ms_per_step"] * 1e-3), rel=1e-9)
    o = _restatement()
    np.testing.assert_array_equal(_words(np.load(tmp_path / "digests.npy")), o.digest())
    assert (np.load(tmp_path / "statuses.npy") == 0).all()
    docs, text = np.load(tmp_path / "text_sample_docs.npy"), np.load(tmp_path / "text_sample.npy")
    for k, doc in enumerate(docs.astype(int)):
        want = np.frombuffer(o.read_doc(int(doc))["text"].encode("utf-16-le", errors="surrogatepass"), "<u2")
        np.testing.assert_array_equal(text[k, :len(want)], want)


@pytest.mark.gpu
def test_gpu_full_run_keeps_the_side_blocks():
    j = _bench("--full", "--no-node-leg", "--local-docs", "614", "--cpu-seconds", "0.2")
    assert j["full"] is True and j["steps"] == 3
    assert j["roofline"]["kernel_ms"] > 0 and j["roofline"]["algo_bytes_per_launch"] > 0
    assert j["end_to_end"]["ms"] > 0
    assert j["tree_placement"]["digest_equal"] is True
    assert j["local_client"]["digest_equal_restatement"] is True
    assert j["parity_sample"]["digest_equal"] is True and j["cpu_baseline"]["value"] > 0
