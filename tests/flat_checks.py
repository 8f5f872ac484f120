"""Checks the GPU test modules of the flat passes share (tests/test_gpu_parity.py,
tests/test_gpu_flat_variants.py): pass 1's sizing and the state of a document
that runs out of capacity."""
import ctypes as C
import functools

import numpy as np

from fluidframework_amd import _native
from fluidframework_amd.abi import MTE_E_CAPACITY
from oracle import SpecOracle
from stream_edit import first_ops, nsegs_trace, ops_before_capacity


@functools.lru_cache(maxsize=None)
def cu_count():
    """The device's compute units, by the call mte_load_docs itself makes
    (hipDeviceGetAttribute) on the HIP runtime libmte.so runs on.  PyTorch's
    torch.cuda.get_device_properties(0).multi_processor_count is the same
    number, but a PyTorch build that brings its own HIP runtime may see no
    device where the engine's does ("No HIP GPUs are available"); where it does
    see one, the two are cross-checked, which also guards the enum value."""
    _native.load_mte()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    n = C.c_int(0)
    hipDeviceAttributeMultiprocessorCount = 63  # hip_runtime_api.h
    assert hip.hipDeviceGetAttribute(C.byref(n), hipDeviceAttributeMultiprocessorCount, 0) == 0
    assert 0 < n.value <= 1024
    try:
        import torch
        seen = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else None
    except (ImportError, RuntimeError, AssertionError):
        seen = None
    assert seen is None or seen == n.value
    return n.value


def resident_docs():
    """The flat documents pass 1 holds one per wave: CUs x 4 SIMDs x 5 waves
    (MTE_PAIR_WAVES, mte_replay.h; `resident` in mte_load_docs, mte_engine.hip).
    g = ceil(flat documents / resident), at most kGroupMax = 8, ride on a wave."""
    return cu_count() * 4 * 5


def assert_stopped_like_spec(stream, d, cap, streamed):
    """A flat document that runs out of capacity stops between two ops and
    keeps the state of the ops it took.  The restatement has no capacity, so
    the op it stops at comes from the restatement's segment counts n_k (before
    op k; one op adds at most two segments).  The register tiers and the
    chunked pass look before the op: they refuse the first op that finds fewer
    than two free segments (n_k + 2 > cap).  The streamed pass (`streamed`)
    looks after it: it refuses the first op that would leave fewer than two
    (n_k+1 + 2 > cap).  Neither stops an op earlier or later.  Statuses,
    digests, read-outs (cur_seq and min_seq among them) and segment lists then
    equal the specification's after exactly those ops."""
    assert (stream["inits"]["flags"] & 1).all()  # new length calc: the flat passes
    n_ops = np.diff(stream["batch"]["op_offsets"].astype(np.int64))
    took = ops_before_capacity(nsegs_trace(stream), cap, after=streamed)
    assert (took < n_ops).all()  # every document stops
    head = first_ops(stream, took)
    o = SpecOracle(stream["n_keys"], threads=8, cap=cap)
    o.load_docs(head["inits"], head["init_text"])
    o.apply_batch(head["batch"])
    assert (o.statuses() == 0).all()
    assert (d.statuses() == MTE_E_CAPACITY).all()
    np.testing.assert_array_equal(d.digest(), o.digest())
    for doc in range(len(n_ops)):
        assert dict(d.read_doc(doc), status=0) == o.read_doc(doc)
        for x, y in zip(d.read_segments(doc), o.read_segments(doc)):
            np.testing.assert_array_equal(x, y)
