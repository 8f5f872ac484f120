"""Pass 1's document pools (pair_kernel, mte_replay.h; the layout, pool_layout.h):
a batch larger than the chip holds at one document per wave runs in pools, a
workgroup's waves taking turns on the pool's documents one burst (128 ops) at a
time, the document handed from wave to wave through HBM.  Every case is
bit-exact against the specification (SpecOracle): statuses, digests, the op
statistics, read-outs and the full segment lists of every document of the pools
it inspects (the helpers of tests/test_gpu_flat_variants.py).

The document counts come from the device: resident = CUs x 4 SIMDs x 6 waves
(the product instantiations' figure), `resident + 1` documents (pools of 5 and
4) and `2 x resident - 1` (pools of 8 and 7).  Where nothing else is said a
document has 400 ops: four bursts, so it changes hands at least twice.  The
instantiations built for five waves lay the same batches out in the same number
of pools or fewer, larger ones; either way every pool here holds more documents
than the workgroup has waves.

No case provokes a fault and none repeats a run to make one happen.
"""
import functools

import numpy as np
import pytest

import stream_edit as se
from flat_checks import cu_count
from fluidframework_amd import gen
from fluidframework_amd.abi import MTE_E_SEQ_ORDER
from fluidframework_amd.engine import DeviceEngine
from oracle import SpecOracle
from test_gpu_flat_variants import assert_same_state, device, spec

pytestmark = pytest.mark.gpu

WPB, POOL_CAP, BURST = 4, 32, 128
OPS = 400


def resident(waves=6):
    return cu_count() * 4 * waves


def pool_first(nf, waves=6):
    """pool_layout.h's rule, restated: first[] of the pools of nf flat documents."""
    res = resident(waves)
    pools = -(-nf // WPB) if nf <= res else max(res // WPB, -(-nf // POOL_CAP))
    q, r = divmod(nf, pools)
    return np.concatenate([[0], np.cumsum([q + (p < r) for p in range(pools)])]).astype(np.int64)


def pool_docs(nf, pools, waves=6):
    first = pool_first(nf, waves)
    return [d for p in pools for d in range(first[p], first[p + 1])]


def first_middle_last(nf, waves=6):
    n = len(pool_first(nf, waves)) - 1
    return [0, n // 2, n - 1]


def with_counts(stream, counts):
    """Documents -> op counts (the others keep OPS)."""
    n = np.full(len(stream["inits"]), OPS, np.int64)
    for d, c in counts.items():
        n[d] = c
    return se.first_ops(stream, n)


# ---- 1. even load -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def even_stream(nf):
    return gen.generate(3, n_docs=nf, ops_per_doc=OPS, length_mode=2)


@functools.lru_cache(maxsize=None)
def even_spec(nf):
    o = spec(even_stream(nf))
    assert (o.statuses() == 0).all()
    return o


@pytest.mark.parametrize("which", ["resident+1", "2*resident-1"])
def test_gpu_pools_even_load(which):
    nf = resident() + 1 if which == "resident+1" else 2 * resident() - 1
    sizes = np.diff(pool_first(nf))
    assert sizes.max() - sizes.min() == 1 and sizes.max() == (5 if which == "resident+1" else 8)
    # statistics on (assert_same_state compares the counters): case 5 too
    assert_same_state(even_spec(nf), device(even_stream(nf)), pool_docs(nf, first_middle_last(nf)))


# ---- 6., 7. resume and replay --------------------------------------------------

def test_gpu_pools_two_batches_on_one_context():
    # the second mte_run starts every document from the header the first left
    nf = resident() + 1
    s = even_stream(nf)
    parts = [gen.cut_ops(s, 0.0, 0.5), gen.cut_ops(s, 0.5, 1.0)]
    o, d = SpecOracle(s["n_keys"], threads=16), DeviceEngine(s["n_keys"])
    gen.load_stream(o, s)
    gen.load_stream(d, s)
    docs = pool_docs(nf, first_middle_last(nf))
    for p in parts:
        o.apply_batch(p)
        d.apply_batch(p)
        assert (o.statuses() == 0).all()
        assert_same_state(o, d, docs)
    np.testing.assert_array_equal(o.digest(), even_spec(nf).digest())


def test_gpu_pools_replay_gives_equal_digests():
    # which wave runs which burst differs from run to run; the result does not
    nf = 2 * resident() - 1
    s = even_stream(nf)
    d = device(s, stats=False)
    once = d.digest().copy()
    d.reset()
    d.run()
    d.sync()
    np.testing.assert_array_equal(d.digest(), once)
    np.testing.assert_array_equal(once, even_spec(nf).digest())
    assert (d.statuses() == 0).all()


# ---- 2. uneven load -------------------------------------------------------------

UNEVEN = [0, 1, BURST - 1, BURST, BURST + 1, 2000]


@functools.lru_cache(maxsize=None)
def long_stream(nf):
    """2,000 ops for every document; the cases cut all but a few to OPS."""
    return gen.generate(3, n_docs=nf, ops_per_doc=2000, length_mode=2)


def test_gpu_pools_uneven_load_in_one_pool():
    # documents of 0, 1, 127, 128, 129 and 2,000 ops in the first, a middle and
    # the last pool (their other documents keep 400): waves find nothing left
    # and exit early, and one wave finishes the long document alone, taking it
    # back from itself burst after burst.  Every word of every document of
    # those pools is compared.
    nf = 2 * resident() - 1
    first = pool_first(nf)
    pools = first_middle_last(nf)
    counts = {}
    for p in pools:
        assert first[p + 1] - first[p] >= len(UNEVEN)
        counts.update({int(first[p]) + i: c for i, c in enumerate(UNEVEN)})
    s = with_counts(long_stream(nf), counts)
    got = np.diff(s["batch"]["op_offsets"].astype(np.int64))
    assert all(got[d] == c for d, c in counts.items())
    o = spec(s)
    assert (o.statuses() == 0).all()
    assert_same_state(o, device(s), pool_docs(nf, pools))


# ---- 3. documents that leave the pool mid-pass -------------------------------

def test_gpu_pools_documents_leave_mid_pass():
    # insert-only documents: 120 ops stay below 254 segments (pass 1 to the
    # end; so do the 130 a failing document applies); in each inspected pool one document keeps 420 ops and outgrows 254
    # segments mid-pass (it goes on in pass 2), one stops at an op whose
    # sequence number runs backwards (MTE_E_SEQ_ORDER) and one has no ops
    nf = resident() + 1
    first = pool_first(nf)
    pools = first_middle_last(nf)
    s = gen.generate(2, n_docs=nf, ops_per_doc=420, mix=gen.MIX_INSERT, min_length=0, length_mode=2)
    n = np.full(nf, 120, np.int64)
    grows = [int(first[p]) for p in pools]
    fails = [int(first[p]) + 1 for p in pools]
    empty = [int(first[p]) + 2 for p in pools]
    n[grows] = 420
    n[fails] = 150
    n[empty] = 0
    s = se.first_ops(s, n)
    offs = s["batch"]["op_offsets"].astype(np.int64)
    ops = s["batch"]["ops"].copy()
    for d in fails:
        k = offs[d] + 130  # in the second burst
        ops["seq"][k] = ops["seq"][k - 1]  # not above the op before it
    s = dict(s, batch=dict(s["batch"], ops=ops))
    o = spec(s)
    st = o.statuses()
    assert (st[fails] == MTE_E_SEQ_ORDER).all() and (np.delete(st, fails) == 0).all()
    assert all(o.nsegs(d) > 254 for d in grows)
    assert max(o.nsegs(d) for d in range(nf) if d not in grows) <= 254
    assert_same_state(o, device(s), pool_docs(nf, pools))


# ---- 4. a document that changes tier across hand-offs ----------------------------

def tier_at_bursts(trace_row, n_ops):
    """The register tier pass 1 picks at each burst's start (pick_pass1_tier)."""
    return [1 if trace_row[k] + 2 <= 64 else 2 if trace_row[k] + 2 <= 128 else 4 for k in range(0, n_ops, BURST)]


def test_gpu_pools_document_changes_tier_across_handoffs():
    # in the long stream's first pool, a document whose bursts run at E = 1,
    # then E = 2, then E = 1 again (segment counts from the restatement); it
    # keeps its 2,000 ops, its pool is inspected whole
    nf = 2 * resident() - 1
    first = pool_first(nf)
    full = long_stream(nf)
    probe = gen.slice_docs(full, 0, int(first[1]))
    trace = se.nsegs_trace(probe)
    found = None
    for d in range(len(trace)):
        t = tier_at_bursts(trace[d], 2000)
        i = next((i for i, e in enumerate(t) if e == 2), None)
        if t[0] == 1 and i is not None and 1 in t[i:] and max(t) == 2:
            found = d
            break
    assert found is not None, "no document of the first pool goes E = 1 -> 2 -> 1"
    s = with_counts(full, {found: 2000})
    o = spec(s)
    assert (o.statuses() == 0).all()
    assert_same_state(o, device(s), pool_docs(nf, [0]))


# ---- 8. the instantiations that may stay at five waves ---------------------------

def test_gpu_pools_no_property_planes():
    # K = 0 (a context without property keys): the plain kernel is built for
    # five waves per SIMD, the one with statistics for six
    nf = resident() + 1
    s = gen.generate(2, n_docs=nf, ops_per_doc=OPS, length_mode=2)
    s = dict(s, n_keys=0)
    o = spec(s)
    assert (o.statuses() == 0).all()
    for waves, stats in ((5, False), (6, True)):
        assert np.diff(pool_first(nf, waves)).max() > WPB
        docs = pool_docs(nf, first_middle_last(nf, waves), waves)
        assert_same_state(o, device(s, stats=stats), docs, stats=stats)


def test_gpu_pools_unpacked_four_planes():
    # value ids past a byte on text: the unpacked K = 4 kernel
    nf = resident() + 1
    s = se.big_colors(even_stream(nf))
    assert se.stream_layout(s) == "unpacked"
    o = spec(s)
    assert (o.statuses() == 0).all()
    assert_same_state(o, device(s), pool_docs(nf, first_middle_last(nf)))

