"""The life of one engine context (mte_engine.hip's host side): what survives a
reload, what a refused load leaves, which of the two batch slots a run replays and reads events from, and
the slot buffers and the text arena growing under a context in use.  Every
case compares the context under test with a fresh context or with the
specification (SpecOracle) on the same input, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from fluidframework_amd import gen
from fluidframework_amd.abi import (DOC_EVENTS, DOC_INIT_DTYPE, DOC_NEW_LENGTH_CALC, DOC_TREE, F_MARKER, MTE_E_HIP,
                                    MTE_E_INVALID_ARG, NO_PROPS, OP_ANNOTATE, OP_DTYPE, OP_INSERT, PROP_DTYPE,
                                    PROPSET_DTYPE, MergeTreeError)
from fluidframework_amd.engine import DeviceEngine
from oracle import SpecOracle

pytestmark = pytest.mark.gpu

STAT_KEYS = ["ops_applied", "segs_scanned", "segs_written", "prop_writes", "units_inserted", "max_segs",
             "algo_bytes"]


def tree_event_stream():
    """48 legacy length-calc documents: the first 16 record delta events (the HBM
    tree pass's own), the rest are plain legacy ones (the register tiers of the
    tree pass)."""
    s = gen.generate(3, n_docs=48, ops_per_doc=300, length_mode=1, max_lag=16)
    s["inits"] = s["inits"].copy()
    s["inits"]["flags"][:16] |= DOC_EVENTS
    return s, list(range(16))


def plain_stream():
    """40 plain config-3 documents (new length calculation, no events)."""
    return gen.generate(3, n_docs=40, ops_per_doc=300), []


def replay(e, s):
    gen.load_stream(e, s)
    e.apply_batch(s["batch"])
    return e


def outcome(e, event_docs):
    st = e.stats()
    return (e.statuses().copy(), e.digest().copy(), {k: st[k] for k in STAT_KEYS},
            [e.read_deltas(d).copy() for d in event_docs])


def assert_outcome_equal(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2] == want[2]
    assert len(got[3]) == len(want[3])
    for a, b in zip(got[3], want[3]):
        np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def fresh_outcomes():
    """Each of the two streams on a context of its own."""
    out = {}
    for name, make in (("tree", tree_event_stream), ("plain", plain_stream)):
        s, ev = make()
        out[name] = (s, ev, outcome(replay(DeviceEngine(s["n_keys"]), s), ev))
    return out


@pytest.mark.parametrize("order", [("tree", "plain"), ("plain", "tree")])
def test_reload_leaves_nothing_of_the_earlier_load(fresh_outcomes, order):
    """A second mte_load_docs with another document count and other passes: the
    context computes what a fresh one does.  No event is reachable in the
    reloaded plain context: mte_read_deltas refuses every document (none has
    MTE_DOC_EVENTS; the engine has no empty answer for such a document), and a
    reload of the event stream reads as empty until its first run."""
    first, ev1, _ = fresh_outcomes[order[0]]
    second, ev2, want = fresh_outcomes[order[1]]
    e = DeviceEngine(first["n_keys"])
    replay(e, first)
    for d in ev1:
        assert len(e.read_deltas(d)) > 0
    replay(e, second)
    assert_outcome_equal(outcome(e, ev2), want)
    if not ev2:
        for d in range(e.n_docs):
            with pytest.raises(MergeTreeError) as err:
                e.read_deltas(d)
            assert err.value.code == MTE_E_INVALID_ARG
        gen.load_stream(e, first)  # back to the event stream: nothing ran yet
    else:
        gen.load_stream(e, second)
    for d in (ev1 if not ev2 else ev2):
        assert len(e.read_deltas(d)) == 0
    with pytest.raises(MergeTreeError):  # no batch of an earlier load is left to run
        e.run()


def device_memory_bytes():
    """Total memory of device 0, from the HIP runtime the engine loaded."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value


def test_refused_allocation_leaves_no_documents(fresh_outcomes):
    """A load whose segment planes alone are at least twice the device's memory:
    the driver refuses the request outright, mte_load_docs frees what it had
    built and the context holds no documents -- no statuses, no batch taken --
    until the next load, which computes what a fresh context does."""
    s, ev, want = fresh_outcomes["plain"]
    cap = 4096
    e = DeviceEngine(s["n_keys"], seg_capacity=cap)
    # six field planes and 4 or 8 property planes (one without keys), four bytes per segment slot
    planes = 6 + (1 if s["n_keys"] == 0 else 4 if s["n_keys"] <= 4 else 8)
    n = 2 * device_memory_bytes() // (cap * 4 * planes) + 1
    inits = np.zeros(n, DOC_INIT_DTYPE)
    inits["flags"] = DOC_NEW_LENGTH_CALC
    inits["propset"] = NO_PROPS
    with pytest.raises(MergeTreeError) as err:
        e.load_docs(inits)
    assert err.value.code == MTE_E_HIP
    assert e.n_docs == n
    with pytest.raises(MergeTreeError) as err:
        e.statuses()
    assert err.value.code == MTE_E_INVALID_ARG
    with pytest.raises(MergeTreeError) as err:
        e.submit({"op_offsets": np.zeros(n + 1, np.uint64), "ops": np.zeros(0, OP_DTYPE)})
    assert err.value.code == MTE_E_INVALID_ARG
    assert_outcome_equal(outcome(replay(e, s), ev), want)


def test_load_refused_for_its_arguments_leaves_the_earlier_load(fresh_outcomes):
    """A load propset no document references that runs past `props` is refused
    before anything of the earlier load is touched: the statuses (a plain copy
    of the headers, so asserted first) and then the digest are what they were."""
    s, _, _ = fresh_outcomes["plain"]
    e = replay(DeviceEngine(s["n_keys"]), s)
    statuses, digest = e.statuses().copy(), e.digest().copy()
    assert (s["inits"]["propset"] == NO_PROPS).all()
    with pytest.raises(MergeTreeError) as err:
        e.load_docs(s["inits"], s["init_text"], propsets=np.array([(1, 4)], PROPSET_DTYPE),
                    props=np.zeros(2, PROP_DTYPE))
    assert err.value.code == MTE_E_INVALID_ARG
    np.testing.assert_array_equal(e.statuses(), statuses)
    np.testing.assert_array_equal(e.digest(), digest)


def test_pipelined_submits_read_the_events_of_the_slot_that_ran():
    """submit(k + 1) before the read-out of run k: the events read are run k's
    (the other batch slot), equal to a context that never overlaps."""
    s = gen.generate(3, n_docs=32, ops_per_doc=400, length_mode=2, max_lag=16)
    s["inits"] = s["inits"].copy()
    s["inits"]["flags"] |= DOC_EVENTS
    s["inits"]["flags"][16:] |= DOC_TREE  # half on the HBM-streamed flat pass, half on the HBM tree pass
    parts = [gen.split_ops(s, k, 4) for k in range(4)]
    n = len(s["inits"])
    ref = DeviceEngine(s["n_keys"])
    gen.load_stream(ref, s)
    want = []
    for b in parts:
        ref.submit(b)
        ref.run()
        ref.sync()
        want.append([ref.read_deltas(d).copy() for d in range(n)])
    assert sum(len(x) for x in want[0]) > 0 and sum(len(x) for x in want[3]) > 0
    pip = DeviceEngine(s["n_keys"])
    gen.load_stream(pip, s)
    pip.submit(parts[0])
    for k in range(4):
        pip.run()
        if k + 1 < 4:
            pip.submit(parts[k + 1])
        for d in range(n):
            np.testing.assert_array_equal(pip.read_deltas(d), want[k][d])
    pip.sync()
    np.testing.assert_array_equal(pip.statuses(), ref.statuses())
    np.testing.assert_array_equal(pip.digest(), ref.digest())


def test_second_submit_without_a_run_replaces_the_first():
    """submit, submit, run: the run replays the second batch only (its text at
    the arena offset behind the first batch's)."""
    s = gen.generate(3, n_docs=48, ops_per_doc=400)
    first, second = gen.split_ops(s, 0, 2), gen.split_ops(s, 0, 4)
    d = DeviceEngine(s["n_keys"])
    gen.load_stream(d, s)
    d.submit(first)
    d.submit(second)
    d.run()
    d.sync()
    o = SpecOracle(s["n_keys"], threads=8)
    gen.load_stream(o, s)
    o.apply_batch(second)
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
    assert d.stats()["ops_applied"] == o.stats()["ops_applied"] == len(second["ops"])
    for doc in (0, 23, 47):
        assert d.read_doc(doc) == o.read_doc(doc)


def compact(batch):
    """The batch with only the text, property sets and properties its own
    records use (gen.cut_ops keeps the whole stream's tables)."""
    ops = batch["ops"].copy()
    text_ins = np.flatnonzero((ops["type"] == OP_INSERT) & ((ops["flags"] & F_MARKER) == 0) & (ops["pos2"] > 0))
    chunks, at = [], 0
    for i in text_ins:
        a, n = int(ops["a"][i]), int(ops["pos2"][i])
        chunks.append(batch["text"][a:a + n])
        ops["a"][i] = at
        at += n
    text = np.concatenate(chunks) if chunks else np.zeros(0, np.uint16)
    ins = np.flatnonzero((ops["type"] == OP_INSERT) & (ops["b"] != NO_PROPS))
    ann = np.flatnonzero(ops["type"] == OP_ANNOTATE)
    used = np.unique(np.concatenate([ops["b"][ins], ops["a"][ann]])).astype(np.int64)
    ps = np.zeros(len(used), batch["propsets"].dtype)
    pe, at = [], 0
    for j, u in enumerate(used):
        f, c = int(batch["propsets"]["first"][u]), int(batch["propsets"]["count"][u])
        pe.append(batch["props"][f:f + c])
        ps[j] = (at, c)
        at += c
    ops["b"][ins] = np.searchsorted(used, ops["b"][ins])
    ops["a"][ann] = np.searchsorted(used, ops["a"][ann])
    props = np.concatenate(pe) if pe else np.zeros(0, batch["props"].dtype)
    return dict(batch, ops=ops, text=text, propsets=ps, props=props)


def test_slot_buffers_and_arena_grow_under_a_context_in_use():
    """Small batches fill both slots, then one of 400 ops per document with
    many times their text, property sets and properties goes into the first:
    every buffer of that slot is reallocated, and the arena with the copy of
    what it holds.  A last small batch goes into the slot that did not grow.
    (One small batch more than the bare sequence small / big / small, so the
    big batch meets allocated buffers instead of a slot's first allocation.)"""
    s = gen.generate(3, n_docs=64, ops_per_doc=430)
    cuts = [0.0, 0.023, 0.046, 0.977, 1.0]
    parts = [compact(gen.cut_ops(s, cuts[k], cuts[k + 1])) for k in range(4)]
    sizes = [(len(p["ops"]), len(p["text"]), len(p["propsets"]), len(p["props"])) for p in parts]
    for small in (sizes[0], sizes[1], sizes[3]):
        assert all(4 * x < y for x, y in zip(small, sizes[2])), sizes
    assert sizes[2][0] >= 64 * 390
    d = DeviceEngine(s["n_keys"])
    o = SpecOracle(s["n_keys"], threads=8)
    for e in (d, o):
        gen.load_stream(e, s)
        for p in parts:
            e.apply_batch(p)
    assert (o.statuses() == 0).all()
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
    whole = SpecOracle(s["n_keys"], threads=8)
    gen.load_stream(whole, s)
    whole.apply_batch(s["batch"])
    np.testing.assert_array_equal(o.digest(), whole.digest())
