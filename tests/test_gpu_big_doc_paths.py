"""Passes 2 and 3 and the chunked pass op after op, case by case against the
specification (SpecOracle), bit-exact: statuses, digests, read-outs (cur_seq
and min_seq among them), full segment lists, the op statistics and, for the
event documents, the delta events of every batch -- of stopped documents too.

The cases, the model of which kernel runs a record and the CPU preconditions
are tests/big_doc_cases.py.  Six contexts: "pass2" (big_kernel, the default
1,024 segments), "stream0 / 4 / 8" (stream_kernel in 2,048-segment contexts at
n_keys 0, 4 and 8: its plane groups of 5 + 1, 5 + 5 and 5 + 5 + 4) and
"chunk8192 / 16384" (ch_ops).  Each runs its documents in the table's order
and again permuted, so that every case sits on another wave of its block of
four documents and next to other neighbours.  The chunked contexts replay the
permuted order with statistics off, the product path through the round
phases' planner, where every stretch of records here has to go op after op:
`round_bytes` stays 0.

test_big_doc_cases_reach_their_conditions needs no GPU: every case reaches its
stated condition on the restatement alone (the kernel of each checked record,
the leaf, slot, tile or chunk it targets, the status, "not a round").
"""
import functools

import numpy as np
import pytest

import big_doc_cases as bc
from fluidframework_amd.abi import DOC_EVENTS, MTE_E_CAPACITY, MergeTreeError
from fluidframework_amd.engine import DeviceEngine
from test_gpu_block_decode import build_stream
from test_gpu_flat_variants import assert_same_segments
from test_gpu_parity import STAT_KEYS

# cases per group, the padding documents included (big_doc_cases.group_cases)
COUNTS = {"pass2": 812, "stream0": 1652, "stream4": 1652, "stream8": 1652, "chunk8192": 384, "chunk16384": 296}
PARTS = 4  # each context's documents are compared in this many slices, so one test stays short


@pytest.mark.parametrize("group", bc.GROUPS)
def test_big_doc_cases_reach_their_conditions(group):
    cases, cap, n_keys, o, _ = bc.reference(group)
    assert len(cases) == COUNTS[group] and len(cases) % bc.DOCS_PER_BLOCK == 0
    assert len({d.name for d in cases}) == len(cases)
    names = {d.name for d in cases}
    stops = [d for d in cases if d.stop]
    assert all((d.status == MTE_E_CAPACITY) == d.capacity and d.status < 0 for d in stops)
    pre = {"pass2": "p2", "chunk8192": "ch"}.get(group, "st")
    if group != "chunk16384":
        for kind in bc.WINDOW_ERRORS:
            assert {f"{pre}_window_{kind}_first", f"{pre}_window_{kind}_last"} <= names
        assert cases[-1].name.endswith("_last") and cases[-1].stop == (0, len(cases[-1].batches[0]) - 1)
        assert {f"{pre}_message_cut1", f"{pre}_message_cut2", f"{pre}_legacy_message_cut1"} <= names
    order, pos = bc.permutation(len(cases))
    assert all(order[p] == i for i, p in enumerate(pos))


@functools.lru_cache(maxsize=1)
def replayed(group, permuted):
    """-> (the device engine after all batches, the case of each of its
    documents, its read_deltas per batch, its statistics per batch).  One
    context at a time: the tests of one (group, permuted) pair run in a row."""
    cases, cap, n_keys, _, _ = bc.reference(group)
    order = bc.expected(group, permuted)[0]
    s, batches = build_stream([cases[i] for i in order], "packed", n_keys=n_keys)
    d = DeviceEngine(n_keys, seg_capacity=cap)
    if permuted and group.startswith("chunk"):
        d.set_stats(False)
    if group.startswith("stream"):
        # 64 x its records + 256 events per document and batch: the annotates over a whole
        # event document of 257 segments fit (the overflow has its own test below)
        d.set_event_capacity(64)
    d.load_docs(s["inits"], s["init_text"])
    d.load_segments(*s["segs"])
    deltas, stats = [], []
    for b in batches:
        d.apply_batch(b)
        deltas.append({p: d.read_deltas(p) for p, i in enumerate(order) if cases[i].flags & DOC_EVENTS})
        stats.append(d.stats())
    return d, order, deltas, stats


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("group", bc.GROUPS)
def test_gpu_big_doc_paths(group, permuted, part):
    cases = bc.reference(group)[0]
    order, o, want_deltas = bc.expected(group, permuted)
    d, _, deltas, stats = replayed(group, permuted)
    st, dg, dgo = d.statuses(), d.digest(), o.digest()
    failed = []
    lo, hi = part * len(cases) // PARTS, (part + 1) * len(cases) // PARTS
    for p in range(lo, hi):
        c = cases[order[p]]
        try:
            assert st[p] == c.status
            assert np.array_equal(dg[p], dgo[p])
            want = o.read_doc(p)
            assert d.read_doc(p) == (dict(want, status=MTE_E_CAPACITY) if c.capacity else want)
            assert_same_segments(o, d, [p])
            for bi in range(len(deltas)):
                if p in deltas[bi]:
                    np.testing.assert_array_equal(deltas[bi][p], want_deltas[bi][p])
        except AssertionError as e:
            failed.append((c.name, str(e).strip().split("\n")[0][:80]))
    assert not failed, f"{len(failed)} of {hi - lo} cases differ: {failed[:40]}"
    if part:
        return
    if permuted and group.startswith("chunk"):
        # statistics off: the round phases' planner saw every batch and took none as a round
        assert all(s["round_bytes"] == 0 for s in stats)
    else:
        so, sd = o.stats(), stats[-1]
        for k in STAT_KEYS:
            assert sd[k] == so[k], k
        assert all(s["round_bytes"] == 0 for s in stats)


def last_record_spec(pre, kind):
    cases, cap = bc.last_record_cases(pre, kind)
    o = bc.spec(cases, 4, cap)
    assert o.statuses().tolist() == [0, cases[1].status] and cases[1].status < 0
    return cases, cap, o


@pytest.mark.parametrize("pre", list(bc.LAST_RECORD))
def test_last_record_cases_stop_at_the_batch_end(pre):
    for kind in bc.WINDOW_ERRORS:
        last_record_spec(pre, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("pre", list(bc.LAST_RECORD))
def test_gpu_window_error_in_the_last_record_of_the_batch(pre):
    """Each of the five window errors as the last record of the last document
    of a batch, on every kernel: nothing follows it but the zeroed pad."""
    for kind in bc.WINDOW_ERRORS:
        cases, cap, o = last_record_spec(pre, kind)
        s, batches = build_stream(cases, "packed")
        d = DeviceEngine(4, seg_capacity=cap)
        d.load_docs(s["inits"], s["init_text"])
        d.load_segments(*s["segs"])
        for b in batches:
            d.apply_batch(b)
        np.testing.assert_array_equal(d.statuses(), o.statuses(), err_msg=kind)
        np.testing.assert_array_equal(d.digest(), o.digest(), err_msg=kind)
        for i in range(2):
            assert d.read_doc(i) == o.read_doc(i), kind
        assert_same_segments(o, d, [0, 1])
        for k in STAT_KEYS:
            assert d.stats()[k] == o.stats()[k], (kind, k)
        d.close()


@pytest.mark.gpu
def test_gpu_event_region_too_small_for_the_op():
    """include/mte.h: an event document's region holds per_op x its records +
    256 events per batch (mte_set_event_capacity); when a batch produces more,
    mte_read_deltas answers MTE_E_CAPACITY and the document itself is replayed
    as if nothing were recorded.  One annotate over 300 segments, from inside
    the first to inside the last, visits 300; with per_op = 1 the region holds 257."""
    n = 300
    cases = [bc.BigDoc("ev_overflow", n, bc.EVENTS), bc.BigDoc("ev_fits", 200, bc.EVENTS)]
    for c in cases:
        c.annotate(1, bc.SEG * c.n - 1, "T_2")
    o = bc.spec(cases, 4, 2048)
    assert len(o.read_deltas(0)) == n > 256 + 1 >= len(o.read_deltas(1)) == 200
    s, batches = build_stream(cases, "packed")
    d = DeviceEngine(4, seg_capacity=2048)
    d.set_event_capacity(1)
    d.load_docs(s["inits"], s["init_text"])
    d.load_segments(*s["segs"])
    d.apply_batch(batches[0])
    with pytest.raises(MergeTreeError) as e:
        d.read_deltas(0)
    assert e.value.code == MTE_E_CAPACITY
    np.testing.assert_array_equal(d.read_deltas(1), o.read_deltas(1))
    np.testing.assert_array_equal(d.statuses(), [0, 0])
    np.testing.assert_array_equal(d.digest(), o.digest())
    for i in range(2):
        assert d.read_doc(i) == o.read_doc(i)
    assert_same_segments(o, d, [0, 1])
