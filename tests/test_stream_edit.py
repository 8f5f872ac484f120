"""The stream edits of tests/stream_edit.py, on the CPU: every edited stream is
still a valid stream for the specification (all statuses 0, the flat
restatement equal to the chunked one in digests, read-outs and segment lists),
forces the pass-1 layout its case names, and really holds what the case is
about (ids >= 256 on a text key, rewrites over markers, sets of 3+ keys)."""
import numpy as np
import pytest

import stream_edit as se
from fluidframework_amd import gen
from oracle import OracleEngine

N_DOCS = 16


def _base():
    return gen.generate(3, n_docs=N_DOCS, ops_per_doc=600, length_mode=2)


def _pair(stream):
    out = []
    for tree in (False, "chunked"):
        o = OracleEngine(stream["n_keys"], threads=8, tree=tree)
        gen.load_stream(o, stream)
        o.apply_batch(stream["batch"])
        out.append(o)
    return out


def _valid(stream):
    f, c = _pair(stream)
    assert (f.statuses() == 0).all()
    np.testing.assert_array_equal(c.statuses(), f.statuses())
    np.testing.assert_array_equal(c.digest(), f.digest())
    for doc in range(0, N_DOCS, 3):
        assert c.read_doc(doc) == f.read_doc(doc)
        for x, y in zip(f.read_segments(doc), c.read_segments(doc)):
            np.testing.assert_array_equal(x, y)
    return f


@pytest.mark.parametrize("name", sorted(se.LAYOUT_CASES))
def test_layout_case_is_valid_and_forces_its_layout(oracle_lib, name):
    edit, layout = se.LAYOUT_CASES[name]
    base = _base()
    before = {k: v.copy() for k, v in base["batch"].items()}
    s = edit(base)
    for k, v in before.items():  # the edit left its argument alone
        np.testing.assert_array_equal(base["batch"][k], v)
    assert se.stream_layout(s) == layout
    assert se.stream_layout(s, pack_env=False) == "unpacked"
    f = _valid(s)
    b = s["batch"]
    if layout == "unpacked":
        assert se.text_ids_at_least(b, 256) > 0
    else:
        assert se.text_ids_at_least(b, 256) == 0
    if name == "id255":
        assert se.text_ids_at_least(b, 255) > 0
    if name == "id256":
        assert (b["props"]["value"] <= 256).all()
    if name.startswith("wide"):
        assert se.wide_sets_applied(b, 3) > 100 and se.wide_sets_applied(b, 4) > 100
        # the null of an added key deletes, as the null of a generated one
        wide = b["propsets"][b["propsets"]["count"] >= 3]
        assert any(b["props"]["value"][int(p["first"]) + 2] == 0 for p in wide)
    if name.startswith("rewrite"):
        assert len(se.docs_with_rewritten_markers(s)) * 2 >= N_DOCS
    elif "wide" not in name or layout == "side3":  # an annotate's null markerId clears a marker's as well
        assert not se.docs_with_rewritten_markers(s)


def test_rewrite_clears_what_the_set_does_not_name(oracle_lib):
    # the same stream with and without the flag differs, and only in properties
    base = _base()
    plain, rw = _valid(base), _valid(se.set_rewrite(base, se.REWRITE_EVERY))
    differ = 0
    for doc in range(N_DOCS):
        (sa, pa, ta), (sb, pb, tb) = plain.read_segments(doc), rw.read_segments(doc)
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(ta, tb)
        differ += bool((pa != pb).any())
    assert differ * 2 > N_DOCS


def test_touch_side_key_flips_the_layout_mid_stream(oracle_lib):
    s = se.touch_side_key_from(_base(), 0.55)
    _valid(s)
    parts = [se.prune_props(gen.cut_ops(s, a, b)) for a, b in ((0, 0.4), (0.4, 0.7), (0.7, 1.0))]
    tables = [se.batch_tables(p) for p in parts]
    assert [se.pass1_layout(tables[:k + 1]) for k in range(3)] == ["side3", "unpacked", "unpacked"]


def test_pruned_batches_replay_as_the_whole_stream(oracle_lib):
    # batches with their own pruned tables end where the uncut stream ends
    s = se.widen_propsets(_base(), 3, se.ALL_KEYS, marker_sets=True)
    whole = OracleEngine(4, threads=8)
    gen.load_stream(whole, s)
    whole.apply_batch(s["batch"])
    cut = OracleEngine(4, threads=8)
    gen.load_stream(cut, s)
    for a, b in ((0, 0.3), (0.3, 0.6), (0.6, 1.0)):
        p = se.prune_props(gen.cut_ops(s, a, b))
        assert len(p["propsets"]) < len(s["batch"]["propsets"])
        cut.apply_batch(p)
    assert (whole.statuses() == 0).all()
    np.testing.assert_array_equal(cut.statuses(), whole.statuses())
    np.testing.assert_array_equal(cut.digest(), whole.digest())


def test_sticky_batches_walk_packed_side_unpacked(oracle_lib):
    parts = se.sticky_batches(_base())
    tables = [se.batch_tables(p) for p in parts]
    assert [se.pass1_layout(tables[:k + 1]) for k in range(3)] == ["packed", "side3", "unpacked"]
    o = OracleEngine(4, threads=8)
    gen.load_stream(o, _base())
    for p in parts:
        o.apply_batch(p)
    assert (o.statuses() == 0).all()


def test_capacity_cut_follows_the_segment_counts(oracle_lib):
    # insert-only documents grow by 1-2 segments an op; a flat pass takes an op
    # only while n + 2 <= cap
    s = gen.generate(2, n_docs=4, ops_per_doc=300, mix=gen.MIX_INSERT, min_length=0, length_mode=2)
    trace = se.nsegs_trace(s)
    whole = OracleEngine(s["n_keys"])
    gen.load_stream(whole, s)
    whole.apply_batch(s["batch"])
    assert [whole.nsegs(d) for d in range(4)] == trace[:, -1].tolist()
    assert set(np.unique(np.diff(trace, axis=1)).tolist()) <= {1, 2}
    cap = 200
    took = se.ops_before_capacity(trace, cap)
    assert (took < 300).all()
    head = se.first_ops(s, took)
    o = OracleEngine(s["n_keys"])
    gen.load_stream(o, head)
    o.apply_batch(head["batch"])
    assert (o.statuses() == 0).all()
    assert all(o.nsegs(d) in (cap - 1, cap) for d in range(4))
    assert all(trace[d, took[d] - 1] + 2 <= cap for d in range(4))
    # a pass that looks after the op stops at the same op or one earlier
    early = se.ops_before_capacity(trace, cap, after=True)
    assert set((took - early).tolist()) <= {0, 1} and (took != early).any()
    assert all(trace[d, early[d]] + 2 <= cap < trace[d, early[d] + 1] + 2 for d in range(4))
    fit = se.first_ops(s, se.ops_peaking_at(trace, cap - 2))
    o = OracleEngine(s["n_keys"])
    gen.load_stream(o, fit)
    o.apply_batch(fit["batch"])
    assert all(o.nsegs(d) in (cap - 3, cap - 2) for d in range(4))
    fit_trace = se.nsegs_trace(fit)
    assert (se.ops_before_capacity(fit_trace, cap) == fit_trace.shape[1] - 1).all()  # no op is refused
