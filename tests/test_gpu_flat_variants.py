"""The variants of the flat passes that the data select, each against the
specification (SpecOracle), bit-exact: statuses, digests, the op statistics,
read-outs and the full segment lists (every segment's seq, removed_seq,
removers, client, kind, properties and text, tombstones above minSeq included).

  * pass 1's three property layouts for 4-key contexts (launch_replay,
    mte_engine.hip): all planes packed in one register, packed with a side key
    in the markers' toff register, and unpacked -- forced through the value ids
    and property sets of edited streams (tests/stream_edit.py), the 255 / 256
    boundary, sets of 3-4 keys, MTE_F_REWRITE, the sticky switch from one batch
    to the next and loaded bodies included;
  * pass 1's wave grouping (g documents per wave, mte_load_docs): g = 2, 3, 8
    with a padded last group;
  * the segment lists after each flat pass (register tiers, the streamed pass,
    the chunked pass op after op and its round phases);
  * the state at which a document stops with MTE_E_CAPACITY, and documents
    that peak two segments below the capacity.
"""
import functools

import numpy as np
import pytest

import stream_edit as se
from flat_checks import assert_stopped_like_spec, resident_docs
from fluidframework_amd import gen
from fluidframework_amd.abi import NO_PROPS, NOT_REMOVED, PROP_DTYPE, PROPSET_DTYPE, SEG_DTYPE
from fluidframework_amd.engine import DeviceEngine
from oracle import SpecOracle

pytestmark = pytest.mark.gpu

STAT_KEYS = ["ops_applied", "segs_scanned", "segs_written", "prop_writes", "units_inserted", "max_segs"]


def assert_same_segments(o, d, docs):
    """mte_read_segments of the engine against the specification's, exactly:
    the same segmentation, and every field, property and text unit equal.
    Nothing is coalesced or left out here.  (The round phases keep a carried
    document's tombstones at or below minSeq in its planes until its next
    re-layout, as the reference's scour drops them in its own time,
    mergeTree.ts:681-747; mte_read_segments lists the canonical state without
    them, so the lists are equal after the round phases too.)"""
    for doc in docs:
        so, po, to = o.read_segments(doc)
        sd, pd, td = d.read_segments(doc)
        assert len(sd) == len(so), doc
        for f in SEG_DTYPE.names:
            np.testing.assert_array_equal(sd[f], so[f], err_msg=f"doc {doc}: {f}")
        np.testing.assert_array_equal(pd, po, err_msg=f"doc {doc}: props")
        np.testing.assert_array_equal(td, to, err_msg=f"doc {doc}: text")


def assert_same_state(o, d, docs, stats=True):
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
    if stats:
        so, sd = o.stats(), d.stats()
        for k in STAT_KEYS:
            assert sd[k] == so[k], k
    for doc in docs:
        assert d.read_doc(doc) == o.read_doc(doc), doc
    assert_same_segments(o, d, docs)


def spec(stream, cap=0, threads=16):
    o = SpecOracle(stream["n_keys"], threads=threads, cap=cap)
    gen.load_stream(o, stream)
    o.apply_batch(stream["batch"])
    return o


def device(stream, cap=0, stats=True):
    d = DeviceEngine(stream["n_keys"], seg_capacity=cap)
    if not stats:
        d.set_stats(False)
    gen.load_stream(d, stream)
    d.apply_batch(stream["batch"])
    return d


# ---- pass 1's property layouts (one document per wave) -----------------------

N_DOCS = 64


@functools.lru_cache(maxsize=None)
def base_stream():
    # length_mode 2: every document on the flat passes, 600 ops keep them in pass 1 / pass 2
    return gen.generate(3, n_docs=N_DOCS, ops_per_doc=600, length_mode=2)


@functools.lru_cache(maxsize=None)
def layout_case(name):
    edit, layout = se.LAYOUT_CASES[name]
    s = edit(base_stream())
    assert se.stream_layout(s) == layout  # the rule of launch_replay on this stream's tables
    o = spec(s)
    assert (o.statuses() == 0).all()
    return s, o


@pytest.mark.parametrize("name", sorted(se.LAYOUT_CASES))
def test_gpu_pass1_layout(name):
    s, o = layout_case(name)
    if name.startswith("rewrite"):
        assert len(se.docs_with_rewritten_markers(s)) * 2 >= N_DOCS
    if name.startswith("wide"):
        assert se.wide_sets_applied(s["batch"], 4 if "side" not in name else 3) > 1000
    assert_same_state(o, device(s), range(N_DOCS))


@pytest.mark.parametrize("name", ["packed", "side", "wide_packed", "rewrite_side"])
def test_gpu_pass1_unpacked_by_environment(name, monkeypatch):
    # MTE_PACK_PROPS=0 (read in mte_create): the unpacked K = 4 pass 1 on streams
    # whose ids would pack -- the same documents as the default engine's
    s, o = layout_case(name)
    assert se.stream_layout(s, pack_env=False) == "unpacked"
    packed = device(s)
    monkeypatch.setenv("MTE_PACK_PROPS", "0")
    plain = device(s)
    np.testing.assert_array_equal(plain.statuses(), packed.statuses())
    np.testing.assert_array_equal(plain.digest(), packed.digest())
    for doc in range(N_DOCS):
        for x, y in zip(plain.read_segments(doc), packed.read_segments(doc)):
            np.testing.assert_array_equal(x, y)
    assert_same_state(o, plain, range(N_DOCS))


def _sticky(parts, layouts, final_alone):
    base = base_stream()
    tables = [se.batch_tables(p) for p in parts]
    assert [se.pass1_layout(tables[:k + 1]) for k in range(len(parts))] == layouts
    assert se.pass1_layout(tables[-1:]) == final_alone
    o = SpecOracle(base["n_keys"], threads=16)
    d = DeviceEngine(base["n_keys"])
    gen.load_stream(o, base)
    gen.load_stream(d, base)
    for p in parts:
        # document state one layout stored is loaded by the next
        o.apply_batch(p)
        d.apply_batch(p)
        assert (o.statuses() == 0).all()
        assert_same_state(o, d, range(N_DOCS))
    # mte_reset + mte_run replays the last batch from the loaded state in the
    # context's (sticky) layout.  Its ops were made for a later state: most
    # documents refuse their first ops (MTE_E_INSERT_FAILED), the same in a
    # fresh context given that batch and in the specification
    d.reset()
    d.run()
    d.sync()
    fresh = DeviceEngine(base["n_keys"])
    gen.load_stream(fresh, base)
    fresh.apply_batch(parts[-1])
    again = SpecOracle(base["n_keys"], threads=16)
    gen.load_stream(again, base)
    again.apply_batch(parts[-1])
    for other in (fresh, again):
        np.testing.assert_array_equal(d.statuses(), other.statuses())
        np.testing.assert_array_equal(d.digest(), other.digest())
        for doc in range(N_DOCS):
            assert d.read_doc(doc) == other.read_doc(doc)
        assert_same_segments(other, d, range(N_DOCS))
    # and the whole stream again from the loaded state, every op applied, now
    # all of it in the layout the context ended in
    assert se.pass1_layout(tables + tables[:1]) == layouts[-1]
    d.reset()
    o = SpecOracle(base["n_keys"], threads=16)
    gen.load_stream(o, base)
    for p in parts:
        o.apply_batch(p)
        d.apply_batch(p)
        assert (o.statuses() == 0).all()
        assert_same_state(o, d, range(N_DOCS), stats=False)


def test_gpu_pass1_sticky_packed_side_unpacked():
    _sticky(se.sticky_batches(base_stream()), ["packed", "side3", "unpacked"], "unpacked")


def test_gpu_pass1_sticky_side_to_unpacked_by_text_key():
    # from 55% of each document's ops annotates carry markerId too: key_text[3]
    # flips inside the second batch
    s = se.touch_side_key_from(base_stream(), 0.55)
    parts = [se.prune_props(gen.cut_ops(s, a, b)) for a, b in ((0, 0.4), (0.4, 0.7), (0.7, 1.0))]
    _sticky(parts, ["side3", "unpacked", "unpacked"], "unpacked")


def _loaded_body(stream, text_set, marker_value):
    """Every document's load text as [20 units with text_set][a marker with
    markerId marker_value(d)][the rest, no properties] -> (segs, propsets, props)."""
    inits = stream["inits"]
    nd = len(inits)
    sets = [text_set] + [[(se.KEY_MARKER_ID, marker_value(d))] for d in range(nd)]
    ps = np.zeros(len(sets), PROPSET_DTYPE)
    ps["count"] = [len(x) for x in sets]
    ps["first"] = np.concatenate([[0], np.cumsum(ps["count"])[:-1]])
    pe = np.array([e for x in sets for e in x], PROP_DTYPE)
    segs = np.zeros(3 * nd, SEG_DTYPE)
    segs["removed_seq"] = NOT_REMOVED
    segs["client"] = -1
    t0, n = inits["text_off"].astype(np.int64), inits["text_len"].astype(np.int64)
    assert (n > 20).all()
    segs["text_off"][0::3], segs["len"][0::3], segs["propset"][0::3] = t0, 20, 0
    segs["len"][1::3], segs["kind"][1::3], segs["propset"][1::3] = 1, 2, 1 + np.arange(nd)
    segs["text_off"][2::3], segs["len"][2::3], segs["propset"][2::3] = t0 + 20, n - 20, NO_PROPS
    return (np.arange(nd + 1, dtype=np.uint64) * 3, segs), ps, pe


@pytest.mark.parametrize("where,layout", [("marker", "side3"), ("text", "unpacked"), ("init_propset", "unpacked"),
                                         ("small", "packed")])
def test_gpu_pass1_layout_from_loaded_body(where, layout):
    # ids >= 256 that only the loaded body holds (mte_load_docs' table, the keys
    # of loaded text segments): on a marker alone -> side key, on text -> unpacked;
    # the ops that follow (a rewrite every fourth annotate) carry small ids only.
    # The loaded marker lengthens each document by one: the ops stay in range
    s = gen.generate(3, n_docs=N_DOCS, ops_per_doc=600, length_mode=2, init_len=40)
    s = se.set_rewrite(se.small_marker_ids(s), 4)
    color = 300 if where in ("text", "init_propset") else 45
    body, ps, pe = _loaded_body(s, [(se.KEY_BOLD, 35), (se.KEY_COLOR, color)],
                                lambda d: 1000 + d if where == "marker" else 70 + d)
    inits = s["inits"].copy()
    if where == "init_propset":
        inits["propset"] = 0  # the whole load text holds the set; no segment body
    text_sets = [{se.KEY_BOLD, se.KEY_COLOR}]
    if where == "init_propset":
        pe = pe[:2]  # the table holds the text's set alone
        ps = ps[:1]
    assert se.pass1_layout([(pe, text_sets), se.batch_tables(s["batch"])]) == layout
    o, d = SpecOracle(4, threads=16), DeviceEngine(4)
    for e in (o, d):
        e.load_docs(inits, s["init_text"], ps, pe)
        if where != "init_propset":
            e.load_segments(*body)
        e.apply_batch(s["batch"])
    assert (o.statuses() == 0).all()
    assert_same_state(o, d, range(N_DOCS))


# ---- pass 1's wave grouping ---------------------------------------------------

def group_of(n_flat):
    r = resident_docs()
    return min(8, max(1, (n_flat + r - 1) // r))


def spread_docs(n, g):
    """32 documents over the range, the padded last group's among them."""
    last = list(range(n - 1 - (n - 1) % g, n))
    return sorted(set(np.linspace(0, n - 1, 32 - len(last)).astype(int).tolist() + last))


def _grouped(stream, g):
    n = len(stream["inits"])
    assert group_of(n) == g and n % g != 0  # the last group is padded
    o = spec(stream)
    assert (o.statuses() == 0).all()
    assert_same_state(o, device(stream), spread_docs(n, g))


def test_gpu_pass1_group2_side_key():
    s = gen.generate(3, n_docs=resident_docs() + 1, ops_per_doc=200, length_mode=2)
    assert se.stream_layout(s) == "side3"
    _grouped(s, 2)


def test_gpu_pass1_group2_unpacked():
    s = se.big_colors(gen.generate(3, n_docs=resident_docs() + 1, ops_per_doc=200, length_mode=2))
    assert se.stream_layout(s) == "unpacked"
    _grouped(s, 2)


def test_gpu_pass1_group2_round_sync_legacy():
    # legacy documents declared round-synchronous stay on the flat passes
    s = gen.generate(3, n_docs=resident_docs() + 1, ops_per_doc=200, round_sync=True)
    assert ((s["inits"]["flags"] & 1) == 0).sum() > resident_docs() // 4
    _grouped(s, 2)


def test_gpu_pass1_group3_rewrite_and_wide_sets():
    s = gen.generate(3, n_docs=2 * resident_docs() + 3, ops_per_doc=200, length_mode=2)
    s = se.set_rewrite(se.widen_propsets(s, 3, marker_sets=True), se.REWRITE_EVERY)
    assert se.stream_layout(s) == "side3"
    assert len(se.docs_with_rewritten_markers(gen.slice_docs(s, 0, 64))) >= 32
    _grouped(s, 3)


@pytest.fixture(scope="module")
def group8():
    s = gen.generate(3, n_docs=7 * resident_docs() + 1, ops_per_doc=200, length_mode=2)
    o = spec(s)
    assert (o.statuses() == 0).all()
    return s, o


@pytest.mark.parametrize("unpacked", [False, True])
def test_gpu_pass1_group8(group8, unpacked, monkeypatch):
    # one replay of the specification for both layouts: the unpacked pass 1
    # through MTE_PACK_PROPS=0 on the same stream
    s, o = group8
    n = len(s["inits"])
    assert group_of(n) == 8 and n % 8 != 0
    assert se.stream_layout(s, pack_env=not unpacked) == ("unpacked" if unpacked else "side3")
    if unpacked:
        monkeypatch.setenv("MTE_PACK_PROPS", "0")
    assert_same_state(o, device(s), spread_docs(n, 8))


# ---- the segment lists after every flat pass ----------------------------------

INSERT_ONLY = dict(mix=gen.MIX_INSERT, min_length=0, length_mode=2)
LONG_DOCS = dict(n_docs=6, ops_per_doc=4000, init_len=20000, round_ops=1024, min_length=16, length_mode=2)
CONFIG5 = dict(n_docs=8, ops_per_doc=8000, init_segs=20000, round_ops=2000)
# name -> (config, generator arguments, context capacity); contexts of >= 8,192
# segments replay documents past the register tiers on the chunked pass, smaller
# ones on the HBM-streamed pass (kChunkMinCap, mte_chunk.h)
PASS_STREAMS = {
    "tiers_insert": (2, dict(n_docs=24, ops_per_doc=420, **INSERT_ONLY), 0),
    "tiers": (3, dict(n_docs=64, ops_per_doc=1500, length_mode=2), 0),
    "insert_cap8192": (2, dict(n_docs=12, ops_per_doc=2600, **INSERT_ONLY), 8192),
    "insert_cap4096": (2, dict(n_docs=12, ops_per_doc=2600, **INSERT_ONLY), 4096),
    "long_cap16384": (3, LONG_DOCS, 16384),
    "long_cap4096": (3, LONG_DOCS, 4096),
    "config5": (5, CONFIG5, gen.seg_capacity(5, dict(CONFIG5, init_segs=20000))),
}
VARIANTS = {
    "plain": lambda s: s,
    "rewrite": lambda s: se.set_rewrite(s, se.REWRITE_EVERY),
    "wide": lambda s: se.widen_propsets(s, 3, se.ALL_KEYS, marker_sets=True),
}
ANNOTATED = ["tiers", "long_cap16384", "long_cap4096", "config5"]
PASS_CASES = [(n, "plain") for n in PASS_STREAMS] + [(n, v) for n in ANNOTATED for v in ("rewrite", "wide")]


@functools.lru_cache(maxsize=None)
def pass_case(name, variant):
    cfg, kw, cap = PASS_STREAMS[name]
    s = VARIANTS[variant](gen.generate(cfg, **kw))
    o = spec(s, cap)
    assert (o.statuses() == 0).all()
    if variant == "wide":
        assert se.wide_sets_applied(s["batch"], 4) > 100
    return s, o, cap


@pytest.mark.parametrize("name,variant", PASS_CASES)
def test_gpu_segments_after_flat_passes(name, variant):
    # statistics on: contexts of the chunked pass replay op after op
    s, o, cap = pass_case(name, variant)
    peak = o.stats()["max_segs"]
    assert peak > {"tiers_insert": 512, "tiers": 16}.get(name, 1022)
    assert peak + 2 <= (cap or 1024)
    assert_same_state(o, device(s, cap), range(len(s["inits"])))


@pytest.mark.parametrize("phases", [True, False])
@pytest.mark.parametrize("variant", ["plain", "rewrite", "wide"])
def test_gpu_segments_after_round_phases(variant, phases, monkeypatch):
    # statistics off: the rounds of config 5 replay chunk-parallel (mte_round.h),
    # or, with MTE_ROUND_PHASES=0 (read in mte_create), op after op on the
    # chunked pass compiled without the statistics
    s, o, cap = pass_case("config5", variant)
    if not phases:
        monkeypatch.setenv("MTE_ROUND_PHASES", "0")
    d = device(s, cap, stats=False)
    # mte_stats.round_bytes counts what the round phases moved: none without them
    assert (d.stats()["round_bytes"] > 0) == phases
    assert_same_state(o, d, range(len(s["inits"])), stats=False)


# ---- capacity -----------------------------------------------------------------

@pytest.mark.parametrize("cap,ops,n_docs", [(1024, 1100, 8), (1536, 1700, 8), (8192, 9000, 3)])
def test_gpu_document_peaking_two_below_capacity_succeeds(cap, ops, n_docs):
    # the longest prefix of each insert-only document that never holds more than
    # cap - 2 segments (counted in the restatement): every op finds room for its
    # two segments, so all succeed -- in the last register tier (1,024), on the
    # streamed pass (1,536) and on the chunked pass (8,192)
    s = gen.generate(2, n_docs=n_docs, ops_per_doc=ops, **INSERT_ONLY)
    trace = se.nsegs_trace(s)
    s = se.first_ops(s, se.ops_peaking_at(trace, cap - 2))
    o = spec(s, cap)
    assert (o.statuses() == 0).all()
    assert sum(o.nsegs(doc) == cap - 2 for doc in range(n_docs)) >= 2
    assert max(o.nsegs(doc) for doc in range(n_docs)) == cap - 2
    assert_same_state(o, device(s, cap if cap != 1024 else 0), range(n_docs))


@pytest.mark.parametrize("cap,ops,n_docs", [(1024, 1100, 8), (1536, 1700, 8), (8192, 9000, 3)])
def test_gpu_document_stops_at_capacity_like_spec(cap, ops, n_docs):
    # the same streams in full: every document stops with MTE_E_CAPACITY between
    # two ops, holding the state of the ops before
    # (1,024: the last register tier; 1,536: the streamed pass; 8,192: the chunked pass)
    s = gen.generate(2, n_docs=n_docs, ops_per_doc=ops, **INSERT_ONLY)
    assert_stopped_like_spec(s, device(s, cap if cap != 1024 else 0), cap, streamed=cap == 1536)
