"""Batched text read-out: mte_read_texts / DeviceEngine.read_texts answer getText
(MergeTreeTextHelper.ts:20-74) and mte_props_at / DeviceEngine.props_at answer
Client.getPropertiesAtPosition (client.ts:1133-1141) for many documents in one
device call.

tests/text_model.py states both flat over a read_doc view.  On the CPU the
model over the restatement must equal the texts the reference itself recorded
(tests/golden/tile_vectors.json.gz: getTextWithPlaceholders at four checkpoints
of generated documents), full and over a grid of ranges.  On the GPU the kernels
must equal the reference's recorded texts -- the 30 replay fixtures' resultText
after every round, the vectors' texts at every checkpoint -- and the model on
synthetic documents built around the 64-slot steps and the 64-unit copy rounds,
on a local client's pending ops, in a big-capacity context and over 1,000
documents.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import text_model
import tile_streams as ts
from fixtures_util import as_msg, doc_inits, load_fixtures
from fluidframework_amd import _native, abi
from fluidframework_amd.abi import (DOC_INIT_DTYPE, DOC_LOCAL_CLIENT, DOC_NEW_LENGTH_CALC, DOC_TREE, MTE_E_INSERT_FAILED,
                                    MTE_E_INVALID_ARG, NO_PROPS, NOT_REMOVED, PROP_DTYPE, PROPSET_DTYPE, SEG_DTYPE,
                                    MergeTreeError)
from fluidframework_amd.packing import TILE_LABELS_KEY, BatchBuilder, DocClients, Interner, units_to_str
from test_find_tile import device_factory, gold_set, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [("newcalc_rounds", 0), ("newcalc_lag16", DOC_TREE), ("legacy_lag16", 0)]


def abi_names():
    """The mirrors of the two calls (absent before they existed: every test here fails then)."""
    return (abi.TEXT_QUERY_DTYPE, abi.TEXT_INFO_DTYPE, abi.POS_QUERY_DTYPE, abi.POS_HIT_DTYPE, abi.TEXT_PLACEHOLDERS,
            abi.TEXT_TO_END)


def grid(length, stride):
    """(start, end) pairs over a stride grid that holds 0, length and length + 5."""
    pts = sorted(set(range(0, length + 1, stride)) | {0, length, length + 5})
    return [(s, e) for s in pts for e in pts if s <= e]


# ---- CPU: the ABI, the model against the reference's texts -----------------------

def test_read_texts_and_props_at_are_declared_exported_and_mirrored(tmp_path):
    TQ, TI, PQ, PH, PLACEHOLDERS, TO_END = abi_names()
    assert {"mte_read_texts", "mte_props_at"} <= set(abi.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libmte.so")], capture_output=True,
                         text=True, check=True).stdout
    assert {"mte_read_texts", "mte_props_at"} <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mte.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(mte_text_query), sizeof(mte_text_info), sizeof(mte_pos_query),\n'
                   '         sizeof(mte_pos_hit));\n'
                   '  printf("%zu %zu %zu %zu\\n", offsetof(mte_text_query, doc), offsetof(mte_text_query, start),\n'
                   '         offsetof(mte_text_query, end), offsetof(mte_text_query, flags));\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", offsetof(mte_text_info, status),\n'
                   '         offsetof(mte_text_info, cur_seq), offsetof(mte_text_info, min_seq),\n'
                   '         offsetof(mte_text_info, length), offsetof(mte_text_info, n_units),\n'
                   '         offsetof(mte_text_info, reserved), offsetof(mte_text_info, offset));\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(mte_pos_query, doc), offsetof(mte_pos_query, pos),\n'
                   '         offsetof(mte_pos_hit, status), offsetof(mte_pos_hit, found), offsetof(mte_pos_hit, kind),\n'
                   '         offsetof(mte_pos_hit, reserved));\n'
                   '  printf("%u %d\\n", MTE_TEXT_PLACEHOLDERS, MTE_TEXT_TO_END);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [[int(x) for x in ln.split()]
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]

    def offsets(dt, names):
        return [dt.fields[n][1] for n in names]

    tq, ti = ["doc", "start", "end", "flags"], ["status", "cur_seq", "min_seq", "length", "n_units", "reserved", "offset"]
    pq, ph = ["doc", "pos"], ["status", "found", "kind", "reserved"]
    assert got == [[TQ.itemsize, TI.itemsize, PQ.itemsize, PH.itemsize], offsets(TQ, tq), offsets(TI, ti),
                   offsets(PQ, pq) + offsets(PH, ph), [PLACEHOLDERS, TO_END]]
    assert got[0] == [16, 32, 8, 16]
    for st, dt, names in ((abi.MteTextQuery, TQ, tq), (abi.MteTextInfo, TI, ti), (abi.MtePosQuery, PQ, pq),
                          (abi.MtePosHit, PH, ph)):
        assert C.sizeof(st) == dt.itemsize and [getattr(st, n).offset for n in names] == offsets(dt, names)
        assert [n for n, _ in st._fields_] == list(dt.names)


def test_both_calls_reject_a_null_context_without_a_device():
    TQ, TI, PQ, PH, _, _ = abi_names()
    lib = _native.load_mte()
    q, info, n = np.zeros(1, TQ), np.zeros(1, TI), C.c_uint64(7)
    assert lib.mte_read_texts(None, q.ctypes.data, 1, info.ctypes.data, None, 0, C.byref(n)) == MTE_E_INVALID_ARG
    assert lib.mte_read_texts(None, None, 0, None, None, 0, C.byref(n)) == MTE_E_INVALID_ARG
    pq, hit = np.zeros(1, PQ), np.zeros(1, PH)
    assert lib.mte_props_at(None, pq.ctypes.data, 1, hit.ctypes.data, None) == MTE_E_INVALID_ARG
    assert lib.mte_props_at(None, None, 0, None, None) == MTE_E_INVALID_ARG


@pytest.mark.parametrize("name", [s for s, _ in SETS])
def test_model_over_restatement_equals_reference_texts(name):
    """The model's range rule against text the reference itself produced."""
    from oracle import SpecOracle
    abi_names()
    S = gold_set(name)
    asked = 0
    for k, e, _ in replay(lambda nk: SpecOracle(nk), S):
        for d, doc in enumerate(S["docs"]):
            if doc["error"]:
                continue
            cp = doc["cps"][k]
            view = e.read_doc(d)
            assert view["length"] == cp["length"] == len(cp["text"])
            assert text_model.get_text(view, placeholders=True) == cp["text"]
            assert text_model.get_text(view) == view["text"]
            for s, t in grid(cp["length"], 13):
                assert text_model.get_text(view, s, t, placeholders=True) == cp["text"][s:t], (name, d, k, s, t)
                asked += 1
    assert asked > 5000


# ---- GPU: the reference's recorded texts ---------------------------------------

@pytest.mark.gpu
def test_gpu_replay_fixtures_one_call_per_round_equals_result_texts():
    """All 30 fixtures as one context; after each round one read_texts call for
    all documents equals every fixture's resultText (a fixture with fewer
    rounds keeps its last)."""
    fx = load_fixtures()
    assert len(fx) == 30
    it = Interner(8)
    e = device_factory(8)
    inits, text = doc_inits([f["rounds"][0]["initialText"] for f in fx])
    e.load_docs(inits, text)
    assert e.read_texts(list(range(len(fx)))) == [f["rounds"][0]["initialText"] for f in fx]
    clients = [DocClients("A") for _ in fx]
    compared = 0
    for r in range(max(len(f["rounds"]) for f in fx)):
        bb = BatchBuilder(len(fx), it)
        for d, f in enumerate(fx):
            for m in (f["rounds"][r]["msgs"] if r < len(f["rounds"]) else []):
                bb.add_message(d, clients[d], as_msg(m))
        e.apply_batch(bb.build())
        assert (e.statuses() == 0).all()
        want = [f["rounds"][min(r, len(f["rounds"]) - 1)]["resultText"] for f in fx]
        assert e.read_texts(list(range(len(fx)))) == want, r
        compared += len(fx)
    assert compared >= 30 * 8
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", SETS)
def test_gpu_vector_documents_equal_reference_texts(name, flags):
    S = gold_set(name)
    rng = random.Random(2)
    asked = 0
    for k, e, _ in replay(device_factory, S, flags):
        qs, want = [], []
        for d, doc in enumerate(S["docs"]):
            if doc["error"]:
                continue
            cp = doc["cps"][k]
            view = e.read_doc(d)
            qs.append((d, 0, None, True))
            want.append(cp["text"])
            qs.append(d)  # plain, the whole document
            want.append(text_model.get_text(view))
            for _ in range(8):
                s = rng.randint(0, cp["length"] + 2)
                t = rng.choice([s, rng.randint(s, cp["length"] + 5), cp["length"], None])
                t = s if t is not None and t < s else t
                qs.append((d, s, t, True))
                want.append(cp["text"][s:t])
                qs.append((d, s, t))
                want.append(text_model.get_text(view, s, t))
        order = list(range(len(qs)))
        rng.shuffle(order)
        got = e.read_texts([qs[i] for i in order])  # one call: all documents, full texts and ranges
        bad = [(name, k, qs[i], g, want[i]) for i, g in zip(order, got) if g != want[i]]
        assert not bad, bad[:3]
        asked += len(qs)
    assert asked > 2000


# ---- GPU: kernel edges on synthetic documents ----------------------------------

def T(n=2, removed=False, props=False):
    return ("t", n, props, removed)


def M(ref_type=1, removed=False):
    return ("m", ref_type, True, removed)


def synthetic_docs():
    """Documents around the 64-slot steps and the 64-unit copy rounds."""
    rng = random.Random(7)
    docs = []
    for nseg in (0, 1, 63, 64, 65, 129):
        doc = []
        for i in range(nseg):
            if i in (0, 63, 64, nseg - 1) and nseg > 1:
                doc.append(M(rng.choice([0, 1, 2])))
            else:
                doc.append(T(1 + i % 3, removed=rng.random() < 0.15, props=i % 5 == 0))
        docs.append(doc)
    docs.append([T(1)])
    docs.append([T(200)])                                            # more than three rounds of the unit loop
    docs.append([T(1 + i % 3) for i in range(63)] + [T(130), T(130)])  # long segments across a step edge
    # tombstones and markers between contributing slots, a run of non-contributing
    # slots, a step (slots 64 .. 127) that gives nothing in plain mode, and one
    # (128 .. 191) that gives nothing in either
    docs.append([T(2), T(1, removed=True), M(), M(1, removed=True), T(3, removed=True), T(3), M(), T(1)] +
                [T(1 + i % 3) for i in range(56)] +
                [M(i % 3) if i % 2 else T(2, removed=True) for i in range(64)] +
                [T(1 + i % 2, removed=True) if i % 3 else M(1, removed=True) for i in range(64)] +
                [T(3), M(), T(2, props=True)])
    docs.append([T(2)])                                              # the last document is stopped below
    return docs


def load_docs_with_text(docs, **kw):
    """load_segments of the documents, every text unit distinct."""
    it = Interner(2)
    sets, entries, segs, offs, units = [], [], [], [0], 0
    for doc in docs:
        for sg in doc:
            rs, rm = (5, 0b10) if sg[3] else (NOT_REMOVED, 0)
            propset = NO_PROPS
            if sg[2]:
                props = {"markerId": f"s{len(segs)}"}
                if sg[0] == "m" and len(segs) % 2:
                    props[TILE_LABELS_KEY] = ["pg"]
                first = len(entries)
                entries.extend(it.kv(k, v) for k, v in props.items())
                sets.append((first, len(entries) - first))
                propset = len(sets) - 1
            if sg[0] == "t":
                segs.append((units, sg[1], 0, rs, rm, -1, 0, propset))
                units += sg[1]
            else:
                segs.append((0, 1, 0, rs, rm, -1, 1 + sg[1], propset))
        offs.append(len(segs))
    inits = np.zeros(len(docs), DOC_INIT_DTYPE)
    inits["flags"], inits["propset"], inits["cur_seq"] = DOC_NEW_LENGTH_CALC, NO_PROPS, 10
    e = device_factory(2, **kw)
    e.load_docs(inits, (0x100 + np.arange(units)).astype(np.uint16), np.array(sets, PROPSET_DTYPE),
                np.array(entries, PROP_DTYPE))
    e.load_segments(np.array(offs, np.uint64), np.array(segs, SEG_DTYPE))
    return e, it


def edge_points(doc, length):
    """Positions worth asking about: the ends, a few segments' first, inner and
    last unit, and the positions where a 64-slot step begins, +- 1."""
    pts, p = {0, 1, length - 1, length, length + 5}, 0
    vis = [i for i, sg in enumerate(doc) if not sg[3]]
    chosen = set(vis[:1] + vis[len(vis) // 2:len(vis) // 2 + 1] + vis[-1:]) | ({62, 63, 64, 65} & set(vis))
    for i, sg in enumerate(doc):
        ln = 0 if sg[3] else (sg[1] if sg[0] == "t" else 1)
        if i and i % 64 == 0:
            pts |= {p - 1, p, p + 1}
        if i in chosen:
            pts |= {p, p + ln // 2, p + ln - 1}
        p += ln
    return sorted(x for x in pts if x >= 0)


@pytest.fixture(scope="module")
def synthetic():
    abi_names()
    docs = synthetic_docs()
    e, it = load_docs_with_text(docs)
    stopped = len(docs) - 1
    bb = BatchBuilder(len(docs), it)  # an insert past the end stops the last document
    bb.add_message(stopped, DocClients("A"), {"clientId": "B", "sequenceNumber": 11, "referenceSequenceNumber": 10,
                                              "minimumSequenceNumber": 0, "type": "op",
                                              "contents": {"type": 0, "pos1": 1000, "seg": "y"}})
    e.apply_batch(bb.build())
    st = e.statuses()
    assert st[stopped] == MTE_E_INSERT_FAILED and (st[:stopped] == 0).all()
    views = [e.read_doc(d) for d in range(stopped)]  # the reference for every test below; never changed
    yield e, it, docs, stopped, views
    e.close()


@pytest.mark.gpu
def test_gpu_kernel_edges_equal_model(synthetic):
    e, it, docs, stopped, views = synthetic
    assert [len(d) for d in docs[:6]] == [0, 1, 63, 64, 65, 129] and views[7]["length"] == 200
    assert views[9]["length"] > 64 and len(docs[9]) == 195
    TO_END = abi.TEXT_TO_END
    qs = []
    for d in range(stopped):
        pts = edge_points(docs[d], views[d]["length"])
        for ph in (0, abi.TEXT_PLACEHOLDERS):
            qs += [(d, s, t, ph) for s in pts for t in pts + [TO_END] if s <= t]
    random.Random(1).shuffle(qs)  # one call, every document many times, in no order
    info, text = e.read_texts_raw(np.array(qs, abi.TEXT_QUERY_DTYPE))
    assert (info["status"] == 0).all() and (info["reserved"] == 0).all()
    sums = np.concatenate([[0], np.cumsum(info["n_units"].astype(np.uint64))])
    assert (info["offset"] == sums[:-1]).all() and sums[-1] == len(text)
    filled, empty, bad = 0, 0, []
    for (d, s, t, ph), h in zip(qs, info):
        want = text_model.get_text(views[d], s, None if t == TO_END else t, placeholders=bool(ph))
        got = units_to_str(text[int(h["offset"]):int(h["offset"]) + int(h["n_units"])])
        if got != want or h["length"] != views[d]["length"] or h["cur_seq"] != views[d]["cur_seq"]:
            bad.append(((d, s, t, ph), got, want, int(h["length"])))
        filled += want != ""
        empty += want == ""
    assert not bad, bad[:3]
    assert filled > 1000 and empty > 200
    # the same through the decoding call, on a sample
    sample = qs[:300]
    assert e.read_texts([(d, s, None if t == TO_END else t, bool(ph)) for d, s, t, ph in sample]) == \
        [text_model.get_text(views[d], s, None if t == TO_END else t, placeholders=bool(ph)) for d, s, t, ph in sample]


@pytest.mark.gpu
def test_gpu_raw_call_sizes_only_short_buffer_no_queries_and_stopped_document(synthetic):
    e, it, docs, stopped, views = synthetic
    TQ, TI = abi.TEXT_QUERY_DTYPE, abi.TEXT_INFO_DTYPE
    q = np.array([(7, 0, abi.TEXT_TO_END, 0), (stopped, 0, abi.TEXT_TO_END, 1), (8, 3, 90, 0), (9, 0, abi.TEXT_TO_END, 1)], TQ)
    info, text = e.read_texts_raw(q)
    sized, none = e.read_texts_raw(q, fill=False)  # sizes only: the same info, no units
    assert (sized == info).all() and len(none) == 0
    assert list(info["status"]) == [0, MTE_E_INSERT_FAILED, 0, 0]
    assert list(info["n_units"][:3]) == [200, 0, 87] and info["length"][1] == 0 and len(text) == info["n_units"].sum()
    # a buffer one unit short is left as it was; MTE_OK and the full size
    n = C.c_uint64()
    buf = np.full(len(text) + 8, 0xABCD, np.uint16)
    info2 = np.zeros(len(q), TI)
    rc = e.lib.mte_read_texts(e.ctx, q.ctypes.data, len(q), info2.ctypes.data, buf.ctypes.data, len(text) - 1, C.byref(n))
    assert rc == 0 and n.value == len(text) and (buf == 0xABCD).all() and (info2 == info).all()
    rc = e.lib.mte_read_texts(e.ctx, q.ctypes.data, len(q), info2.ctypes.data, buf.ctypes.data, len(text), C.byref(n))
    assert rc == 0 and n.value == len(text) and (buf[:len(text)] == text).all() and (buf[len(text):] == 0xABCD).all()
    # n == 0
    n.value = 5
    assert e.lib.mte_read_texts(e.ctx, None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    info0, text0 = e.read_texts_raw(np.zeros(0, TQ))
    assert len(info0) == 0 and len(text0) == 0 and e.read_texts([]) == []
    with pytest.raises(MergeTreeError) as ei:
        e.read_texts([1, stopped])
    assert ei.value.code == MTE_E_INSERT_FAILED
    with pytest.raises(MergeTreeError) as ei:
        e.props_at([(1, 0), (stopped, 0)], it)
    assert ei.value.code == MTE_E_INSERT_FAILED


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [("doc", 10 ** 6), ("start", -1), ("end", 2), ("flags", 2)])
def test_gpu_invalid_text_queries_are_refused_before_any_launch(synthetic, bad):
    e, it, docs, stopped, views = synthetic
    q = np.zeros(2, abi.TEXT_QUERY_DTYPE)
    q[:] = (7, 3, 9, abi.TEXT_PLACEHOLDERS)
    want = text_model.get_text(views[7], 3, 9)
    assert [units_to_str(u) for u in np.split(e.read_texts_raw(q)[1], 2)] == [want, want]  # fine as it stands
    q[bad[0]][1] = bad[1]  # end 2 is below start 3
    with pytest.raises(MergeTreeError) as ei:
        e.read_texts_raw(q)
    assert ei.value.code == MTE_E_INVALID_ARG
    q[bad[0]][1] = 7 if bad[0] == "doc" else 3 if bad[0] == "start" else 9 if bad[0] == "end" else 0
    assert units_to_str(e.read_texts_raw(q)[1][-6:]) == want  # and a valid call still works


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [("doc", 10 ** 6), ("pos", -1)])
def test_gpu_invalid_position_queries_are_refused_before_any_launch(synthetic, bad):
    e, it, docs, stopped, views = synthetic
    q = np.zeros(2, abi.POS_QUERY_DTYPE)
    q[:] = (7, 3)
    assert list(e.props_at_raw(q)[0]["found"]) == [1, 1]
    q[bad[0]][1] = bad[1]
    with pytest.raises(MergeTreeError) as ei:
        e.props_at_raw(q)
    assert ei.value.code == MTE_E_INVALID_ARG
    q[:] = (7, 3)
    assert list(e.props_at_raw(q)[0]["found"]) == [1, 1]


# ---- GPU: props_at ---------------------------------------------------------------

def check_props_at(e, it, views, rng):
    """Every position in [0, length + 2] of every view in one shuffled call."""
    qs = [(d, p) for d, v in enumerate(views) for p in range(v["length"] + 3)]
    rng.shuffle(qs)
    hits, props = e.props_at_raw(np.array(qs, abi.POS_QUERY_DTYPE))
    bare, none = e.props_at_raw(np.array(qs, abi.POS_QUERY_DTYPE), want_props=False)  # out_props == NULL
    assert none is None and (bare == hits).all()
    decoded = e.props_at(qs, it)
    bad, found = [], 0
    for i, (d, p) in enumerate(qs):
        w = text_model.segment_at(views[d], p)
        assert (w is None) == (p >= views[d]["length"])
        if w is None:
            ok = hits[i]["found"] == 0 and hits[i]["kind"] == 0 and not props[i].any() and decoded[i] is None
        else:
            ok = (hits[i]["found"] == 1 and hits[i]["kind"] == w[0] and tuple(int(x) for x in props[i]) == w[1] and
                  decoded[i] == it.decode_props(w[1]))
            found += 1
        if not ok or hits[i]["status"] != 0:
            bad.append(((d, p), hits[i], props[i], w))
    assert not bad, bad[:3]
    return found, len(qs) - found


@pytest.mark.gpu
def test_gpu_props_at_equals_model_on_synthetic_documents(synthetic):
    e, it, docs, stopped, views = synthetic
    found, missed = check_props_at(e, it, views, random.Random(4))
    assert found > 1000 and missed == 3 * len(views)
    kinds = {int(k) for k in e.props_at_raw(np.array([(9, p) for p in range(views[9]["length"])],
                                                     abi.POS_QUERY_DTYPE))[0]["kind"]}
    assert kinds == {0, 1, 2, 3}  # text, and markers of refType 0, 1, 2


@pytest.mark.gpu
def test_gpu_props_at_equals_model_on_vector_documents():
    abi_names()
    S = gold_set("newcalc_rounds")
    for k, e, it in replay(device_factory, S):
        pass
    views = [e.read_doc(d) for d in range(len(S["docs"]))]
    found, _ = check_props_at(e, it, views, random.Random(6))
    assert found > 2000
    assert sum(1 for v in views for _, kind, pl in v["segs"] if kind and any(pl)) > 100  # markers with properties


# ---- GPU: a local client's own view --------------------------------------------

@pytest.mark.gpu
def test_gpu_pending_insert_is_read_and_pending_removal_is_not():
    abi_names()
    inits, text = doc_inits(["abcd"], flags=DOC_NEW_LENGTH_CALC | DOC_LOCAL_CLIENT)
    it = Interner(4)
    e = device_factory(4)
    e.load_docs(inits, text)
    cl = DocClients("B", local=True)
    marker = {"marker": {"refType": 1}, "props": {"markerId": "p1", TILE_LABELS_KEY: ["pg"]}}
    bb = BatchBuilder(1, it)
    bb.add_local(0, cl, {"type": 0, "pos1": 2, "seg": marker})
    bb.add_local(0, cl, {"type": 0, "pos1": 4, "seg": "XY"})
    e.apply_batch(bb.build())
    # pending, unacked: visible to its own client
    assert e.read_texts([0, (0, 0, None, True), (0, 1, 6, True), (0, 1, 6)]) == ["abcXYd", "ab cXYd", "b cXY", "bcXY"]
    assert e.props_at([(0, 2), (0, 1), (0, 7)], it) == [marker["props"], {}, None]
    hits, _ = e.props_at_raw(np.array([(0, 2), (0, 4)], abi.POS_QUERY_DTYPE))
    assert list(hits["kind"]) == [2, 0] and list(hits["found"]) == [1, 1]
    bb = BatchBuilder(1, it)
    bb.add_local(0, cl, {"type": 1, "pos1": 0, "pos2": 1})
    bb.add_local(0, cl, {"type": 1, "pos1": 2, "pos2": 3})  # "c"
    e.apply_batch(bb.build())
    assert e.read_doc(0)["text"] == "bXYd" and e.read_doc(0)["length"] == 5
    assert e.read_texts([0, (0, 0, None, True)]) == ["bXYd", "b XYd"]  # pending removals: gone
    assert e.props_at([(0, 1), (0, 5)], it) == [marker["props"], None]
    info, _ = e.read_texts_raw(np.array([(0, 0, abi.TEXT_TO_END, 0)], abi.TEXT_QUERY_DTYPE))
    assert info["length"][0] == 5 and info["n_units"][0] == 4
    assert (e.statuses() == 0).all()
    e.close()


# ---- GPU: a big-capacity context, and one call against many ---------------------

@pytest.mark.gpu
def test_gpu_big_capacity_context_equals_model():
    abi_names()
    S = dict(gold_set("newcalc_lag16"), n_docs=2)
    st = ts.label_stream(ts.generate(S))
    e = device_factory(st["n_keys"], seg_capacity=8192)  # the chunked pass and its round phases
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    assert min(len(e.read_segments(d)[0]) for d in range(2)) > 128
    views = [e.read_doc(d) for d in range(2)]
    qs = [(d, s, t, ph) for d in range(2) for ph in (False, True) for s, t in grid(views[d]["length"], 9)]
    random.Random(5).shuffle(qs)
    assert e.read_texts(qs) == [text_model.get_text(views[d], s, t, placeholders=ph) for d, s, t, ph in qs]
    assert e.read_texts([0, 1]) == [v["text"] for v in views] and min(len(v["text"]) for v in views) > 50
    found, _ = check_props_at(e, ts.stream_interner(st), views, random.Random(8))
    assert found > 100
    e.close()


@pytest.mark.gpu
def test_gpu_one_call_for_1000_documents_equals_1000_calls():
    abi_names()
    S = {"config": 3, "n_docs": 1000, "ops_per_doc": 60, "params": dict(length_mode=2, marker_every=2, min_length=24)}
    st = ts.label_stream(ts.generate(S))
    e = device_factory(st["n_keys"])
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    rng = random.Random(11)
    qs = [(d, rng.randint(0, 10), rng.choice([None, 20, 30]), rng.random() < 0.5) for d in range(1000)]
    rng.shuffle(qs)
    batched = e.read_texts(qs)
    assert batched == [e.read_texts([q])[0] for q in qs]
    assert sum(b != "" for b in batched) > 900 and len(set(batched)) > 500
    assert e.read_texts(list(range(0, 1000, 50))) == [e.read_doc(d)["text"] for d in range(0, 1000, 50)]
    e.close()
