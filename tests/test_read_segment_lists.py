"""Batched summary read-out: mte_read_segment_lists /
DeviceEngine.read_segment_lists answer mte_read_segments for many documents in
one device call -- as it is (MTE_SEGS_RAW) or already dropped and coalesced the
way SnapshotV1.extractSegment (MTE_SEGS_V1) and SnapshotLegacy.extractSync
(MTE_SEGS_LEGACY) reduce it at a minSeq -- and snapshot.write_bodies,
write_v1_all and write_legacy_all build every document's summary from one read.

The chain the checks hang on: snapshot.reduce_segments states the two rules over
a raw list in closed form (no serial pass); on the CPU it is held to the
sequential writers (write_body, extract_legacy through load_bodies) on the
summary fixture strings and the replay fixtures' final states, and the closed
form of the length rule to the sequential canAppend loop; on the GPU the
kernels are held to read_segments (raw) and to reduce_segments over the same
engine's raw list (V1, legacy), on directed documents with one trap each, on
replayed documents of every owner, and through the writers to the reference's
blob digests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import snapshot_strings as ss
from fixtures_util import as_msg, doc_inits, load_fixtures, replay_farm, replay_fixtures
from fluidframework_amd import _native, abi, snapshot
from fluidframework_amd.abi import (DOC_INIT_DTYPE, DOC_NEW_LENGTH_CALC, DOC_TREE, MTE_E_INVALID_ARG, MTE_E_SEQ_ORDER,
                                    MTE_E_UNSUPPORTED, MTE_VALUE_UNEQUAL, NO_PROPS, NOT_REMOVED, PROP_DTYPE,
                                    PROPSET_DTYPE, SEG_DTYPE, MergeTreeError)
from fluidframework_amd.packing import BatchBuilder, DocClients, Interner
from oracle import OracleEngine
from test_snapshot_fixtures import CASES, FIXTURES, digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("len", "seq", "removed_seq", "removers", "client", "kind")  # all but propset and text_off


def abi_names():
    """The mirrors of the call (absent before it existed)."""
    return (abi.SEGS_QUERY_DTYPE, abi.SEGS_INFO_DTYPE, abi.MteSegsQuery, abi.MteSegsInfo, abi.SEGS_RAW, abi.SEGS_V1,
            abi.SEGS_LEGACY, abi.SEGS_DOC_MIN_SEQ)


def tree_factory(k):
    e = OracleEngine(k, tree="items")
    e.lib.oti_set_limit(e.ctx, 1 << 20)
    return e


def device_factory(k, **kw):
    from fluidframework_amd.engine import DeviceEngine
    return DeviceEngine(k, **kw)


def row_texts(segs, text):
    return [text[int(s["text_off"]): int(s["text_off"]) + int(s["len"])].tolist() if s["kind"] == 0 else None
            for s in segs]


def assert_lists_equal(got, want, what, exact=False):
    """Rows, property rows and each row's text; exact: also text_off and propset
    and the text array as a whole (raw mode)."""
    gs, gp, gt = got
    ws, wp, wt = want
    assert len(gs) == len(ws), (what, len(gs), len(ws))
    for f in FIELDS + (("text_off", "propset") if exact else ()):
        np.testing.assert_array_equal(gs[f], ws[f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(gp, wp, err_msg=f"{what}: props")
    if exact:
        np.testing.assert_array_equal(gt, wt, err_msg=f"{what}: text")
    assert row_texts(gs, gt) == row_texts(ws, wt), what
    assert len(gt) == sum(int(s["len"]) for s in gs if s["kind"] == 0), what  # n_text: the text rows' units


def body_rows(body, n_keys):
    """A body (write_body's, or extract_legacy's specs wrapped) as load_bodies'
    rows with their property rows spelled out."""
    _, text, ps, pe, _, segs = snapshot.load_bodies([body], [(0, 0)], [0], n_keys)
    props = np.zeros((len(segs), n_keys), np.uint32)
    for i, s in enumerate(segs):
        if s["propset"] != NO_PROPS:
            first, count = ps[int(s["propset"])]
            for k, v in pe[int(first): int(first) + int(count)]:
                props[i, int(k)] = v
    return segs, props, text


# ---- CPU: the ABI -------------------------------------------------------------------

def test_read_segment_lists_is_declared_exported_and_mirrored(tmp_path):
    SQ, SI, CQ, CI, RAW, V1, LEGACY, DOC_MIN = abi_names()
    assert "mte_read_segment_lists" in abi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libmte.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "mte_read_segment_lists" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    qn = ["doc", "mode", "min_seq", "flags"]
    im = ["status", "cur_seq", "min_seq", "n_segs", "n_text", "reserved", "seg_offset", "text_offset"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mte.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(mte_segs_query), sizeof(mte_segs_info));\n'
                   + '  printf("' + " ".join(["%zu"] * len(qn)) + '\\n", '
                   + ", ".join(f"offsetof(mte_segs_query, {n})" for n in qn) + ');\n'
                   + '  printf("' + " ".join(["%zu"] * len(im)) + '\\n", '
                   + ", ".join(f"offsetof(mte_segs_info, {n})" for n in im) + ');\n'
                   '  printf("%u %u %u %u\\n", MTE_SEGS_RAW, MTE_SEGS_V1, MTE_SEGS_LEGACY, MTE_SEGS_DOC_MIN_SEQ);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [[int(x) for x in ln.split()]
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]

    def offsets(dt, names):
        return [dt.fields[n][1] for n in names]

    assert got == [[SQ.itemsize, SI.itemsize], offsets(SQ, qn), offsets(SI, im), [RAW, V1, LEGACY, DOC_MIN]]
    assert got[0] == [16, 40] and got[3] == [0, 1, 2, 1]
    for st, dt, names in ((CQ, SQ, qn), (CI, SI, im)):
        assert C.sizeof(st) == dt.itemsize and [getattr(st, n).offset for n in names] == offsets(dt, names)
        assert [n for n, _ in st._fields_] == list(dt.names)
    # a null context is refused without a device
    lib = _native.load_mte()
    q, info = np.zeros(1, SQ), np.zeros(1, SI)
    ns, nt = C.c_uint64(7), C.c_uint64(7)
    assert lib.mte_read_segment_lists(None, q.ctypes.data, 1, info.ctypes.data, None, None, 0, None, 0, C.byref(ns),
                                      C.byref(nt)) == MTE_E_INVALID_ARG
    assert lib.mte_read_segment_lists(None, None, 0, None, None, None, 0, None, 0, None, None) == MTE_E_INVALID_ARG
    assert (ns.value, nt.value) == (7, 7)


# ---- CPU: the length rule in closed form ----------------------------------------------

def sequential_starts(lens, soft):
    """The writers' loop: segment i joins the run when it joins softly and
    TextSegment.canAppend allows the lengths (snapshot._can_append)."""
    starts, acc = [], None
    for ln, s in zip(lens, soft):
        cur = {"kind": 0, "text": [0x61] * ln}
        if acc is not None and s and snapshot._can_append(acc, cur):
            acc = {"kind": 0, "text": acc["text"] + cur["text"]}
            starts.append(False)
        else:
            acc = cur
            starts.append(True)
    return starts


def test_closed_form_of_the_length_rule_equals_the_sequential_loop():
    abi_names()
    rng = np.random.default_rng(20261021)
    choice = np.array([1, 2, 128, 255, 256, 257, 300, 600])
    seen_breaks = seen_joined_long = 0
    for case in range(3000):
        n = int(rng.integers(1, 14))
        lens = choice[rng.integers(0, len(choice), n)]
        if case % 3 == 0:  # mostly short ones around one or two long ones
            lens = np.where(rng.random(n) < 0.7, choice[rng.integers(0, 3, n)], lens)
        soft = rng.random(n) < 0.85
        soft[0] = False
        want = sequential_starts(lens.tolist(), soft.tolist())
        got = (~soft | snapshot.soft_joins_break(lens, soft)).tolist()
        assert got == want, (lens.tolist(), soft.tolist())
        seen_breaks += sum(1 for g, s in zip(got, soft) if g and s)
        seen_joined_long += sum(1 for g, ln in zip(got, lens) if not g and ln > 256)
    assert seen_breaks > 500 and seen_joined_long > 500  # both sides of the rule were met
    # the cases of the issue, by hand: 256 then 257 joins, 257 then 257 breaks, 300 300 10
    for lens, want in (([200, 56, 257], [True, False, False]), ([200, 57, 257], [True, False, True]),
                       ([300, 300, 10], [True, True, False]), ([300, 10, 300, 300], [True, False, True, True])):
        soft = np.array([False] + [True] * (len(lens) - 1))
        assert (~soft | snapshot.soft_joins_break(lens, soft)).tolist() == want == sequential_starts(lens, soft)


# ---- CPU: the per-document fallback against the sequential writers --------------------

def resolve(e, docs, m):
    """A minSeq choice per document: None (the document's own), a number, or a
    function of the document's window."""
    views = [e.read_doc(d) for d in docs]
    return [int(m(v)) if callable(m) else m for v in views], [int(v["min_seq"]) for v in views]


def check_fallback_against_writers(e, docs, min_seqs, what):
    """EngineBase.read_segment_lists' V1 and legacy rows against
    load_bodies([write_body]) and extract_legacy, its raw ones against
    read_segments -> (rows compared, of them with merge info)."""
    n = kept_info = 0
    for m in min_seqs:
        ms, own = resolve(e, docs, m)
        qs = [(d, mode, ms[i]) for i, d in enumerate(docs) for mode in (abi.SEGS_RAW, abi.SEGS_V1, abi.SEGS_LEGACY)]
        lists, infos = e.read_segment_lists(qs, info=True)
        for i, d in enumerate(docs):
            assert infos[3 * i]["min_seq"] == own[i]
            mm = own[i] if ms[i] is None else ms[i]
            assert_lists_equal(lists[3 * i], e.read_segments(d), (what, d, "raw"), exact=True)
            assert_lists_equal(lists[3 * i + 1], body_rows(snapshot.write_body(e, d, mm), e.n_keys), (what, d, "v1", mm))
            assert_lists_equal(lists[3 * i + 2],
                               body_rows([{"json": s} for s in snapshot.extract_legacy(e, d, mm)], e.n_keys),
                               (what, d, "legacy", mm))
            n += len(lists[3 * i + 1][0]) + len(lists[3 * i + 2][0])
            v1 = lists[3 * i + 1][0]
            kept_info += int(((v1["seq"] > 0) | (v1["removed_seq"] != NOT_REMOVED)).sum())
    return n, kept_info


def load_strings(make, cases, **kw):
    """The summary fixture strings of `cases` as documents of one engine."""
    it = ss.interner()
    bodies = [ss.body(ss.build(name), it) for _, name in cases]
    inits, text, ps, pe, offs, segs = snapshot.load_bodies(bodies, [(0, 0)] * len(bodies), [0] * len(bodies), 8)
    e = make(8, **kw)
    e.load_docs(inits, text, ps, pe)
    e.load_segments(offs, segs)
    return e, it


@pytest.mark.parametrize("make", [OracleEngine, tree_factory], ids=["oracle", "tree"])
def test_fallback_on_the_summary_fixture_strings(oracle_lib, make):
    abi_names()
    assert len(CASES) == 19
    e, _ = load_strings(make, CASES)
    assert check_fallback_against_writers(e, list(range(19)), [0, None], "strings")[0] > 19 * 4


@pytest.mark.parametrize("make", [OracleEngine, tree_factory], ids=["oracle", "tree"])
def test_fallback_on_the_replay_fixtures_final_states(oracle_lib, make):
    abi_names()
    passed, failures, e = replay_fixtures(make, check=False)
    assert not failures and e.n_docs == 30
    # the documents' own minSeq, the middle of the last round (segments and tombstones above it keep
    # their merge info), the log's end
    n, kept_info = check_fallback_against_writers(e, list(range(30)), MIN_SEQS, "replay")
    assert n > 3000 and kept_info > 1000


MIN_SEQS = [None, lambda v: v["cur_seq"] - 64, lambda v: v["cur_seq"]]


def emitted(blobs, it, key):
    for c in blobs.values():
        c[key] = [snapshot.to_json(sp, it) for sp in c[key]]
    return blobs


def assert_blobs_equal_fixture(blobs, version, name):
    want = FIXTURES[f"{version}/{name}"]
    assert sorted(blobs) == sorted(want), (version, name)
    for bid, c in blobs.items():
        meta = {k: v for k, v in c.items() if k not in ("segments", "segmentTexts")}
        assert meta == want[bid]["meta"], (version, name, bid)
        assert digest(c) == want[bid]["sha256"], (version, name, bid)


def check_writers_reproduce_the_fixtures(e, it):
    """One write_v1_all over the v1 documents, one write_legacy_all over the
    others: every blob of the 19 fixtures."""
    v1 = [i for i, (v, _) in enumerate(CASES) if v == "v1"]
    other = [i for i, (v, _) in enumerate(CASES) if v != "v1"]
    n = 0
    for docs, blobs_of, key in ((v1, snapshot.write_v1_all(e, v1, [0] * len(v1), [0] * len(v1)), "segments"),
                                (other, snapshot.write_legacy_all(e, other, [0] * len(other)), "segmentTexts")):
        assert len(blobs_of) == len(docs)
        for d, blobs in zip(docs, blobs_of):
            assert_blobs_equal_fixture(emitted(blobs, it, key), *CASES[d])
            n += len(blobs)
    assert n == 29
    # the documents' own window (0, 0) gives the same
    assert snapshot.write_v1_all(e, v1[:2]) == snapshot.write_v1_all(e, v1[:2], [0, 0], [0, 0])


def test_batched_writers_over_the_fallback_reproduce_the_fixture_digests(oracle_lib):
    abi_names()
    e, it = load_strings(OracleEngine, CASES)
    check_writers_reproduce_the_fixtures(e, it)
    # write_bodies is write_body, document by document, first_remover included
    passed, failures, r = replay_fixtures(OracleEngine, files=[0, 5, 29], check=False)
    fr = {1: (lambda seq: 2)}
    for ms in (None, [7, 30, 60]):
        got = snapshot.write_bodies(r, [0, 1, 2], ms, first_remover=fr)
        for d in range(3):
            m = r.read_doc(d)["min_seq"] if ms is None else ms[d]
            assert got[d] == snapshot.write_body(r, d, m, fr.get(d)), (d, m)


# ---- GPU: directed documents ------------------------------------------------------------

N_KEYS = 3
DOC_MIN, DOC_CUR = 10, 40     # every directed document's window
BELOW, ABOVE = 5, 30          # a removal at or below / above the window's minSeq
NL = 0x0A


class Rows:
    """One directed document: rows of (units, seq, removed_seq, removers, client, kind, props)."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def text(self, units, seq=0, rs=NOT_REMOVED, rm=0, client=-1, props=(0, 0, 0)):
        if isinstance(units, int):
            units = [0x61 + (len(self.rows) + j) % 26 for j in range(units)]
        self.rows.append((list(units), seq, rs, rm if rs != NOT_REMOVED else 0, client, 0, tuple(props)))
        return self

    def marker(self, seq=0, rs=NOT_REMOVED, rm=0, client=-1, props=(0, 0, 0), ref_type=1):
        self.rows.append((None, seq, rs, rm if rs != NOT_REMOVED else 0, client, 1 + ref_type, tuple(props)))
        return self

    def many(self, n, units=1, **kw):
        for _ in range(n):
            self.text(units, **kw)
        return self


def mixed(n):
    """n segments of every kind: markers, tombstones on both sides of minSeq,
    inserts on both sides, three property rows, a newline now and then."""
    d = Rows(f"mixed{n}")
    for i in range(n):
        seq = (0, 3, 12, 25, 0, 0, 7)[i % 7]
        rs = (NOT_REMOVED, NOT_REMOVED, BELOW + 20 * (i % 2), NOT_REMOVED, NOT_REMOVED)[i % 5] if i % 11 else ABOVE
        rs = max(rs, seq + 1) if rs != NOT_REMOVED else rs
        props = ((0, 0, 0), (1, 0, 0), (1, 0, 2))[(i // 3) % 3]
        if i % 9 == 4:
            d.marker(seq, rs, 0b101, seq % 3, props)
        else:
            units = [0x41 + (i + j) % 26 for j in range(1 + i % 5)]
            if i % 13 == 6:
                units[-1] = NL
            d.text(units, seq, rs, 1 << (i % 4), (seq % 3) if seq else -1, props)
    return d


def directed_documents():
    docs = [Rows("empty"), Rows("one").text(4), mixed(63), mixed(64), mixed(65), mixed(128), mixed(129)]
    # an eligible run across the 64-slot step: slots 60-70 joinable, their neighbours not
    d = Rows("run across the step")
    for i in range(60):
        d.text(2, props=(1 + i % 2, 0, 0))
    d.many(11, 3, props=(7, 7, 7))
    for i in range(9):
        d.text(2, props=(1 + i % 2, 0, 0))
    docs.append(d)
    docs.append(Rows("elided tombstone inside a run").text(3).text(2, seq=2, rs=BELOW, rm=2).text(4).text(1))
    docs.append(Rows("kept removed segment splits a run").text(3).text(2, seq=2, rs=ABOVE, rm=6).text(4).text(1))
    docs.append(Rows("newline").text(3).text([0x61, NL]).text(4).text([NL]).text(2))
    docs.append(Rows("marker inside a run").text(3).marker().text(4).text(2).marker(props=(1, 0, 0)).marker(props=(1, 0, 0)))
    docs.append(Rows("last key differs").text(3, props=(1, 2, 3)).text(2, props=(1, 2, 4)).text(2, props=(1, 2, 4))
                .text(2, props=(1, 2, 0)).text(2, props=(0, 2, 0)))
    nan = MTE_VALUE_UNEQUAL | 5
    docs.append(Rows("unequal value").text(3, props=(1, nan, 0)).text(2, props=(1, nan, 0)).text(2, props=(1, 0, 0))
                .text(2, props=(1, 0, 0)))
    docs.append(Rows("256 and 257 before 257").text(200).text(56).text(257).marker().text(200).text(57).text(257)
                .text(1).text(256).text(257))
    docs.append(Rows("300 300 10").text(300).text(300).text(10).text(300).text(256).text(1))
    docs.append(Rows("130 single units").many(130))
    docs.append(Rows("one of 1000").text(1000))
    docs.append(Rows("inserted below, removed above").text(3).text(2, seq=3, rs=ABOVE, rm=1, client=0).text(4)
                .text(2, seq=20, rs=ABOVE, rm=2, client=1).text(2, seq=20, client=1).text(5))
    # the step's last slot opens a run that the next step goes on with; a tombstone first in a step
    d = Rows("open row over two steps").many(63, 1, props=(1, 0, 0)).many(70, 2, props=(2, 0, 0))
    d.text(2, seq=1, rs=BELOW, rm=1).many(60, 300, props=(2, 0, 0))
    docs.append(d)
    return docs


def load_directed(make, docs, **kw):
    """load_docs + load_segments of the directed documents, every row's seq,
    removed_seq and removers as written, minSeq DOC_MIN."""
    inits = np.zeros(len(docs), DOC_INIT_DTYPE)
    inits["flags"], inits["propset"] = DOC_NEW_LENGTH_CALC, NO_PROPS
    inits["min_seq"], inits["cur_seq"] = DOC_MIN, DOC_CUR
    psets, pents, where, units, rows, offs = [], [], {}, [], [], [0]
    for d in docs:
        for t, seq, rs, rm, client, kind, props in d.rows:
            ps = NO_PROPS
            if any(props):
                if props not in where:
                    where[props] = len(psets)
                    items = [(k, v) for k, v in enumerate(props) if v]
                    psets.append((len(pents), len(items)))
                    pents.extend(items)
                ps = where[props]
            rows.append((len(units) if t is not None else 0, len(t) if t is not None else 1, seq, rs, rm, client, kind, ps))
            units.extend(t or [])
        offs.append(len(rows))
    e = make(N_KEYS, **kw)
    e.load_docs(inits, np.array(units, np.uint16), np.array(psets, PROPSET_DTYPE), np.array(pents, PROP_DTYPE))
    e.load_segments(np.array(offs, np.uint64), np.array(rows, SEG_DTYPE))
    return e


def test_directed_documents_hold_their_traps_on_the_restatement(oracle_lib):
    """The directed documents before any device: loaded into the restatement
    they read back as written, the fallback agrees with the sequential writers
    on them, and each trap does what its name says at minSeq DOC_MIN."""
    abi_names()
    docs = directed_documents()
    e = load_directed(OracleEngine, docs)
    assert (e.statuses() == 0).all()
    assert [len(e.read_segments(i)[0]) for i in range(7)] == [0, 1, 63, 64, 65, 128, 129]
    for i, d in enumerate(docs):
        segs, props, text = e.read_segments(i)
        assert [tuple(int(s[f]) for f in FIELDS[1:]) for s in segs] == [r[1:6] for r in d.rows], d.name
        assert [tuple(p) for p in props.tolist()] == [r[6] for r in d.rows], d.name
    check_fallback_against_writers(e, list(range(len(docs))), [None, 0, BELOW, 20, DOC_CUR], "directed")
    by = {d.name: i for i, d in enumerate(docs)}

    def lens(name, mode=abi.SEGS_V1, m=DOC_MIN):
        return e.read_segment_lists([(by[name], mode, m)])[0][0]["len"].tolist()

    assert lens("run across the step")[59:62] == [2, 33, 2]
    assert lens("elided tombstone inside a run") == [8]
    assert lens("kept removed segment splits a run") == [3, 2, 5]
    assert lens("kept removed segment splits a run", abi.SEGS_LEGACY) == [10]
    assert lens("newline") == [5, 5, 2]
    assert lens("marker inside a run") == [3, 1, 6, 1, 1]
    assert lens("last key differs") == [3, 4, 2, 2]
    assert lens("unequal value") == [3, 2, 4]
    assert lens("256 and 257 before 257") == [513, 1, 257, 514, 257]
    assert lens("300 300 10") == [300, 310, 557]
    assert lens("130 single units") == [130]
    assert lens("one of 1000") == [1000]
    assert lens("inserted below, removed above") == [3, 2, 4, 2, 2, 5]
    assert lens("inserted below, removed above", abi.SEGS_LEGACY) == [14]
    rows = e.read_segment_lists([(by["inserted below, removed above"], abi.SEGS_V1, DOC_MIN)])[0][0]
    assert [(int(r["seq"]), int(r["client"]), int(r["removed_seq"])) for r in rows[1:5]] == \
        [(0, -1, ABOVE), (0, -1, NOT_REMOVED), (20, 1, ABOVE), (20, 1, NOT_REMOVED)]


def model_of(e, doc, mode, m):
    return snapshot.reduce_segments(*e.read_segments(doc), mode, m)


def raw_queries(qs):
    return np.array([(d, mode, 0 if m is None else m, abi.SEGS_DOC_MIN_SEQ if m is None else 0) for d, mode, m in qs],
                    abi.SEGS_QUERY_DTYPE)


def split(info, segs, props, text):
    out = []
    for h in info:
        so, to = int(h["seg_offset"]), int(h["text_offset"])
        out.append((segs[so: so + int(h["n_segs"])], props[so: so + int(h["n_segs"])], text[to: to + int(h["n_text"])]))
    return out


def check_against_per_document_lists(e, docs, min_seqs, what, orders=1):
    """One call: every document in every mode at every minSeq; raw against
    read_segments exactly, V1 and legacy against the model over that list.
    orders > 1: the same queries reversed and shuffled, with repeats."""
    raw = {d: e.read_segments(d) for d in docs}
    qs, own = [], {}
    for m in min_seqs:
        ms, mine = resolve(e, docs, m)
        own.update(zip(docs, mine))
        qs += [(d, mode, ms[i]) for i, d in enumerate(docs) for mode in (abi.SEGS_RAW, abi.SEGS_V1, abi.SEGS_LEGACY)]
    rng = np.random.default_rng(7)
    for o in range(orders):
        if o == 1:
            qs = qs[::-1]
        elif o == 2:
            qs = [qs[i] for i in rng.permutation(len(qs))] + qs[:9]
        info, segs, props, text = e.read_segment_lists_raw(raw_queries(qs))
        assert (info["status"] == 0).all(), what
        ns, nt = info["n_segs"].astype(np.uint64), info["n_text"].astype(np.uint64)
        assert (info["seg_offset"] == np.cumsum(ns) - ns).all() and (info["text_offset"] == np.cumsum(nt) - nt).all()
        assert len(segs) == ns.sum() and len(text) == nt.sum() and props.shape == (len(segs), e.n_keys)
        assert (segs["propset"] == NO_PROPS).all()
        for i, (got, (d, mode, m)) in enumerate(zip(split(info, segs, props, text), qs)):
            assert int(info[i]["min_seq"]) == own[d]
            if mode == abi.SEGS_RAW:
                assert_lists_equal(got, raw[d], (what, d, "raw"), exact=True)
            else:
                mm = own[d] if m is None else m
                assert_lists_equal(got, snapshot.reduce_segments(*raw[d], mode, mm), (what, d, mode, mm), exact=True)
    return raw


@pytest.fixture(scope="module")
def directed():
    abi_names()
    docs = directed_documents()
    e = load_directed(device_factory, docs, seg_capacity=320)
    assert (e.statuses() == 0).all()
    yield e, docs
    e.close()


@pytest.mark.gpu
def test_gpu_directed_documents_raw_v1_and_legacy_in_every_order(directed):
    e, docs = directed
    raw = check_against_per_document_lists(e, list(range(len(docs))), [None, 0, BELOW, 20, DOC_CUR], "directed", orders=3)
    assert [len(raw[i][0]) for i in range(7)] == [0, 1, 63, 64, 65, 128, 129]
    for i, d in enumerate(docs):  # the documents are the ones written down
        assert [tuple(int(s[f]) for f in FIELDS[1:]) for s in raw[i][0]] == [r[1:6] for r in d.rows], d.name
    # and through the decoding call and the writers
    ids = list(range(len(docs)))
    lists = e.read_segment_lists([(d, abi.SEGS_V1, None) for d in ids])
    for d in ids:
        assert_lists_equal(lists[d], snapshot.reduce_segments(*raw[d], abi.SEGS_V1, DOC_MIN), (d, "decoded"), exact=True)
    fr = {10: (lambda seq: 2)}
    assert snapshot.write_bodies(e, ids, first_remover=fr) == [snapshot.write_body(e, d, DOC_MIN, fr.get(d)) for d in ids]
    assert snapshot.write_v1_all(e, ids, [20] * len(ids)) == [snapshot.write_v1(e, d, 20, DOC_CUR) for d in ids]
    assert snapshot.write_legacy_all(e, ids) == [snapshot.write_legacy(e, d, DOC_MIN) for d in ids]


# ---- GPU: replayed documents of every owner ------------------------------------------------

def replay_all_owners(make):
    """The 30 replay fixtures three times in one context: flat (new length
    calculation), MTE_DOC_TREE and legacy (tree pass) documents."""
    fx = load_fixtures()
    flags = [DOC_NEW_LENGTH_CALC] * 30 + [DOC_NEW_LENGTH_CALC | DOC_TREE] * 30 + [0] * 30
    inits, text = doc_inits([fx[d % 30]["rounds"][0]["initialText"] for d in range(90)])
    inits["flags"] = flags
    it = Interner(8)
    e = make(8)
    e.load_docs(inits, text)
    clients = [DocClients("A", tree=bool(f & DOC_TREE)) for f in flags]
    for r in range(max(len(f["rounds"]) for f in fx)):
        bb = BatchBuilder(90, it)
        for d in range(90):
            if r < len(fx[d % 30]["rounds"]):
                for m in fx[d % 30]["rounds"][r]["msgs"]:
                    bb.add_message(d, clients[d], as_msg(m))
        e.apply_batch(bb.build())
    return e


@pytest.mark.gpu
def test_gpu_replayed_documents_of_every_owner():
    abi_names()
    e = replay_all_owners(device_factory)
    try:
        assert (e.statuses() == 0).all()
        raw = check_against_per_document_lists(e, list(range(90)), MIN_SEQS, "owners")
        assert min(len(raw[d][0]) for d in range(90)) > 20 and sum(len(raw[d][0]) for d in range(90)) > 10000
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_local_client_farm_final_state():
    abi_names()
    passed, failures, e = replay_farm(device_factory, files=[0, 7, 19])
    try:
        assert not failures and (e.statuses() == 0).all() and e.n_docs > 9
        check_against_per_document_lists(e, list(range(e.n_docs)), MIN_SEQS[:2], "farm")
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_document_after_carried_round_phases():
    """Three runs in one launch (test_gpu_round_paths case g): the second and
    third run are taken from the carried layout, whose tombstones at or below
    minSeq come back to the flat planes; the lists leave them out."""
    abi_names()
    from test_gpu_round_paths import build, oracle_of, run_all
    c = build("g-one-batch")
    o = oracle_of(c)
    e = device_factory(0, seg_capacity=c.cap)
    try:
        e.set_stats(False)
        assert run_all(e, c, device=True)[0] > 0  # the round phases ran
        assert e.statuses().tolist() == c.status
        raw = check_against_per_document_lists(e, [0], [None, 300, 600, 900], "rounds")
        for x, y in zip(raw[0], o.read_segments(0)):
            np.testing.assert_array_equal(x, y)
        assert (raw[0][0]["removed_seq"] > e.read_doc(0)["min_seq"]).all() and len(raw[0][0]) > 3000
    finally:
        e.close()


# ---- GPU: the writers against the reference's blobs ------------------------------------------

@pytest.mark.gpu
def test_gpu_batched_writers_reproduce_the_fixture_digests():
    abi_names()
    e, it = load_strings(device_factory, CASES, seg_capacity=16384)
    try:
        check_writers_reproduce_the_fixtures(e, it)
    finally:
        e.close()


# ---- GPU: size-then-fill, refusals, statuses -------------------------------------------------

def call(e, q, seg_cap, text_cap, segs=True, props=True, text=True):
    info = np.full(len(q) * 40, 0x55, np.uint8).view(abi.SEGS_INFO_DTYPE)
    bs = np.full(max(seg_cap, 1) * 32, 0x5a, np.uint8).view(SEG_DTYPE)
    bp = np.full(max(seg_cap, 1) * e.n_keys, 0x5a5a5a5a, np.uint32)
    bt = np.full(max(text_cap, 1), 0x5a5a, np.uint16)
    ns, nt = C.c_uint64(77), C.c_uint64(77)
    rc = e.lib.mte_read_segment_lists(e.ctx, q.ctypes.data if len(q) else None, len(q), info.ctypes.data,
                                      bs.ctypes.data if segs else None, bp.ctypes.data if props else None, seg_cap,
                                      bt.ctypes.data if text else None, text_cap, C.byref(ns), C.byref(nt))
    return rc, info, bs, bp, bt, ns.value, nt.value


def untouched(bs, bp, bt):
    return (bs.view(np.uint8) == 0x5a).all() and (bp == 0x5a5a5a5a).all() and (bt == 0x5a5a).all()


@pytest.mark.gpu
def test_gpu_size_then_fill(directed):
    e, docs = directed
    q = raw_queries([(5, abi.SEGS_RAW, None), (16, abi.SEGS_V1, None), (0, abi.SEGS_RAW, None), (17, abi.SEGS_LEGACY, 0)])
    want = [e.read_segments(5), model_of(e, 16, abi.SEGS_V1, DOC_MIN), e.read_segments(0), model_of(e, 17, abi.SEGS_LEGACY, 0)]
    ns, nt = sum(len(w[0]) for w in want), sum(len(w[2]) for w in want)
    assert ns > 128 and nt > 1000
    for seg_cap, text_cap, kw in ((0, 0, {}), (ns - 1, nt, {}), (ns, nt - 1, {}), (ns, nt, {"segs": False}),
                                  (ns, nt, {"props": False}), (ns, nt, {"text": False})):
        rc, info, bs, bp, bt, gs, gt = call(e, q, seg_cap, text_cap, **kw)
        assert rc == 0 and (gs, gt) == (ns, nt) and untouched(bs, bp, bt), (seg_cap, text_cap, kw)
        assert info["n_segs"].tolist() == [len(w[0]) for w in want] and info["n_text"].tolist() == [len(w[2]) for w in want]
        assert (info["status"] == 0).all() and (info["cur_seq"] == DOC_CUR).all() and (info["min_seq"] == DOC_MIN).all()
    rc, info, bs, bp, bt, gs, gt = call(e, q, ns, nt)
    assert rc == 0 and (gs, gt) == (ns, nt)
    for got, w in zip(split(info, bs[:ns], bp[: ns * N_KEYS].reshape(ns, N_KEYS), bt[:nt]), want):
        assert_lists_equal(got, w, "exact capacity", exact=True)
    # no queries: nothing launched, totals zero
    rc, info, bs, bp, bt, gs, gt = call(e, raw_queries([]), 4, 4)
    assert rc == 0 and (gs, gt) == (0, 0) and untouched(bs, bp, bt)
    assert e.read_segment_lists([]) == [] and e.read_segment_lists([], info=True) == ([], [])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["doc", "mode", "flag", "min_seq", "totals"])
def test_gpu_invalid_queries_are_refused_before_any_launch(directed, bad):
    e, docs = directed
    q = raw_queries([(1, abi.SEGS_RAW, None), (2, abi.SEGS_V1, 3), (3, abi.SEGS_LEGACY, 3)])
    if bad == "doc":
        q[1]["doc"] = len(docs)
    elif bad == "mode":
        q[1]["mode"] = 3
    elif bad == "flag":
        q[1]["flags"] = 2
    elif bad == "min_seq":
        q[1]["min_seq"] = -1
    if bad == "totals":
        info = np.zeros(3, abi.SEGS_INFO_DTYPE)
        nt = C.c_uint64()
        assert e.lib.mte_read_segment_lists(e.ctx, q.ctypes.data, 3, info.ctypes.data, None, None, 0, None, 0, None,
                                            C.byref(nt)) == MTE_E_INVALID_ARG
        assert e.lib.mte_read_segment_lists(e.ctx, q.ctypes.data, 3, None, None, None, 0, None, 0, C.byref(nt),
                                            C.byref(nt)) == MTE_E_INVALID_ARG
    else:
        rc, info, bs, bp, bt, gs, gt = call(e, q, 4096, 1 << 16)
        assert rc == MTE_E_INVALID_ARG and (gs, gt) == (77, 77) and untouched(bs, bp, bt)
        assert (info.view(np.uint8) == 0x55).all()
        msg = e.lib.mte_last_error(e.ctx).decode()
        assert "mte_read_segment_lists" in msg and "query 1" in msg, msg
        with pytest.raises(MergeTreeError) as ei:
            e.read_segment_lists_raw(q)
        assert ei.value.code == MTE_E_INVALID_ARG
    # a negative min_seq under MTE_SEGS_DOC_MIN_SEQ is not looked at, and a valid call still works
    q = raw_queries([(2, abi.SEGS_V1, None)])
    q[0]["min_seq"] = -5
    info, segs, props, text = e.read_segment_lists_raw(q)
    assert_lists_equal((segs, props, text), model_of(e, 2, abi.SEGS_V1, DOC_MIN), "valid", exact=True)


def remote(cid, seq, contents, ref_seq=0):
    return {"clientId": cid, "sequenceNumber": seq, "referenceSequenceNumber": ref_seq, "minimumSequenceNumber": 0,
            "type": "op", "contents": contents}


@pytest.mark.gpu
def test_gpu_stopped_and_wide_remover_documents_answer_their_status_beside_others():
    """Document 0 is served; 1 stops on an out-of-order seq; 2 holds a segment
    removed by short id 40 (the vectors of tests/test_many_clients.py), which
    mte_seg.removers cannot carry; 3 holds 40 clients but no such removal."""
    abi_names()
    inits, text = doc_inits(["abc"] * 4, flags=DOC_NEW_LENGTH_CALC | DOC_TREE)
    e = device_factory(0)
    try:
        e.load_docs(inits, text)
        cls = [DocClients("obs", tree=True) for _ in range(4)]
        bb = BatchBuilder(4, Interner(0))
        bb.add_message(0, cls[0], remote("c0", 1, {"type": 0, "pos1": 1, "seg": "xy"}))
        bb.add_message(1, cls[1], remote("c0", 5, {"type": 0, "pos1": 0, "seg": "x"}))
        bb.add_message(1, cls[1], remote("c0", 3, {"type": 0, "pos1": 0, "seg": "y"}))
        for d in (2, 3):
            for i in range(40):
                bb.add_message(d, cls[d], remote(f"c{i}", i + 1, {"type": 0, "pos1": 0, "seg": "x"}))
        bb.add_message(2, cls[2], remote("c39", 41, {"type": 1, "pos1": 39, "pos2": 40}, ref_seq=40))
        bb.add_message(3, cls[3], remote("c3", 41, {"type": 1, "pos1": 39, "pos2": 40}, ref_seq=40))
        e.apply_batch(bb.build())
        assert e.statuses().tolist() == [0, MTE_E_SEQ_ORDER, 0, 0] and cls[2].ids["c39"] == 40
        with pytest.raises(MergeTreeError) as ei:
            e.read_segments(2)
        assert ei.value.code == MTE_E_UNSUPPORTED
        for mode in (abi.SEGS_RAW, abi.SEGS_V1, abi.SEGS_LEGACY):
            qs = [(2, mode, None), (0, mode, None), (1, mode, None), (3, mode, 41), (2, mode, 41)]
            info, segs, props, text = e.read_segment_lists_raw(raw_queries(qs))
            assert info["status"].tolist() == [MTE_E_UNSUPPORTED, 0, MTE_E_SEQ_ORDER, 0, MTE_E_UNSUPPORTED]
            assert info["n_segs"][[0, 2, 4]].tolist() == [0, 0, 0] and info["n_text"][[0, 2, 4]].tolist() == [0, 0, 0]
            got = split(info, segs, props, text)
            for i in (1, 3):
                d, _, m = qs[i]
                assert_lists_equal(got[i], model_of(e, d, mode, 0 if m is None else m), (d, mode), exact=True)
            assert len(segs) == info["n_segs"][1] + info["n_segs"][3]
            for bad, code in ((0, MTE_E_UNSUPPORTED), (2, MTE_E_SEQ_ORDER)):
                with pytest.raises(MergeTreeError) as ei:
                    e.read_segment_lists([qs[1], qs[bad]])
                assert ei.value.code == code
        assert len(e.read_segments(1)[0]) > 0  # the per-document call still serves the stopped document
    finally:
        e.close()


# ---- GPU: a thousand documents in one call -----------------------------------------------------

@pytest.mark.gpu
def test_gpu_a_thousand_documents_in_one_call():
    abi_names()
    from fluidframework_amd import gen
    s = gen.generate(3, n_docs=1000, ops_per_doc=60)
    e = device_factory(s["n_keys"], seg_capacity=256)
    try:
        e.load_docs(s["inits"], s["init_text"])
        e.apply_batch(s["batch"])
        assert (e.statuses() == 0).all()
        docs = list(range(1000))
        lists, infos = e.read_segment_lists([(d, abi.SEGS_RAW, None) for d in docs], info=True)
        v1 = e.read_segment_lists([(d, abi.SEGS_V1, None) for d in docs])
        rows = 0
        for d in docs:
            raw = e.read_segments(d)
            assert_lists_equal(lists[d], raw, (d, "raw"), exact=True)
            assert_lists_equal(v1[d], snapshot.reduce_segments(*raw, abi.SEGS_V1, infos[d]["min_seq"]), (d, "v1"), exact=True)
            rows += len(raw[0])
        assert rows > 20000
    finally:
        e.close()
