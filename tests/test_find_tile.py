"""Batched marker search: mte_find_tiles / DeviceEngine.find_tiles answer
SharedString.findTile (sharedString.ts:229-234 -> client.ts:1185-1188 ->
MergeTree.findTile, mergeTree.ts:1135-1163) for many documents in one device
call.

Pinned against the reference itself: tests/golden/tile_vectors.json.gz (made by
tests/golden/make_tile_golden.py through tests/golden/ref_tiles.js) holds
Client.findTile's answer for every start position, three labels and both
directions at four checkpoints of 200 generated documents whose markers carry
tile labels (tests/tile_streams.py).  tests/tile_model.py states the rule flat;
on the CPU the model over the restatements' read-outs must equal every recorded
answer (which validates vectors and model), on the GPU the kernel must -- with
all of a checkpoint's queries for all documents in one call -- and must equal
the model on synthetic documents built around the kernel's 64-slot steps, on
local-client documents with pending ops and in a big-capacity context.
"""
import copy
import ctypes as C
import functools
import gzip
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import tile_model
import tile_streams as ts
from fluidframework_amd import _native, abi
from fluidframework_amd.abi import (DOC_INIT_DTYPE, DOC_LOCAL_CLIENT, DOC_NEW_LENGTH_CALC, DOC_TREE, MTE_E_INSERT_FAILED,
                                    MTE_E_INVALID_ARG, NO_PROPS, NOT_REMOVED, PROP_DTYPE, PROPSET_DTYPE, SEG_DTYPE,
                                    TILE_HIT_DTYPE, TILE_PRECEDING, TILE_QUERY_DTYPE, MergeTreeError)
from fluidframework_amd.packing import TILE_LABELS_KEY, BatchBuilder, DocClients, Interner

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "tile_vectors.json.gz")
NEWCALC = ["newcalc_rounds", "newcalc_lag16", "newcalc_lag64"]
LEGACY = ["legacy_rounds", "legacy_lag16"]


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(GOLD, "rt", encoding="utf-8") as fh:
        return json.load(fh)


def gold_set(name):
    return next(S for S in golden()["sets"] if S["name"] == name)


def device_factory(k, **kw):
    from fluidframework_amd.engine import DeviceEngine
    return DeviceEngine(k, **kw)


def replay(factory, S, extra_flags=0):
    """Replay a vectors set's labelled stream; yields (checkpoint, engine,
    interner) after each quarter of every document's messages."""
    st = ts.label_stream(ts.generate(S))
    it = ts.stream_interner(st)
    batches, _ = ts.checkpoints(st)
    inits = st["inits"].copy()
    inits["flags"] |= extra_flags
    e = factory(st["n_keys"])
    e.load_docs(inits, st["init_text"])
    for k, b in enumerate(batches):
        e.apply_batch(b)
        assert (e.statuses() == 0).all()
        yield k, e, it


def starts(length, preceding):
    """The start positions the vectors record."""
    return list(range(length + 1)) + [length + 5] if preceding else list(range(length))


# ---- CPU: the vectors, the model, the packers, the ABI -------------------------

def test_vectors_keep_every_query_and_most_documents():
    g = golden()
    assert [S["name"] for S in g["sets"]] == NEWCALC + LEGACY and g["labels"] == ["pg", "li", "zz"]
    for S in g["sets"]:
        left_out = [d for d in S["docs"] if d["error"]]
        assert len(left_out) <= 0.10 * len(S["docs"])
        for d in S["docs"]:
            if d["error"]:
                continue
            assert len(d["cps"]) == 4
            for cp in d["cps"]:
                for label in g["labels"]:
                    pre, fol = cp["q"][label]
                    assert sum(pre[1::2]) == cp["length"] + 2 and sum(fol[1::2]) == cp["length"]
    assert os.path.getsize(GOLD) <= max(os.path.getsize(os.path.join(HERE, "golden", f))
                                        for f in os.listdir(os.path.join(HERE, "golden")) if f != "tile_vectors.json.gz")


@pytest.mark.parametrize("name", NEWCALC + LEGACY)
def test_model_over_restatement_equals_reference(name):
    """new-calc documents on the flat restatement, legacy ones on the tree's."""
    from oracle import SpecOracle
    S = gold_set(name)
    asked = 0
    for k, e, it in replay(lambda nk: SpecOracle(nk), S):
        for d, doc in enumerate(S["docs"]):
            if doc["error"]:
                continue
            cp = doc["cps"][k]
            view = e.read_doc(d)
            segs = tile_model.decoded_segs(view, it)
            assert view["length"] == cp["length"]
            assert tile_model.text_with_placeholders(view) == cp["text"]
            hits = {p: pr for p, pr in cp["hits"]}
            for label in golden()["labels"]:
                for preceding, r in zip((True, False), cp["q"][label]):
                    want = ts.unrle(r)
                    assert tile_model.tile_answers(segs, label, preceding) == want, (name, d, k, label, preceding)
                    sp = starts(cp["length"], preceding)
                    for j in sorted(set(range(0, len(sp), 5)) | set(range(max(0, len(sp) - 3), len(sp)))):
                        h = tile_model.find_tile(segs, sp[j], label, preceding)
                        assert (h[0] if h else -1) == want[j], (name, d, k, label, preceding, sp[j])
                        if h:
                            assert h[1] == 1 and h[2] == hits[h[0]]
                    asked += len(want)
    assert asked > 50000


def test_following_at_length_finds_nothing_in_the_model():
    segs = [(3, 0, {}), (1, 2, {TILE_LABELS_KEY: ["pg"]})]
    assert tile_model.find_tile(segs, 3, "pg", False) == (3, 1, {TILE_LABELS_KEY: ["pg"]})
    assert tile_model.find_tile(segs, 4, "pg", False) is None
    assert tile_model.find_tile(segs, 9, "pg", True)[0] == 3
    assert tile_model.find_tile(segs, 2, "pg", True) is None


def _label_interner():
    it = Interner(3)
    it.kv("markerId", "a")
    for v in (["pg"], ["li"], ["pg", "li"], "pg", {"pg": 1}, ["pgx"]):
        it.kv(TILE_LABELS_KEY, v)
    it.kv("other", ["pg"])  # the same array under another key: the id is shared
    it.value(["zz"])        # interned, never given to the key
    return it


def test_tile_values_picks_the_arrays_holding_the_label_and_interns_nothing():
    it = Interner(2)
    it.kv("markerId", "a")
    assert it.tile_values("pg") == (None, [])
    assert it.key_names == ["markerId"]
    it = _label_interner()
    n_values, n_keys = len(it.value_json), list(it.key_names)
    ids = {json.dumps(v): it.values[json.dumps(v, separators=(",", ":"))] for v in (["pg"], ["li"], ["pg", "li"])}
    assert it.tile_values("pg") == (1, sorted([ids['["pg"]'], ids['["pg", "li"]']]))
    assert it.tile_values("li") == (1, sorted([ids['["li"]'], ids['["pg", "li"]']]))
    assert it.tile_values("zz") == (1, []) and it.tile_values("pgx")[1] != []
    assert len(it.value_json) == n_values and it.key_names == n_keys
    full = Interner(1)
    full.kv("markerId", "a")
    assert full.tile_values("pg") == (None, [])  # n_keys is used up: still no error, nothing interned


NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_tile_values_agree_with_python():
    js = """
const { Interner } = require("./fluidframework_amd/node/packing.js");
const it = new Interner(3);
it.kv("markerId", "a");
for (const v of [["pg"], ["li"], ["pg", "li"], "pg", { pg: 1 }, ["pgx"]]) it.kv("referenceTileLabels", v);
it.kv("other", ["pg"]);
it.value(["zz"]);
const n = it.valueJson.length;
const out = ["pg", "li", "zz", "pgx"].map((l) => it.tileValues(l));
out.push(new Interner(2).tileValues("pg"), it.valueJson.length === n, it.keyNames);
console.log(JSON.stringify(out));
"""
    r = subprocess.run([NODE, "-e", js], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    it = _label_interner()
    want = [list(it.tile_values(lb)) for lb in ("pg", "li", "zz", "pgx")]
    assert got[:4] == want
    assert got[4:] == [[None, []], True, it.key_names]


def test_find_tiles_is_declared_exported_and_mirrored(tmp_path):
    assert "mte_find_tiles" in abi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path("libmte.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "mte_find_tiles" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mte.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %u\\n", sizeof(mte_tile_query), sizeof(mte_tile_hit),\n'
                   '         offsetof(mte_tile_query, key), offsetof(mte_tile_query, flags),\n'
                   '         offsetof(mte_tile_hit, status), offsetof(mte_tile_hit, ref_type), MTE_TILE_PRECEDING);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    q, h = TILE_QUERY_DTYPE.fields, TILE_HIT_DTYPE.fields
    assert got == [TILE_QUERY_DTYPE.itemsize, TILE_HIT_DTYPE.itemsize, q["key"][1], q["flags"][1], h["status"][1],
                   h["ref_type"][1], TILE_PRECEDING]
    assert C.sizeof(abi.MteTileQuery) == TILE_QUERY_DTYPE.itemsize and C.sizeof(abi.MteTileHit) == TILE_HIT_DTYPE.itemsize
    assert abi.MteTileQuery.flags.offset == q["flags"][1] and abi.MteTileHit.ref_type.offset == h["ref_type"][1]


def test_find_tiles_rejects_a_null_context_without_a_device():
    lib = _native.load_mte()
    q = np.zeros(1, TILE_QUERY_DTYPE)
    hit = np.zeros(1, TILE_HIT_DTYPE)
    assert lib.mte_find_tiles(None, q.ctypes.data, 1, None, 0, hit.ctypes.data, None) == MTE_E_INVALID_ARG
    assert lib.mte_find_tiles(None, None, 0, None, 0, None, None) == MTE_E_INVALID_ARG


# ---- GPU: the reference's answers ----------------------------------------------

def recorded_queries(S, k):
    """Every query the vectors record at checkpoint k, for every surviving
    document -> (queries, [(position, props | None)])."""
    qs, want = [], []
    for d, doc in enumerate(S["docs"]):
        if doc["error"]:
            continue
        cp = doc["cps"][k]
        hits = {p: pr for p, pr in cp["hits"]}
        for label in golden()["labels"]:
            for preceding, r in zip((True, False), cp["q"][label]):
                for p, w in zip(starts(cp["length"], preceding), ts.unrle(r)):
                    qs.append((d, p, label, preceding))
                    want.append((w, hits.get(w)))
    return qs, want


def check_vectors(name, extra_flags=0):
    S = gold_set(name)
    asked = 0
    for k, e, it in replay(device_factory, S, extra_flags):
        qs, want = recorded_queries(S, k)
        got = e.find_tiles(qs, it)  # one call: all documents, all queries of the checkpoint
        bad = [(name, k, q, g, w) for q, g, w in zip(qs, got, want)
               if (g is None) != (w[0] < 0) or (g is not None and (g["pos"], g["refType"], g["props"]) != (w[0], 1, w[1]))]
        assert not bad, bad[:3]
        asked += len(qs)
    assert asked > 50000


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEWCALC)
def test_gpu_flat_documents_equal_reference(name):
    check_vectors(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEWCALC)
def test_gpu_tree_flagged_documents_equal_reference(name):
    check_vectors(name, DOC_TREE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEGACY)
def test_gpu_legacy_documents_equal_reference(name):
    check_vectors(name)


# ---- GPU: kernel edges on synthetic documents ----------------------------------

PG, LI, BOTH = ["pg"], ["li"], ["pg", "li"]


def T(n=2):
    return ("t", n)


def M(ref_type=1, labels=None, removed=False):
    return ("m", ref_type, labels, removed)


def synthetic_docs():
    """Documents around the kernel's 64-slot steps."""
    docs = [[]]                                     # 0: no segment at all
    for nseg in (1, 63, 64, 65, 129):
        for slot in sorted({0, 63, 64, nseg - 1}):  # the only match at the step's edges and the last slot
            if slot < nseg:
                docs.append([M(1, PG) if i == slot else T() for i in range(nseg)])
    docs.append([T(), M(1, PG, removed=True), T(), M(1, LI), T()])   # a tombstone still held
    docs.append([T(), M(1, None), T()])                              # a Tile marker without the key
    docs.append([T(), M(2, PG), M(4, PG), M(0, PG), T()])            # NestBegin / NestEnd / Simple with the label
    docs.append([M(1, BOTH), T(3), M(3, LI), T(1), M(1, PG)])        # a two-label array; Tile | NestBegin
    rng = random.Random(7)
    mixed = []
    for i in range(129):                                             # everything at once, over three steps
        x = rng.random()
        mixed.append(T(rng.randint(1, 3)) if x < 0.5 else ("t", 2, True) if x < 0.6 else
                     M(rng.choice([1, 1, 1, 2]), rng.choice([PG, LI, BOTH, None]), removed=rng.random() < 0.25))
    docs.append(mixed)
    docs.append([T()])                                               # the last document is stopped below
    return docs


def load_synthetic(docs, **kw):
    it = Interner(2)
    sets, entries, segs, offs = [], [], [], [0]
    for doc in docs:
        for i, sg in enumerate(doc):
            removed = sg[-1] is True
            rs, rm = (5, 0b10) if removed else (NOT_REMOVED, 0)
            if sg[0] == "t":
                segs.append((0, sg[1], 0, rs, rm, -1, 0, NO_PROPS))
            else:
                props = {"markerId": f"m{len(segs)}"}
                if sg[2] is not None:
                    props[TILE_LABELS_KEY] = sg[2]
                first = len(entries)
                entries.extend(it.kv(k, v) for k, v in props.items())
                sets.append((first, len(entries) - first))
                segs.append((0, 1, 0, rs, rm, -1, 1 + sg[1], len(sets) - 1))
        offs.append(len(segs))
    inits = np.zeros(len(docs), DOC_INIT_DTYPE)
    inits["flags"], inits["propset"], inits["cur_seq"] = DOC_NEW_LENGTH_CALC, NO_PROPS, 10
    e = device_factory(2, **kw)
    e.load_docs(inits, np.full(4, ord("x"), np.uint16), np.array(sets, PROPSET_DTYPE), np.array(entries, PROP_DTYPE))
    e.load_segments(np.array(offs, np.uint64), np.array(segs, SEG_DTYPE))
    return e, it


def model_queries(e, it, docs, rng):
    """Both directions, three labels, every start position in [0, length + 5]
    of every document, shuffled -> (queries, model answers)."""
    qs, want = [], []
    for d in docs:
        segs = tile_model.decoded_segs(e.read_doc(d), it)
        length = sum(ln for ln, _, _ in segs)
        for label in ("pg", "li", "zz"):
            for preceding in (True, False):
                for p in range(length + 6):
                    qs.append((d, p, label, preceding))
                    want.append(tile_model.find_tile(segs, p, label, preceding))
    order = list(range(len(qs)))
    rng.shuffle(order)
    return [qs[i] for i in order], [want[i] for i in order]


def assert_equal_model(got, want, qs):
    bad = [(q, g, w) for q, g, w in zip(qs, got, want)
           if (g is None) != (w is None) or (g is not None and (g["pos"], g["refType"], g["props"]) != w)]
    assert not bad, bad[:3]


@pytest.fixture(scope="module")
def synthetic():
    docs = synthetic_docs()
    e, it = load_synthetic(docs)
    stopped = len(docs) - 1
    bb = BatchBuilder(len(docs), it)  # an insert past the end stops the last document
    bb.add_message(stopped, DocClients("A"), {"clientId": "B", "sequenceNumber": 11, "referenceSequenceNumber": 10,
                                              "minimumSequenceNumber": 0, "type": "op",
                                              "contents": {"type": 0, "pos1": 1000, "seg": "y"}})
    e.apply_batch(bb.build())
    st = e.statuses()
    assert st[stopped] == MTE_E_INSERT_FAILED and (st[:stopped] == 0).all()
    yield e, it, docs, stopped
    e.close()


@pytest.mark.gpu
def test_gpu_kernel_edges_equal_model(synthetic):
    e, it, docs, stopped = synthetic
    views = [e.read_doc(d) for d in range(stopped)]
    assert [len(v["segs"]) for v in views[:2]] == [0, 1]
    assert max(len(docs[d]) for d in range(stopped)) == 129
    qs, want = model_queries(e, it, range(stopped), random.Random(1))  # unordered, every document many times
    assert_equal_model(e.find_tiles(qs, it), want, qs)
    assert sum(w is not None for w in want) > 1000 and sum(w is None for w in want) > 1000
    # the tombstone, the marker without the key and the markers without the Tile bit are never found
    first = 1 + sum(1 for n in (1, 63, 64, 65, 129) for s in {0, 63, 64, n - 1} if s < n)
    got = e.find_tiles([(first, 9, "pg", True), (first, 0, "pg", False), (first, 9, "li", True),
                        (first + 1, 9, "pg", True), (first + 2, 9, "pg", True), (first + 2, 0, "pg", False),
                        (first + 3, 0, "li", True), (first + 3, 1, "li", False), (first + 3, 9, "pg", True)], it)
    assert [g and (g["pos"], g["refType"]) for g in got] == [None, None, (4, 1), None, None, None, (0, 1), (4, 3), (6, 1)]
    assert got[6]["props"][TILE_LABELS_KEY] == BOTH


@pytest.mark.gpu
def test_gpu_start_positions_at_and_past_the_end(synthetic):
    e, it, docs, stopped = synthetic
    d = next(i for i, doc in enumerate(docs) if len(doc) == 65 and doc[64][0] == "m")  # the match is the last unit
    length = e.read_doc(d)["length"]
    assert length == 129
    got = e.find_tiles([(d, p, "pg", pre) for pre in (True, False) for p in (0, length - 1, length, length + 5)], it)
    assert [g and g["pos"] for g in got] == [None, 128, 128, 128, 128, 128, None, None]


@pytest.mark.gpu
def test_gpu_raw_call_count_zero_no_props_no_queries_and_stopped_document(synthetic):
    e, it, docs, stopped = synthetic
    key, ids = it.tile_values("pg")
    q = np.zeros(3, TILE_QUERY_DTYPE)
    q[0] = (1, 0, key, 0, len(ids), 0)                  # found
    q[1] = (1, 0, key, 0, 0, 0)                         # count == 0: never
    q[2] = (stopped, 0, key, 0, len(ids), TILE_PRECEDING)
    hits, props = e.find_tiles_raw(q, ids)
    assert list(hits["pos"]) == [0, -1, -1] and list(hits["status"]) == [0, 0, MTE_E_INSERT_FAILED]
    assert hits["ref_type"][0] == 1 and it.decode_props(props[0])[TILE_LABELS_KEY] == PG and not props[1:].any()
    bare, none = e.find_tiles_raw(q, ids, want_props=False)  # out_props == NULL
    assert none is None and (bare == hits).all()
    empty, _ = e.find_tiles_raw(np.zeros(0, TILE_QUERY_DTYPE), ids)  # n == 0
    assert len(empty) == 0
    assert e.find_tiles([], it) == []
    with pytest.raises(MergeTreeError) as ei:
        e.find_tiles([(1, 0, "pg", True), (stopped, 0, "pg", True)], it)
    assert ei.value.code == MTE_E_INSERT_FAILED


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [("doc", 10 ** 6), ("pos", -1), ("key", 2), ("count", 3), ("first", 0xFFFFFFFF),
                                 ("flags", 2)])
def test_gpu_invalid_queries_are_refused_before_any_launch(synthetic, bad):
    e, it, docs, stopped = synthetic
    key, ids = it.tile_values("pg")
    assert len(ids) == 2
    q = np.zeros(2, TILE_QUERY_DTYPE)
    q[:] = (1, 0, key, 0, len(ids), TILE_PRECEDING)
    e.find_tiles_raw(q, ids)  # fine as it stands
    q[bad[0]][1] = bad[1]
    with pytest.raises(MergeTreeError) as ei:
        e.find_tiles_raw(q, ids)
    assert ei.value.code == MTE_E_INVALID_ARG


# ---- GPU: a local client's own view --------------------------------------------

@pytest.mark.gpu
def test_gpu_pending_insert_is_found_and_pending_removal_is_not():
    from fixtures_util import doc_inits
    inits, text = doc_inits(["abcd"], flags=DOC_NEW_LENGTH_CALC | DOC_LOCAL_CLIENT)
    it = Interner(4)
    e = device_factory(4)
    e.load_docs(inits, text)
    cl = DocClients("B", local=True)
    marker = {"marker": {"refType": 1}, "props": {"markerId": "p1", TILE_LABELS_KEY: ["pg"]}}
    bb = BatchBuilder(1, it)
    bb.add_local(0, cl, {"type": 0, "pos1": 2, "seg": marker})
    e.apply_batch(bb.build())
    got = e.find_tiles([(0, 4, "pg", True), (0, 0, "pg", False), (0, 1, "pg", True)], it)
    assert [g and g["pos"] for g in got] == [2, 2, None]  # pending, unacked: visible to its own client
    assert got[0]["props"] == marker["props"]
    bb = BatchBuilder(1, it)
    bb.add_local(0, cl, {"type": 1, "pos1": 2, "pos2": 3})
    e.apply_batch(bb.build())
    assert e.read_doc(0)["text"] == "abcd" and e.read_doc(0)["length"] == 4
    assert e.find_tiles([(0, 4, "pg", True), (0, 0, "pg", False)], it) == [None, None]  # pending removal: gone
    assert (e.statuses() == 0).all()


def labelled_farms(sets):
    """Farm sets with tile labels on their marker inserts (tests/tile_streams.py's cases, by seq)."""
    def relabel(op, seq):
        if op.get("type") == 3:
            for o in op["ops"]:
                relabel(o, seq)
        elif op.get("type") == 0 and isinstance(op.get("seg"), dict) and "marker" in op["seg"]:
            case = seq % 5
            op["seg"]["marker"]["refType"] = ts.CASE_REFTYPE[case]
            if ts.CASE_VALUE[case]:
                op["seg"].setdefault("props", {})[TILE_LABELS_KEY] = ts.LABEL_VALUES[ts.CASE_VALUE[case]]
    out = copy.deepcopy(sets)
    for s in out:
        for m in s["log"]:
            if m[5]:
                relabel(m[5], m[1])
    return out


@pytest.mark.gpu
def test_gpu_local_client_farm_equals_model_with_ops_pending():
    """Every client of three reference farms as a local-client document, tile
    labels added: after each checkpoint's batch -- local ops still pending --
    find_tiles equals the model over the same engine's read_doc."""
    import fixtures_util
    from test_local_ops import farm_sets
    from fluidframework_amd.engine import DeviceEngine
    sets = labelled_farms(farm_sets()[4:7])
    seen = {"interner": None, "asked": 0, "found": 0, "pending": 0}

    class Recording(Interner):
        def __init__(self, n_keys):
            super().__init__(n_keys)
            seen["interner"] = self

    class Checked(DeviceEngine):
        def apply_batch(self, batch):
            rc = super().apply_batch(batch)
            it = seen["interner"]
            docs = [d for d, s in enumerate(self.statuses()) if s == 0]
            assert len(docs) == self.n_docs
            qs, want = model_queries(self, it, docs, random.Random(3))
            assert_equal_model(self.find_tiles(qs, it), want, qs)
            seen["asked"] += len(qs)
            seen["found"] += sum(w is not None for w in want)
            seen["pending"] += int(np.count_nonzero(batch["ops"]["flags"] & abi.F_LOCAL))
            return rc

    orig = fixtures_util.Interner
    fixtures_util.Interner = Recording
    try:
        fixtures_util.replay_ref_farm(lambda k: Checked(k), sets)
    finally:
        fixtures_util.Interner = orig
    assert seen["asked"] > 10000 and seen["found"] > 1000 and seen["pending"] > 100


# ---- GPU: a big-capacity context, and one call against many ---------------------

@pytest.mark.gpu
def test_gpu_big_capacity_context_equals_model():
    S = dict(gold_set("newcalc_lag16"), n_docs=2)
    st = ts.label_stream(ts.generate(S))
    it = ts.stream_interner(st)
    e = device_factory(st["n_keys"], seg_capacity=8192)  # the chunked pass and its round phases
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    assert min(len(e.read_segments(d)[0]) for d in range(2)) > 128
    qs, want = model_queries(e, it, range(2), random.Random(5))
    assert_equal_model(e.find_tiles(qs, it), want, qs)
    assert sum(w is not None for w in want) > 500


@pytest.mark.gpu
def test_gpu_one_call_for_1000_documents_equals_1000_calls():
    S = {"config": 3, "n_docs": 1000, "ops_per_doc": 60, "params": dict(length_mode=2, marker_every=2, min_length=24)}
    st = ts.label_stream(ts.generate(S))
    it = ts.stream_interner(st)
    e = device_factory(st["n_keys"])
    e.load_docs(st["inits"], st["init_text"])
    e.apply_batch(st["batch"])
    assert (e.statuses() == 0).all()
    rng = random.Random(11)
    qs = [(d, rng.randint(0, 30), rng.choice(["pg", "li"]), rng.random() < 0.5) for d in range(1000)]
    rng.shuffle(qs)
    batched = e.find_tiles(qs, it)
    assert batched == [e.find_tiles([q], it)[0] for q in qs]
    assert 300 < sum(b is not None for b in batched) < 1000
