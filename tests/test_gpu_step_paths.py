"""Every ordered pair of step paths of pass 1 (seg_op_v, block_run,
mte_step1.h) back to back on one document, against the specification
(SpecOracle), bit-exact: statuses, digests, read-outs and full segment lists.

The step's wave-uniform branches (op type, "is there a split", "is there a
second split", nlen > 0, the return codes, the zam bit) merge the segment
planes of their arms.  A wrong merge shows as a value left over from the path
the *previous* op took, so a document here is a short prelude and then two ops,
one of each path, in that order; every ordered pair is a document, once with
8 segments (register tier E = 1) and once with 70 (E = 2).  A few pairs start
at 62 and at 126 segments, where the first op ends its tier (62 -> 64 hands
over to E = 2, 126 -> 128 to E = 4) and the second runs in the next one.  The
exits (MTE_E_INSERT_FAILED, a window error whose record is applied first, a
client out of range) each follow an op of another path.

The prelude gives every document a marker with a property set and two
tombstones (removed at seq 2 and seq 3), so that a rewrite finds a marker and
an END that advances minSeq finds a tombstone to drop.  Ops are written from
the restatement's segment list at that point of the document, and each case
asserts on the CPU, from that list and from the restatement's segment counts,
that its two ops take the paths it names, before anything runs on the GPU.
The documents run one per wave, and again two per wave (test_gpu_step_flags).
"""
import functools

import numpy as np
import pytest

import stream_edit as se
from flat_checks import resident_docs
from fluidframework_amd.abi import (F_MARKER, F_REWRITE, MTE_E_CLIENT_RANGE, MTE_E_INSERT_FAILED,
                                    MTE_E_MSN_GT_SEQ, MTE_MAX_CLIENTS, NO_PROPS, NOT_REMOVED, OP_ANNOTATE, OP_INSERT,
                                    OP_NOOP, OP_REMOVE)
from fluidframework_amd.engine import DeviceEngine
from oracle import OracleEngine, SpecOracle
from test_gpu_flat_variants import assert_same_segments
from test_gpu_step_flags import ONE_KEY, SEG, TWO_KEYS, Case, build_stream, rec, run, tier

PRELUDE = 3  # records ahead of the pair
# segments before the pair's first op -> preloaded segments (the prelude's marker adds one)
BODY = {1: 8, 2: 70}
EDGES = {62: 64, 126: 128}  # segments before the first op -> after it


def prelude(n0):
    """A marker with a set between segments 1 and 2, then segments 4 and
    n0 - 2 removed whole (tombstones of seq 2 and 3)."""
    a, b = SEG * 4 + 1, SEG * (n0 - 2) + 1
    return [rec(1, OP_INSERT, SEG * 2, 1, flags=F_MARKER, b=ONE_KEY), rec(2, OP_REMOVE, a, a + SEG),
            rec(3, OP_REMOVE, b, b + SEG)]


# ---- the restatement's view of a document ------------------------------------

class View:
    """The segment list every later op sees (each op's refSeq is the seq before
    it): tombstones have no length."""

    def __init__(self, segs):
        self.live = segs["removed_seq"] == NOT_REMOVED
        self.len = np.where(self.live, segs["len"], 0).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.len)])
        self.total = int(self.start[-1])
        self.marker = self.live & (segs["kind"] != 0)
        self.tomb_seqs = sorted(int(s) for s in segs["removed_seq"][~self.live])
        self.n = len(segs)

    def inside(self, p):
        """The leaf p splits (start < p < end), or None."""
        i = int(np.searchsorted(self.start, p, "right")) - 1
        while i + 1 < self.n and self.len[i] == 0:
            i += 1
        return i if i < self.n and self.start[i] < p < self.start[i] + self.len[i] else None

    def text_leaves(self, min_len):
        """Visible text leaves of at least min_len units, the middle one first."""
        idx = [i for i in range(self.n) if self.live[i] and not self.marker[i] and self.len[i] >= min_len]
        assert idx, "no leaf left to work on"
        mid = idx[len(idx) // 2]
        return sorted(idx, key=lambda i: abs(i - mid))

    def pair_of_leaves(self):
        """Two visible text leaves next to each other (tombstones may lie
        between them, the marker does not), the middle pair first."""
        idx = sorted(self.text_leaves(2))
        pairs = [(i, j) for i, j in zip(idx, idx[1:]) if not self.marker[i:j].any()]
        return min(pairs, key=lambda p: abs(p[0] + p[1] - self.n))


def classify(v, op, min_seq):
    """The path of mte_step1.h one record takes on the list `v`."""
    seq, _, msn, typ, client, flags, p1, p2, _, b = op
    if client >= MTE_MAX_CLIENTS:
        return "client_range"
    # a record that violates the window is applied, its minSeq is not
    drops = min_seq < msn <= seq and any(s <= msn for s in v.tomb_seqs)
    tail = ("_zamboni" if drops else "") + ("_msn_gt_seq" if msn > seq else "")
    if typ == OP_NOOP:
        return "noop" + tail
    if typ == OP_INSERT:
        mk = bool(flags & F_MARKER)
        kind = ("marker_set" if b != NO_PROPS else "marker_plain") if mk else ("ins" if p2 > 0 else "ins_zero")
        if v.inside(p1) is not None:
            where = "split"
        elif p1 > v.total:
            return "insert_failed"
        else:
            where = "first" if p1 == 0 else "append" if p1 == v.total else "boundary"
        return f"{kind}_{where}{tail}"
    kind = "rm" if typ == OP_REMOVE else "an"
    b1, b2 = min(p1, p2), max(p1, p2)
    l1, l2 = v.inside(b1), v.inside(b2) if b2 != b1 else None
    if p1 == p2:
        shape = "empty"
    elif l1 is not None and l1 == l2:
        shape = "same"
    else:
        shape = {(False, False): "none", (True, False): "start", (False, True): "end", (True, True): "two"}[
            (l1 is not None, l2 is not None)]
    marks = p2 > p1 and bool(((v.start[:-1] < p2) & (v.start[:-1] + v.len > p1) & (v.len > 0)).any())
    if typ == OP_ANNOTATE and (flags & F_REWRITE):
        over = bool((v.marker & (v.start[:-1] >= p1) & (v.start[:-1] < p2)).any())
        return f"an_rewrite_{'marker' if over else 'text'}_{shape}{tail}"
    return f"{kind}_{shape}{'' if marks or p1 == p2 else '_nomark'}{tail}"


# ---- the paths: name -> the op written on a view ---------------------------------

def _ins(v, where, n=3, flags=0, b=NO_PROPS):
    if where == "split":
        i = v.text_leaves(3)[0]
        pos = int(v.start[i]) + 2
    elif where == "boundary":
        i = next(i for i in v.text_leaves(1) if 0 < v.start[i] < v.total)
        pos = int(v.start[i])
    else:
        pos = 0 if where == "first" else v.total
    return dict(typ=OP_INSERT, p1=pos, p2=n, flags=flags, b=b)


def _range(v, typ, shape, flags=0, reverse=False):
    if shape == "two":
        i, j = v.pair_of_leaves()
        p1, p2 = int(v.start[i]) + 1, int(v.start[j]) + 1
    else:
        i = v.text_leaves(3)[0]
        s, e = int(v.start[i]), int(v.start[i] + v.len[i])
        p1, p2 = {"none": (s, e), "start": (s + 1, e), "end": (s, e - 1), "same": (s + 1, e - 1),
                  "empty": (s + 1, s + 1)}[shape]
    if reverse:
        p1, p2 = p2, p1
    return dict(typ=typ, p1=p1, p2=p2, flags=flags, a=TWO_KEYS if typ == OP_ANNOTATE else 0)


def _rewrite_over_marker(v):
    m = int(np.flatnonzero(v.marker)[0])
    before = max(i for i in range(m) if v.len[i] > 0)
    after = min(i for i in range(m + 1, v.n) if v.len[i] > 0)
    return dict(typ=OP_ANNOTATE, p1=int(v.start[before]), p2=int(v.start[after] + v.len[after]), flags=F_REWRITE,
                a=TWO_KEYS)


PATHS = {
    "ins_split": lambda v: _ins(v, "split"),
    "ins_boundary": lambda v: _ins(v, "boundary"),
    "ins_append": lambda v: _ins(v, "append"),
    "ins_first": lambda v: _ins(v, "first"),
    "marker_set_split": lambda v: _ins(v, "split", 1, F_MARKER, ONE_KEY),
    "marker_plain_boundary": lambda v: _ins(v, "boundary", 1, F_MARKER),
    "ins_zero_split": lambda v: _ins(v, "split", 0),
    "an_two_nomark": lambda v: _range(v, OP_ANNOTATE, "two", reverse=True),
    "an_rewrite_marker_none": _rewrite_over_marker,
    "noop": lambda v: dict(typ=OP_NOOP, p1=0, p2=0),
    "ins_split_zamboni": lambda v: dict(_ins(v, "split"), advance=True),
}
for _shape in ("none", "start", "end", "same", "two", "empty"):
    PATHS[f"rm_{_shape}"] = functools.partial(_range, typ=OP_REMOVE, shape=_shape)
    PATHS[f"an_{_shape}"] = functools.partial(_range, typ=OP_ANNOTATE, shape=_shape)
# segments an op of the path adds (the zamboni drops one tombstone)
DELTA = {"ins_split": 2, "ins_boundary": 1, "ins_append": 1, "ins_first": 1, "marker_set_split": 2,
         "marker_plain_boundary": 1, "ins_zero_split": 1, "an_two_nomark": 2, "an_rewrite_marker_none": 0, "noop": 0,
         "ins_split_zamboni": 1, "none": 0, "start": 1, "end": 1, "same": 2, "two": 2, "empty": 1}
EXITS = {"insert_failed": MTE_E_INSERT_FAILED, "ins_split_msn_gt_seq": MTE_E_MSN_GT_SEQ,
         "client_range": MTE_E_CLIENT_RANGE}
EXIT_AFTER = ("ins_split", "rm_two", "an_same", "noop", "ins_split_zamboni")
EDGE_FIRST = ("ins_split", "rm_two", "an_same")
EDGE_SECOND = ("ins_split", "ins_first", "rm_same", "an_two", "marker_set_split", "ins_split_zamboni")


def delta(path):
    return DELTA[path] if path in DELTA else DELTA[path.split("_", 1)[1]]


def write(path, v, seq, min_seq):
    """-> (the record, min_seq after it)."""
    if path in EXITS:
        o = _ins(v, "split")
        if path == "insert_failed":
            o["p1"] = v.total + 5
        kw = {"client": MTE_MAX_CLIENTS} if path == "client_range" else {}
        msn = seq + 2 if path == "ins_split_msn_gt_seq" else min_seq
        return rec(seq, OP_INSERT, o["p1"], o["p2"], msn=msn, **kw), min_seq
    o = PATHS[path](v)
    msn = min_seq
    if o.pop("advance", False):  # past the oldest tombstone left
        msn = min(s for s in v.tomb_seqs if s > min_seq)
    return rec(seq, o["typ"], o["p1"], o["p2"], flags=o["flags"] if "flags" in o else 0, a=o.get("a", 0),
               b=o.get("b", NO_PROPS), msn=msn), max(msn, min_seq)


def views_after(docs):
    """The restatement's segment list of each document (n0, records) after its records."""
    s = build_stream([Case(str(i), n0, ops) for i, (n0, ops) in enumerate(docs)])
    o = run(OracleEngine(s["n_keys"], threads=8), s)
    assert (o.statuses() == 0).all()
    return [View(o.read_segments(i)[0]) for i in range(len(docs))]


@functools.lru_cache(maxsize=None)
def reference():
    """-> (cases, stream, the specification after the batch).  A case carries
    .paths, the two paths it was written for and, asserted here, takes."""
    shapes = [(f"e{e}", n - 1) for e, n in BODY.items()] + [(f"edge{n}", n - 1) for n in EDGES]
    firsts = {nm: (list(PATHS) if nm.startswith("e") and not nm.startswith("edge") else list(EDGE_FIRST))
              for nm, _ in shapes}
    # stage 0: the list after the prelude, one probe per shape; stage 1: after each first op
    v0 = dict(zip([nm for nm, _ in shapes], views_after([(n0, prelude(n0)) for _, n0 in shapes])))
    probes, op1 = [], {}
    for nm, n0 in shapes:
        for p1 in firsts[nm]:
            r, ms = write(p1, v0[nm], PRELUDE + 1, 0)
            assert classify(v0[nm], r, 0) == p1, (nm, p1, classify(v0[nm], r, 0))
            op1[nm, p1] = (r, ms)
            probes.append((nm, n0, p1))
    v1 = dict(zip([(nm, p1) for nm, _, p1 in probes],
                  views_after([(n0, prelude(n0) + [op1[nm, p1][0]]) for nm, n0, p1 in probes])))
    cases = []
    for nm, n0 in shapes:
        edge = nm.startswith("edge")
        for p1 in firsts[nm]:
            r1, ms = op1[nm, p1]
            seconds = list(EDGE_SECOND) if edge else list(PATHS) + (list(EXITS) if p1 in EXIT_AFTER else [])
            for p2 in seconds:
                r2, _ = write(p2, v1[nm, p1], PRELUDE + 2, ms)
                assert classify(v1[nm, p1], r2, ms) == p2, (nm, p1, p2, classify(v1[nm, p1], r2, ms))
                c = Case(f"{nm}_{p1}__{p2}", n0, prelude(n0) + [r1, r2])
                c.paths, c.shape, c.status = (p1, p2), nm, EXITS.get(p2, 0)
                cases.append(c)
    s = build_stream(cases)
    assert se.stream_layout(s) == "packed"  # the packed pass 1: the flagship's kernel
    # the restatement's segment counts: the tier each op runs at, what it adds
    trace = se.nsegs_trace(s)
    for d, c in enumerate(cases):
        before = int(trace[d, PRELUDE])
        assert before == c.n + 1, c.name
        if c.shape.startswith("edge"):
            assert EDGES[before] == trace[d, PRELUDE + 1], (c.name, trace[d])
            assert tier(before) < tier(int(trace[d, PRELUDE + 1])), c.name  # the first op ends its tier
        else:
            assert tier(before) == tier(int(trace[d, PRELUDE + 1])) == int(c.shape[1:]), c.name
        assert trace[d, PRELUDE + 1] - before == delta(c.paths[0]), (c.name, trace[d])
        if not c.status:
            assert trace[d, PRELUDE + 2] - trace[d, PRELUDE + 1] == delta(c.paths[1]), (c.name, trace[d])
    o = run(SpecOracle(s["n_keys"], threads=16), s)
    np.testing.assert_array_equal(o.statuses(), [c.status for c in cases])
    return cases, s, o


@pytest.fixture(scope="module", params=[1, 2], ids=["one_per_wave", "two_per_wave"])
def replayed(request):
    """-> (the device engine after the batch, the specification for the same
    stream); one engine at a time, dropped when its tests are done."""
    cases, s, o = reference()
    if request.param == 1:
        assert len(cases) <= resident_docs()
        return run(DeviceEngine(s["n_keys"]), s), o
    n = resident_docs() + 1  # more flat documents than pass 1 holds one per wave: two per wave
    padded = build_stream(cases, pad_to=n)
    op = run(SpecOracle(padded["n_keys"], threads=16), padded)
    np.testing.assert_array_equal(op.digest()[:len(cases)], o.digest())
    return run(DeviceEngine(padded["n_keys"]), padded), op


def test_every_ordered_pair_is_a_case():
    cases, _, _ = reference()
    assert len(PATHS) >= 16 and len({c.name for c in cases}) == len(cases)
    for e in BODY:
        have = {c.paths for c in cases if c.shape == f"e{e}"}
        assert {(a, b) for a in PATHS for b in PATHS} <= have
        assert {(a, x) for a in EXIT_AFTER for x in EXITS} <= have
    for n in EDGES:
        assert len([c for c in cases if c.shape == f"edge{n}"]) == len(EDGE_FIRST) * len(EDGE_SECOND)


# ---- the split-insert merge, modelled ------------------------------------------
# seg_op_v's insert path writes a split leaf's pieces with three selects per
# slot (own ? x : kept, kept = tl ? rest : len, tl ? moved : off).  The model
# below restates that path slot by slot (flags, shift, selects) in numpy; two
# hand mutations of the selects are judged against it here, on the CPU, and
# never run on the GPU: a wrong toff can point outside the text arena.  What
# is mutated is this restatement, not the HIP source: the test shows that the
# model tells either mistake from the right selects in every case; that the GPU
# cases above would catch the same mistake in seg_op_v follows only as far as
# the model restates it (every split insert of those cases is such a case).

def split_insert_model(lens, toffs, pos, nlen, new_toff, mutant=None):
    """-> (len, toff) per slot after an insert at `pos` inside a leaf."""
    lens, toffs = np.asarray(lens, np.int64), np.asarray(toffs, np.int64)
    n = len(lens)
    lens, toffs = np.concatenate([lens, [0, 0]]), np.concatenate([toffs, [0, 0]])  # two free slots
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    x = pos - start
    sp = (x >= 1) & (x <= lens - 1)  # the leaf pos splits
    assert sp.sum() == 1
    ins = nlen > 0
    after = np.concatenate([[False], np.cumsum(sp)[:-1] > 0])  # after_flag
    nb, nb2 = np.concatenate([[False], sp[:-1]]), np.concatenate([[False, False], sp[:-2]])  # prev_flags
    d = after.astype(int) + (after & ~nb & ins)  # shift_v: new[i] = old[i - d(i)]
    src = np.arange(n + 2) - d
    lens, toffs, x = lens[src], toffs[src], x[src]
    tail = (nb2 & ins) | (nb & ~ins)
    rest, moved = lens - x, toffs + x
    kept = np.where(tail, lens, rest) if mutant == "kept_arms_swapped" else np.where(tail, rest, lens)
    out_len = np.where(sp, x, kept)
    out_toff = toffs if mutant == "tail_toff_not_written" else np.where(tail, moved, toffs)
    at = nb & ins  # put_new_v
    out_len, out_toff = np.where(at, nlen, out_len), np.where(at, new_toff, out_toff)
    return out_len[:n + (2 if ins else 1)], out_toff[:n + (2 if ins else 1)]


def split_insert_expected(lens, toffs, pos, nlen, new_toff):
    start = np.concatenate([[0], np.cumsum(lens)])
    k = int(np.searchsorted(start, pos, "right")) - 1
    x = pos - int(start[k])
    new = [(nlen, new_toff)] if nlen > 0 else []
    segs = list(zip(lens[:k], toffs[:k])) + [(x, toffs[k])] + new + [(lens[k] - x, toffs[k] + x)] + \
        list(zip(lens[k + 1:], toffs[k + 1:]))
    return np.array([s[0] for s in segs]), np.array([s[1] for s in segs])


@pytest.mark.parametrize("mutant", [None, "kept_arms_swapped", "tail_toff_not_written"])
def test_split_insert_selects_against_the_model(mutant):
    differ = total = 0
    for n in (1, 2, 8, 70):
        lens = [SEG + i % 3 for i in range(n)]
        toffs = [100 * i for i in range(n)]
        for k in sorted({0, n // 2, n - 1}):
            for nlen in (0, 3):
                pos = sum(lens[:k]) + 2
                got = split_insert_model(lens, toffs, pos, nlen, 7777, mutant)
                want = split_insert_expected(lens, toffs, pos, nlen, 7777)
                total += 1
                differ += not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
    assert differ == (total if mutant else 0), (mutant, differ, total)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["e1", "e2", "edge", "exit"])
def test_gpu_step_paths(which, replayed):
    cases, _, _ = reference()
    d, o = replayed
    if which == "exit":
        docs = [i for i, c in enumerate(cases) if c.status]
    else:
        docs = [i for i, c in enumerate(cases) if c.shape.startswith(which) and not c.status]
    assert docs
    failed = []
    for i in docs:
        try:
            assert d.statuses()[i] == o.statuses()[i] == cases[i].status
            assert np.array_equal(d.digest()[i], o.digest()[i])
            assert d.read_doc(i) == o.read_doc(i)
            assert_same_segments(o, d, [i])
        except AssertionError as e:
            failed.append((cases[i].name, str(e).strip().split("\n")[0][:80]))
    assert not failed, f"{len(failed)} of {len(docs)} cases differ: {failed[:20]}"


@pytest.mark.gpu
def test_gpu_step_paths_all_documents(replayed):
    d, o = replayed
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
