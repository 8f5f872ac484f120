"""The shift of pass 1's step at two slots per lane (shift_v, E = 2,
mte_step1.h), the split bookkeeping next to it at one slot per lane, and the
record words block_run reads late, case by case against the specification
(SpecOracle), bit-exact: statuses, digests, read-outs and the full segment
lists.

At E = 2 slot j of lane l holds segment 2l + j.  A shifting op moves every
plane by d(i) = (i > t1) + (i > t2) slots, so a lane's two slots move by one of
(0,0), (0,1), (1,1), (1,2), (2,2), and each plane is pulled across lanes twice
and selected twice.  Which pairs a case produces follows from where its
thresholds fall, so the shift cases put the first split leaf (or the insert
slot) at slot 0 and at slot 1 of lanes 0, 1, 31, 32, 62 and of the document's
last occupied lane, in bodies of 63, 64, 65, 96, 124, 125 and 126 four-unit
segments: 126 + 2 fills the tier's 128 slots exactly, and every case that ends
at 127 or 128 segments goes on with one or two ops that run at E = 4.  Every document
is one case: the body, then at most three records.  The context's markers
carry an id of 1000, so the kernel is the flagship's: four keys packed in one
plane, the marker id riding in the marker's `toff` register through every
shift ("side3", tests/stream_edit.py pass1_layout).

Before anything runs on the GPU each case asserts on the CPU, from the segment
lengths at its checked op and the restatement's segment counts, which leaves
it splits, the slot and lane of the first, the segments it adds, and the
(d0, d1) pairs its shift produces; all five pairs occur, each at the lanes
listed in `test_cases_reach_their_conditions`.

The record cases (a block of 64 records whose only minSeq advance sits at one
record; an insert's property-set word after an insert without one) are scripts
of tests/test_gpu_block_decode.py's Doc.  The soak replays 64 generated
documents of the flagship's configuration, which cross the E = 1 / E = 2 border
many times, in one batch and in four, against the restatement.

The documents run one per wave, and again two per wave.
"""
import functools

import numpy as np
import pytest

import stream_edit as se
import test_gpu_block_decode as bd
import test_gpu_step_flags as sf
from flat_checks import resident_docs
from fluidframework_amd import gen
from fluidframework_amd.abi import F_REWRITE, NO_PROPS, OP_ANNOTATE, OP_INSERT, OP_REMOVE
from fluidframework_amd.engine import DeviceEngine
from oracle import OracleEngine, SpecOracle
from test_gpu_flat_variants import assert_same_segments
from test_gpu_step_flags import SEG, ins, marker, rng, tier

pytestmark = pytest.mark.gpu

E2_SIZES = (63, 64, 65, 96, 124, 125, 126)
LANES = (0, 1, 31, 32, 62)
MARKER_ID = 1000  # above a byte: the marker id is the context's side key
INF = 1 << 30
PAIRS = ((0, 0), (0, 1), (1, 1), (1, 2), (2, 2))
MAX_RECORDS = 3


class Case:
    """One document: `body` preloaded segments, `ops`, the checked op at index
    `at`; `lens`: the segment lengths the checked op finds; `lane` / `slot`:
    where its first split leaf (`first`: or its insert slot) must sit; `e`: the
    tier it runs at."""

    def __init__(self, name, body, ops, lens, lane, slot, at=0, e=2):
        self.name, self.body, self.ops, self.lens = name, body, list(ops), list(lens)
        self.lane, self.slot, self.at, self.e = lane, slot, at, e


def thresholds(lens, op):
    """-> (t1, t2, added, first): the op's shift moves slot i by (i > t1) +
    (i > t2) (seg_op_v: ensureIntervalBoundary at each end, insertingWalk),
    adds `added` segments; first = the first split leaf, or the insert slot."""
    starts = np.concatenate([[0], np.cumsum(lens)])
    typ, flags, pos1, pos2 = op[3], op[5], op[6], op[7]

    def leaf_split_by(p):
        k = int(np.searchsorted(starts, p, "right")) - 1
        return k if k < len(lens) and starts[k] < p < starts[k + 1] else None

    if typ == OP_INSERT:
        k = leaf_split_by(pos1)
        nlen = 1 if flags & sf.F_MARKER else pos2
        if k is not None:
            return (k, k + 1, 2, k) if nlen > 0 else (k, INF, 1, k)
        assert nlen > 0
        k = int(np.searchsorted(starts[:-1], pos1, "left"))  # before the first leaf that starts at or after pos1
        return (k - 1, INF, 1, k) if k < len(lens) else (INF, INF, 1, None)
    hit = [k for k in (leaf_split_by(p) for p in sorted({pos1, pos2})) if k is not None]
    if not hit:
        return INF, INF, 0, None
    if len(hit) == 1:
        return hit[0], INF, 1, hit[0]
    return hit[0], hit[1] + 1, 2, hit[0]


def lane_pairs(t1, t2, n_after):
    """{(d0, d1): lanes} over the lanes the document occupies after the op."""
    d = lambda i: int(i > t1) + int(i > t2)
    out = {}
    for lane in range((n_after + 1) // 2):
        out.setdefault((d(2 * lane), d(2 * lane + 1)), set()).add(lane)
    return out


def leaves(n):
    """(lane, slot, leaf) of the listed lanes and the last occupied one."""
    out = []
    for lane in sorted(set(LANES) | {(n - 1) // 2}):
        for slot in (0, 1):
            if 2 * lane + slot < n:
                out.append((lane, slot, 2 * lane + slot))
    return out


def shift_cases(n):
    out = []
    mid = lambda k: SEG * k + 2
    for lane, slot, k in leaves(n):
        def add(name, *ops):
            out.append(Case(f"n{n}_{name}_l{lane}s{slot}", n, ops, [SEG] * n, lane, slot))

        add("ins_text", ins(1, mid(k)))
        add("ins_zero_length", ins(1, mid(k), 0))
        add("marker", marker(1, mid(k)))
        add("ins_between", ins(1, SEG * k))
        add("rm_one_end", rng(1, OP_REMOVE, mid(k), SEG * (k + 1)))
        ends = {"same": SEG * k + 3}
        if k + 1 < n:
            ends["adjacent"] = mid(k + 1)
        if k + 2 < n:
            ends["two_apart"] = mid(k + 2)
        if k + 3 < n:
            ends["far"] = mid(n - 1)
        for j, (nm, p2) in enumerate(ends.items()):
            p1 = SEG * k + 1 if nm == "same" else mid(k)
            typ, tn = ((OP_REMOVE, "rm"), (OP_ANNOTATE, "an"))[(j + slot) % 2]
            add(f"{tn}_{nm}", rng(1, typ, p1, p2))
            add(f"rev_rm_{nm}", rng(1, OP_REMOVE, p2, p1))
            add(f"rev_an_{nm}", rng(1, OP_ANNOTATE, p2, p1, flags=F_REWRITE))
    return out


def side_cases(n):
    """A marker appended first (it holds the side key, in its toff register),
    then a rewrite at the shift positions: beside the marker (shifted by two,
    kept), over it (shifted by one, cleared), reversed (shifted, kept)."""
    out = []
    body = n - 1
    lens = [SEG] * body + [1]
    end = SEG * body + 1
    for lane, slot, k in leaves(body):
        for nm, p1, p2 in (("keep", SEG * k + 1, SEG * k + 3), ("clear", SEG * k + 2, end),
                           ("reversed", end, SEG * k + 2)):
            ops = [marker(1, SEG * body), rng(2, OP_ANNOTATE, p1, p2, flags=F_REWRITE)]
            out.append(Case(f"side{n}_{nm}_l{lane}s{slot}", body, ops, lens, lane, slot, at=1))
    return out


def e1_cases():
    """One slot per lane: the first split at lanes 0, 1, 31, 32, 61, the second
    0, 1, 2 and 3 slots behind it."""
    out = []
    n = 62
    for k in (0, 1, 31, 32, 61):
        for dist in (0, 1, 2, 3):
            if k + dist >= n:
                continue
            p1 = SEG * k + 1
            p2 = SEG * k + 3 if dist == 0 else SEG * (k + dist) + 2
            for tn, typ, a, b, fl in (("rm", OP_REMOVE, p1, p2, 0), ("an", OP_ANNOTATE, p1, p2, 0),
                                      ("rev_an", OP_ANNOTATE, p2, p1, F_REWRITE)):
                out.append(Case(f"e1_{tn}_dist{dist}_l{k}", n, [rng(1, typ, a, b, flags=fl)], [SEG] * n, k, 0, e=1))
        out.append(Case(f"e1_ins_text_l{k}", n, [ins(1, SEG * k + 2)], [SEG] * n, k, 0, e=1))
        out.append(Case(f"e1_ins_between_l{k}", n, [ins(1, SEG * k)], [SEG] * n, k, 0, e=1))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for n in E2_SIZES:
        out += shift_cases(n) + side_cases(n)
    out += e1_cases()
    for c in out:
        t1, t2, added, _ = thresholds(c.lens, c.ops[c.at])
        c.leaves_tier = c.e == 2 and len(c.lens) + added + 2 > 128
        if c.leaves_tier:  # the records left go to ops at E = 4
            s = len(c.ops)
            c.ops += [ins(s + 1, 2), rng(s + 2, OP_ANNOTATE, 1, SEG * 3)][:MAX_RECORDS - s]
        assert len(c.ops) <= MAX_RECORDS
    assert len({c.name for c in out}) == len(out)
    return out


GROUPS = tuple(f"n{n}" for n in E2_SIZES) + ("side", "e1")


def build_stream(cases, pad_to=0):
    """test_gpu_step_flags' stream of the cases, its markers' id above a byte."""
    s = sf.build_stream([sf.Case(c.name, c.body, c.ops) for c in cases], pad_to=pad_to)
    props = s["batch"]["props"]
    props["value"][props["key"] == se.KEY_MARKER_ID] = MARKER_ID
    return s


@functools.lru_cache(maxsize=None)
def reference():
    """-> (cases, stream, the specification after the batch, {pair: lanes}); every
    case has reached its condition, or this fails."""
    cases = all_cases()
    s = build_stream(cases)
    assert se.stream_layout(s) == f"side{se.KEY_MARKER_ID}"
    trace = se.nsegs_trace(s)
    loaded = SpecOracle(s["n_keys"], threads=16)
    loaded.load_docs(s["inits"], s["init_text"])
    loaded.load_segments(*s["segs"])
    seen = {p: set() for p in PAIRS}
    for d, c in enumerate(cases):
        segs = loaded.read_segments(d)[0]
        assert len(segs) == c.body == trace[d, 0] and (segs["len"] == SEG).all(), c.name
        n = len(c.lens)
        assert trace[d, c.at] == n and tier(n) == c.e, (c.name, trace[d, :c.at + 1])
        if c.at:  # the marker before the checked op went to the end
            assert c.at == 1 and n == c.body + 1 and c.lens[-1] == 1, c.name
        t1, t2, added, first = thresholds(c.lens, c.ops[c.at])
        assert trace[d, c.at + 1] - n == added, (c.name, trace[d, c.at:c.at + 2])
        assert first is not None and first % c.e == c.slot and first // c.e == c.lane, (c.name, first)
        assert n + added <= 64 * c.e, c.name  # the op runs at its tier
        if c.e == 2:
            got = lane_pairs(t1, t2, n + added)
            assert set(got) <= set(PAIRS), (c.name, sorted(got))
            for p, lanes in got.items():
                seen[p] |= lanes
            assert c.leaves_tier == (tier(n + added) == 4), c.name
            if c.leaves_tier:
                assert len(c.ops) == MAX_RECORDS and tier(int(trace[d, c.at + 2])) == 4, c.name
    o = sf.run(SpecOracle(s["n_keys"], threads=16), s)
    assert (o.statuses() == 0).all(), [c.name for c, st in zip(cases, o.statuses()) if st]
    # the rewrite over the marker cleared its id, the others kept it
    cleared = se.docs_with_cleared_markers(o, [d for d, c in enumerate(cases) if c.name.startswith("side")])
    assert cleared == {d for d, c in enumerate(cases) if c.name.startswith("side") and "_clear_" in c.name}
    return cases, s, o, seen


@functools.lru_cache(maxsize=None)
def replayed(group):
    """-> (the device engine after the batch, the specification for the same stream)."""
    cases, s, o, _ = reference()
    if group == 1:
        assert len(cases) <= resident_docs()
        return sf.run(DeviceEngine(s["n_keys"]), s), o
    n = resident_docs() + 1  # more flat documents than pass 1 holds one per wave: two per wave
    assert min(8, (n + resident_docs() - 1) // resident_docs()) == 2
    padded = build_stream(cases, pad_to=n)
    op = sf.run(SpecOracle(padded["n_keys"], threads=16), padded)
    np.testing.assert_array_equal(op.digest()[:len(cases)], o.digest())
    return sf.run(DeviceEngine(padded["n_keys"]), padded), op


def differing(d, o, docs, names, status=None):
    failed = []
    for i in docs:
        try:
            assert d.statuses()[i] == o.statuses()[i] == (0 if status is None else status[i])
            assert np.array_equal(d.digest()[i], o.digest()[i])
            assert d.read_doc(i) == o.read_doc(i)
            assert_same_segments(o, d, [i])
        except AssertionError as e:
            failed.append((names[i], str(e).strip().split("\n")[0][:80]))
    return failed


def test_cases_reach_their_conditions():
    cases, _, _, seen = reference()
    # every pair, at the lanes next to the listed split lanes and at the wave's last lane
    assert seen[(0, 1)] >= {0, 1, 31, 32, 62}
    assert seen[(1, 2)] >= {1, 2, 32, 33, 63}
    assert seen[(1, 1)] >= {1, 2, 32, 33, 63}
    assert seen[(2, 2)] >= {1, 2, 32, 33, 63}
    assert seen[(0, 0)] >= {0, 30, 31, 61}
    ends = {len(c.lens) + thresholds(c.lens, c.ops[c.at])[2] for c in cases if c.e == 2}
    assert max(ends) == 128 and {127, 128} <= ends  # the tier's last slot is used
    for n in E2_SIZES:
        assert sum(c.name.startswith(f"n{n}_") for c in cases) >= 70


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("which", GROUPS)
def test_gpu_e2_pull_shift(which, group):
    cases, _, _, _ = reference()
    d, o = replayed(group)
    docs = [i for i, c in enumerate(cases) if c.name.startswith(which + "_") or
            (which == "side" and c.name.startswith("side"))]
    assert docs
    failed = differing(d, o, docs, [c.name for c in cases])
    assert not failed, f"{len(failed)} of {len(docs)} cases differ: {failed[:20]}"


@pytest.mark.parametrize("group", [1, 2])
def test_gpu_e2_pull_shift_all_documents(group):
    d, o = replayed(group)
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())


# ---- record words read late ---------------------------------------------------

LAYOUT = "side3"


def record_cases():
    out = []
    # a block of 64 records whose only minSeq advance (two preloaded tombstones leave) sits at one record
    for p in (0, 63):
        d = bd.Doc(f"advance_only_at{p}", 8, tomb=(2, 5)).fill(p).advance(bd.CUR0)
        d.checks.append((d.append_text(), -1))
        out.append(d.fill(63 - p).next_batch().fill(2))
        assert len(d.batches[0]) == 64
    # ... and at the record behind an early tier exit: three appends take 61 segments
    # to 64, the third does not fit E = 1 and opens the next burst
    for start, behind in ((20, 0), (20, 1), (41, 0)):
        d = bd.Doc(f"advance_behind_tier_exit_at{start}_{behind}", 61 - start // 8, tomb=(2, 5)).fill(start)
        at = [d.append_text() for _ in range(2)]
        if behind == 0:
            d.advance(bd.CUR0)  # on the record that leaves the tier
        at.append(d.append_text())
        d.checks += [(at[0], 1), (at[1], 1), (at[2], 1 - 2 * (behind == 0))]
        if behind:
            d.advance(bd.CUR0)
            d.checks.append((d.annotate(0, SEG, "T_2"), -2))
        d.exit = at
        out.append(d.fill(64 - len(d.recs)).next_batch().fill(2))
        assert len(d.batches[0]) == 64
    # an insert's property-set word and text word after records that leave other values there
    for first in (None, "T_2"):
        for second in ("T_3", None):
            if first is None and second is None:
                continue
            d = bd.Doc(f"stale_words_{first}_{second}", 5)
            for ps in (first, second, first):
                d.add(OP_INSERT, SEG + 1, 3, a=2, b=NO_PROPS if ps is None else bd.PS[ps])
                d.len += 3
                d.marker(2, None if ps is None else "M_1")
                d.annotate(1, d.len - 1, "T_1")
                d.remove(1, 2)
            out.append(d.next_batch().fill(3))
    assert len({d.name for d in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def record_reference():
    cases = record_cases()
    s, batches = bd.build_stream(cases, LAYOUT)
    tables = [se.batch_tables(b) for b in batches]
    tables = [(props, [{k for k in keys if k < 8} for keys in sets]) for props, sets in tables]
    assert se.pass1_layout(tables, s["n_keys"]) == LAYOUT
    trace = se.nsegs_trace(s)
    for i, d in enumerate(cases):
        assert trace[i, 0] == d.n, d.name
        for k, delta in d.checks:
            assert trace[i, k + 1] - trace[i, k] == delta, (d.name, k, trace[i, k:k + 2])
        if hasattr(d, "exit"):  # 63 segments before the third append: it does not fit E = 1
            a = d.exit
            assert trace[i, a[2]] == 63 and tier(int(trace[i, a[1]])) == 1 and a[2] % 64 not in (0, 63), d.name
    o = bd.run(SpecOracle(s["n_keys"], threads=16), s, batches)
    assert (o.statuses() == 0).all()
    return cases, o


@pytest.mark.parametrize("group", [1, 2])
def test_gpu_late_record_words(group):
    cases, o = record_reference()
    pad = 0 if group == 1 else resident_docs() + 1
    if pad:
        o = bd.spec(cases, LAYOUT, pad_to=pad)
    s, batches = bd.build_stream(cases, LAYOUT, pad_to=pad)
    d = bd.run(DeviceEngine(s["n_keys"]), s, batches)
    failed = differing(d, o, range(len(cases)), [c.name for c in cases])
    assert not failed, failed
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())


# ---- soak -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def soak():
    s = gen.generate(3, ops_per_doc=2000, doc_ids=range(64), round_sync=True)
    o = OracleEngine(s["n_keys"], threads=16)
    gen.load_stream(o, s)
    o.apply_batch(s["batch"])
    tiers = np.array([[tier(int(n)) for n in row] for row in se.nsegs_trace(se.first_ops(s, np.full(64, 400)))])
    crossings = (np.diff(tiers, axis=1) != 0).sum(axis=1)
    assert (crossings >= 2).sum() >= 32, crossings  # already in the first 400 ops most documents change tier back and forth
    return s, o


@pytest.mark.parametrize("parts", [1, 4])
def test_gpu_soak_across_the_tier_border(parts):
    s, o = soak()
    d = DeviceEngine(s["n_keys"])
    gen.load_stream(d, s)
    for k in range(parts):
        d.apply_batch(s["batch"] if parts == 1 else gen.split_ops(s, k, parts))
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
