"""Pass 1's record decode, collab window and compiled property sets
(block_run / put_new_v / seg_op_v in mte_step1.h, props_kernel in
mte_engine.hip), case by case against the specification (SpecOracle),
bit-exact: statuses, digests, read-outs (cur_seq and min_seq among them) and
the full segment lists, of stopped documents too.

Every document is one case, written by hand: a body of 1-130 preloaded
four-unit segments, a first batch of 1-300 records and a short second batch that
continues the document, so its window state comes back from the header.  The
cases sit where a burst of 128 records and its two halves of 64 begin and end:
each window error at record 0, 1, 62, 63, 64, 65, 127 and 128, minSeq rising
at 0, 63, 64, 127 and 128, a register tier left upward or downward in the
middle of a burst.  The property cases give marker inserts, text inserts and
annotates (with and without MTE_F_REWRITE) sets of 0, 1, 2, 3 and 5 entries.

Before anything runs on the GPU every case asserts on the CPU that the
restatement reaches its condition: status 0 after the records before the stop
record, the intended status with it, and nothing applied behind it; for the
window and tier cases the restatement's segment counts.

The file runs in three property layouts of pass 1 (tests/stream_edit.py
pass1_layout): "packed" (every value id below 256), "side3" (marker ids of
1000: the flagship's layout) and "unpacked" (a value id of 300 on a text key:
the four-plane K = 4 kernel), each at one document per wave and at two.

A record of an invalid type next to a window violation is not among the cases:
mte_submit refuses every type above MTE_OP_NOOP for a document of the flat
passes (bad_op, mte_engine.hip), so none reaches the kernel.
"""
import functools

import numpy as np
import pytest

import stream_edit as se
from flat_checks import resident_docs
from fluidframework_amd.abi import (DOC_INIT_DTYPE, DOC_NEW_LENGTH_CALC, F_MARKER, F_MSG_END, F_REWRITE,
                                    MTE_E_CLIENT_RANGE, MTE_E_INSERT_FAILED, MTE_E_MSN_GT_SEQ, MTE_E_MSN_ORDER,
                                    MTE_E_SEQ_ORDER, NO_PROPS, NOT_REMOVED, OP_ANNOTATE, OP_DTYPE, OP_INSERT, OP_NOOP,
                                    OP_REMOVE, PROP_DTYPE, PROPSET_DTYPE, SEG_DTYPE)
from fluidframework_amd.engine import DeviceEngine
from oracle import SpecOracle
from test_gpu_flat_variants import assert_same_segments
from test_gpu_step_flags import tier

pytestmark = pytest.mark.gpu

SEG = 4            # units of every preloaded segment
CUR0, MIN0 = 10, 5  # every document's window before the first batch
TEXT_UNITS = 8
LAYOUTS = ("packed", "side3", "unpacked")
EDGES = (0, 1, 62, 63, 64, 65, 127, 128)
C, B, COL, MID = se.KEY_CLIENT, se.KEY_BOLD, se.KEY_COLOR, se.KEY_MARKER_ID


def prop_sets(layout):
    """-> (sets, names): the batch's property sets.  T_*: on text inserts and
    annotates (never the marker id, so "side3" keeps its side key); M_*: on
    marker inserts, the marker id as entry 0, 1, 2, 3 and twice."""
    mid = 1000 if layout == "side3" else 50
    wide = 300 if layout == "unpacked" else 46
    sets = {
        "T_1": [(B, 35)],
        "T_2": [(B, 36), (COL, 45)],
        "T_3": [(C, 1), (B, 37), (COL, wide)],
        "T_5": [(C, 2), (B, 38), (COL, 47), (B, 0), (C, 3)],  # keys repeated, a delete in between
        "T_repeat": [(COL, 41), (COL, 42)],
        "T_delete": [(B, 0), (COL, 0)],
        "T_delete_then_set": [(C, 0), (C, 7), (B, 39), (B, 0)],
        "T_foreign_key": [(9, 77), (B, 40), (11, 5)],  # keys >= n_keys are ignored
        "M_0": [(MID, mid)],
        "M_1": [(B, 33), (MID, mid + 1)],
        "M_2": [(B, 34), (COL, 43), (MID, mid + 2)],
        "M_3": [(C, 4), (B, 35), (COL, 44), (MID, mid + 3), (B, 36)],
        "M_twice": [(MID, mid + 4), (B, 37), (MID, mid + 5)],
        "M_none": [(B, 38), (COL, 48)],
        "M_deleted": [(MID, mid + 6), (COL, 41), (MID, 0)],
        "E_0": [],  # no entries (tests/big_doc_cases.py); last, so the sets above keep their numbers
    }
    names = list(sets)
    return [sets[k] for k in names], {k: i for i, k in enumerate(names)}


_, PS = prop_sets("packed")
TEXT_SETS = [k for k in PS if k.startswith("T_")]
MARKER_SETS = [k for k in PS if k.startswith("M_")]


class Doc:
    """One document's script: records are appended with the running seq, minSeq
    and length kept, so a filler record is always valid.  `status` / `stop`:
    the status the document must end with and the (batch, record) it stops at."""

    def __init__(self, name, n, tomb=()):
        self.name, self.n, self.tomb = name, n, tuple(tomb)
        self.seq, self.msn, self.len = CUR0, MIN0, SEG * (n - len(self.tomb))
        self.batches = [[]]
        self.status, self.stop = 0, None
        self.checks = []  # (record, segment count change of that record) in batch 0

    @property
    def recs(self):
        return self.batches[-1]

    def next_batch(self):
        self.batches.append([])
        return self

    def add(self, typ, p1=0, p2=0, client=0, flags=0, a=0, b=NO_PROPS, end=True, seq=None, msn=None, same=False):
        """One record; seq / msn given: as written, the running values untouched."""
        if seq is None:
            if not same:
                self.seq += 1
            seq = self.seq
        if msn is None:
            msn = self.msn
        self.recs.append((seq, seq - 1, msn, typ, client, flags | (F_MSG_END if end else 0), p1, p2, a, b))
        return len(self.recs) - 1

    def advance(self, to=None):
        """The next record's minSeq: everything so far (or `to`)."""
        self.msn = self.seq if to is None else to
        return self

    def append_text(self, n=1, **kw):
        k = self.add(OP_INSERT, self.len, n, a=0, **kw)
        self.len += n
        return k

    def noop(self, **kw):
        return self.add(OP_NOOP, **kw)

    def remove(self, p1, p2, **kw):
        k = self.add(OP_REMOVE, p1, p2, **kw)
        self.len -= p2 - p1
        return k

    def annotate(self, p1, p2, ps, rewrite=False, **kw):
        return self.add(OP_ANNOTATE, p1, p2, flags=F_REWRITE if rewrite else 0, a=PS[ps], **kw)

    def marker(self, pos, ps, **kw):
        k = self.add(OP_INSERT, pos, 1, flags=F_MARKER, b=NO_PROPS if ps is None else PS[ps], **kw)
        self.len += 1
        return k

    def fill(self, k):
        """k valid records that change no segment count but every eighth (an
        append): annotates of the first segment, NOOPs."""
        for _ in range(k):
            j = len(self.recs) % 8
            if j == 7:
                self.append_text(1 + len(self.recs) % 3)
            elif j in (1, 5):
                self.noop()
            elif j == 2:
                self.annotate(0, SEG, "T_1", rewrite=True)
            else:
                self.annotate(0, SEG, TEXT_SETS[(len(self.recs) // 8) % len(TEXT_SETS)])
        return self

    def fails(self, status):
        self.status, self.stop = status, (len(self.batches) - 1, len(self.recs) - 1)
        return self


def window_error(kind, d):
    """The record that violates the window, appended to d -> the status."""
    if kind == "seq_live":  # a live record at the current seq
        d.append_text(seq=d.seq)
        return MTE_E_SEQ_ORDER
    if kind == "seq_noop_end":  # an END below it
        d.noop(seq=d.seq - 1)
        return MTE_E_SEQ_ORDER
    if kind == "msn_live":  # a live record inside a message, its minSeq below the window's
        d.append_text(end=False, seq=d.seq + 1, msn=d.msn - 1)
        return MTE_E_MSN_ORDER
    if kind == "msn_end":
        d.noop(seq=d.seq + 1, msn=d.msn - 1)
        return MTE_E_MSN_ORDER
    assert kind == "msn_gt_seq"
    d.append_text(seq=d.seq + 1, msn=d.seq + 2)
    return MTE_E_MSN_GT_SEQ


WINDOW_ERRORS = ("seq_live", "seq_noop_end", "msn_live", "msn_end", "msn_gt_seq")


def edge_cases():
    """Batches that end at a block or burst edge, continued by a second batch."""
    out = []
    for k in (1, 63, 64, 65, 127, 128, 129, 200, 300):
        d = Doc(f"edge_len{k}", 3).fill(k).next_batch().advance()
        d.fill(5)
        out.append(d)
    for k in (1, 64, 129):  # a document of one segment
        out.append(Doc(f"edge_one_segment_len{k}", 1).fill(k).next_batch().advance().fill(5))
    d = Doc("edge_one_segment_window_error", 1).fill(64)
    out.append(d.fails(window_error("seq_live", d)).fill(3).next_batch().fill(2))
    for kind in WINDOW_ERRORS:  # the second batch's first record against the header's window
        d = Doc(f"edge_second_batch_{kind}", 3).fill(60).advance().fill(4).next_batch()
        out.append(d.fails(window_error(kind, d)).fill(3))
    return out


def window_cases():
    out = []
    for kind in WINDOW_ERRORS:
        for p in EDGES:
            d = Doc(f"window_{kind}_at{p}", 3).fill(p)
            d.fails(window_error(kind, d)).fill(3)
            out.append(d.next_batch().fill(2))  # a later valid batch: the document stays stopped
    for p in (2, 62, 126):
        # a message of three records, END on the last; then a live record at that seq
        d = Doc(f"window_message_then_same_seq_at{p}", 3).fill(p)
        d.append_text(end=False)
        d.annotate(0, SEG, "T_2", end=False, same=True)
        d.append_text(same=True)
        d.append_text(seq=d.seq)
        out.append(d.fails(MTE_E_SEQ_ORDER).fill(3).next_batch().fill(2))
        # the same message, valid: minSeq of the inner records does not move the window
        d = Doc(f"window_message_at{p}", 3).fill(p)
        d.append_text(end=False)
        d.annotate(0, SEG, "T_2", end=False, same=True)
        d.remove(0, 2, same=True)
        out.append(d.advance().fill(5).next_batch().fill(2))
    return out


def precedence_cases():
    out = []
    for p in (0, 63, 64):
        d = Doc(f"prec_client_and_window_at{p}", 3).fill(p)
        d.append_text(client=40, seq=d.seq)
        out.append(d.fails(MTE_E_CLIENT_RANGE).fill(3).next_batch().fill(2))
        d = Doc(f"prec_insert_failed_and_window_at{p}", 3).fill(p)
        d.add(OP_INSERT, 1 << 20, 2, seq=d.seq)
        out.append(d.fails(MTE_E_INSERT_FAILED).fill(3).next_batch().fill(2))
    for first, gap in ((3, 7), (60, 4), (63, 1), (64, 63)):
        d = Doc(f"prec_window_at{first}_then_client", 3).fill(first)
        d.append_text(seq=d.seq)
        d.fails(MTE_E_SEQ_ORDER).fill(gap)
        d.append_text(client=40)
        out.append(d.fill(2).next_batch().fill(2))
        d = Doc(f"prec_client_at{first}_then_window", 3).fill(first)
        d.append_text(client=40)
        d.fails(MTE_E_CLIENT_RANGE).fill(gap)
        d.append_text(seq=d.seq)
        out.append(d.fill(2).next_batch().fill(2))
    return out


def advance_cases():
    """minSeq rising: tombstones at or below it leave (the zamboni)."""
    out = []
    for p in (0, 63, 64, 127, 128):
        for how in ("live", "noop_end"):
            # two preloaded tombstones (removed at seq 8 > MIN0) leave at record p
            d = Doc(f"advance_{how}_at{p}", 8, tomb=(2, 5)).fill(p)
            d.advance(CUR0)
            k = d.noop() if how == "noop_end" else d.append_text()
            d.checks.append((k, -2 if how == "noop_end" else -1))
            out.append(d.fill(4).next_batch().fill(2))
    # an END with the window's own minSeq is no advance: removed at seq 8, minSeq stays MIN0 ...
    d = Doc("advance_equal_min_seq", 8, tomb=(2, 5)).fill(70)
    d.checks += [(k, 0) for k in range(0, 70, 8)]
    out.append(d.next_batch().advance().fill(2))
    # ... and minSeq rises to 7, still below the removal
    d = Doc("advance_below_removal", 8, tomb=(2, 5)).fill(3).advance(7)
    d.checks.append((d.noop(), 0))
    out.append(d.fill(70).next_batch().fill(2))
    # on every record of two blocks: append, remove it again, minSeq always at the previous record
    d = Doc("advance_every_record", 4)
    for _ in range(70):
        d.advance()
        d.append_text(2)
        d.advance()
        d.remove(d.len - 2, d.len)
    d.checks += [(0, 1), (1, 0), (2, 0), (3, 0), (64, 0), (127, 0), (128, 0)]
    out.append(d.next_batch().advance().fill(3))
    return out


def tier_cases():
    out = []
    for n, start in ((61, 20), (61, 56), (125, 20), (125, 58), (125, 100)):
        # three appends in a row cross the tier's last segment count; splits and annotates follow
        # (the filler appends once in eight records: n segments when the three appends begin)
        d = Doc(f"tier_up_n{n}_at{start}", n - start // 8).fill(start)
        at = [d.append_text() for _ in range(3)]
        d.checks += [(k, 1) for k in at]
        d.checks.append((d.add(OP_INSERT, 2, 2), 2))
        d.len += 2
        d.annotate(1, d.len - 1, "T_3")
        d.checks.append((d.remove(SEG * 3 + 1, SEG * 5 - 1), 2))
        d.up = (n, at)
        out.append(d.fill(30).next_batch().fill(2))
    for n, block, start in ((130, 110, 4), (130, 110, 57), (130, 60, 63), (100, 80, 5), (100, 80, 62)):
        # a block of tombstones leaves in the middle of a burst: a lower tier for the records behind
        d = Doc(f"tier_down_n{n}_block{block}_at{start}", n).fill(start)
        d.remove(SEG * 3, SEG * (3 + block))
        d.fill(3).advance()
        k = d.append_text()
        d.checks.append((k, 1 - block))
        d.down = (n, k)
        d.checks.append((d.add(OP_INSERT, 2, 2), 2))
        d.len += 2
        d.annotate(1, d.len - 1, "T_2", rewrite=True)
        out.append(d.fill(30).next_batch().fill(2))
    return out


def property_cases():
    out = []
    for i, t in enumerate(TEXT_SETS + [None]):
        for m in MARKER_SETS + [None]:
            d = Doc(f"props_{t}_{m}", 5)
            d.marker(2, m)  # splits the first segment
            d.add(OP_INSERT, SEG + 3, 3, a=1, b=NO_PROPS if t is None else PS[t])
            d.len += 3
            d.marker(d.len, MARKER_SETS[(i + 3) % len(MARKER_SETS)])
            ann = t or "T_2"
            d.annotate(0, d.len, ann)  # over both markers
            d.annotate(3, d.len - 2, TEXT_SETS[(i + 1) % len(TEXT_SETS)])
            d.annotate(1, SEG * 2, "T_delete")
            d.annotate(0, d.len - 1, ann, rewrite=True)  # the first marker loses its side value, the last keeps it
            d.marker(1, m)
            d.annotate(SEG, d.len, TEXT_SETS[(i + 2) % len(TEXT_SETS)], rewrite=True)
            d.add(OP_INSERT, 0, 2, a=3, b=NO_PROPS if t is None else PS[t])
            d.len += 2
            out.append(d.next_batch().fill(9))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = edge_cases() + window_cases() + precedence_cases() + advance_cases() + tier_cases() + property_cases()
    assert len({d.name for d in out}) == len(out)
    for d in out:
        assert 1 <= d.n <= 130 and all(len(b) <= 300 for b in d.batches) and len(d.batches) == 2, d.name
    return out


GROUPS = ("edge", "window", "prec", "advance", "tier", "props")


def build_stream(cases, layout, pad_to=0, cut=None, n_keys=se.N_KEYS):
    """-> (stream, batches): the cases as documents 0 .. len(cases) - 1, then
    trivial documents up to pad_to.  cut(d) -> (batch, records): document d's
    records up to there only.  A case may carry its own document flags
    (`flags`) and more or fewer than two batches (tests/big_doc_cases.py)."""
    ns = [d.n for d in cases] + [1] * max(0, pad_to - len(cases))
    nd = len(ns)
    units = SEG * np.array(ns, np.int64)
    text_off = np.concatenate([[0], np.cumsum(units)])
    inits = np.zeros(nd, DOC_INIT_DTYPE)
    inits["text_off"], inits["text_len"] = text_off[:-1], units
    inits["flags"], inits["propset"] = DOC_NEW_LENGTH_CALC, NO_PROPS
    inits["flags"][:len(cases)] = [getattr(d, "flags", DOC_NEW_LENGTH_CALC) for d in cases]
    inits["min_seq"], inits["cur_seq"] = MIN0, CUR0
    init_text = (65 + np.arange(int(text_off[-1])) % 26).astype(np.uint16)
    seg_offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.uint64)
    segs = np.zeros(int(seg_offs[-1]), SEG_DTYPE)
    segs["text_off"] = SEG * np.arange(len(segs))
    segs["len"], segs["removed_seq"], segs["client"], segs["propset"] = SEG, NOT_REMOVED, -1, NO_PROPS
    for i, d in enumerate(cases):
        for t in d.tomb:  # removed by client 1 at seq 8, inside the window
            g = int(seg_offs[i]) + t
            segs["removed_seq"][g], segs["removers"][g], segs["seq"][g], segs["client"][g] = 8, 2, 0, -1
    sets, _ = prop_sets(layout)
    ps = np.zeros(len(sets), PROPSET_DTYPE)
    ps["count"] = [len(x) for x in sets]
    ps["first"] = np.concatenate([[0], np.cumsum(ps["count"])[:-1]])
    pe = np.array([e for x in sets for e in x], PROP_DTYPE)
    text = (97 + np.arange(TEXT_UNITS) % 26).astype(np.uint16)
    batches = []
    for bi in range(max(len(d.batches) for d in cases)):
        recs = []
        for i, d in enumerate(cases):
            r = d.batches[bi] if bi < len(d.batches) else []
            if cut is not None:
                cb, ck = cut(d)
                r = r if bi < cb else (r[:ck] if bi == cb else [])
            recs.append(r)
        filler = Doc("pad", 1)
        filler.seq += 100 * bi
        recs += [[filler.recs[filler.append_text()]]] * (nd - len(cases))
        flat = [x for r in recs for x in r]
        ops = np.array(flat, OP_DTYPE) if flat else np.zeros(0, OP_DTYPE)
        offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
        batches.append({"op_offsets": offs, "ops": ops, "text": text, "propsets": ps, "props": pe})
    stream = {"inits": inits, "init_text": init_text, "n_keys": n_keys, "segs": (seg_offs, segs), "batch": batches[0]}
    return stream, batches


def run(engine, stream, batches):
    engine.load_docs(stream["inits"], stream["init_text"])
    engine.load_segments(*stream["segs"])
    for b in batches:
        engine.apply_batch(b)
    return engine


def spec(cases, layout, cut=None, pad_to=0):
    s, batches = build_stream(cases, layout, pad_to=pad_to, cut=cut)
    return run(SpecOracle(s["n_keys"], threads=16), s, batches)


@functools.lru_cache(maxsize=None)
def reference(layout):
    """-> (cases, the specification after both batches); every case has reached
    its condition, or this fails."""
    cases = all_cases()
    s, batches = build_stream(cases, layout)
    tables = [se.batch_tables(b) for b in batches]
    tables = [(props, [{k for k in keys if k < 8} for keys in sets]) for props, sets in tables]  # keys the engine tracks
    assert se.pass1_layout(tables, s["n_keys"]) == layout
    want = np.array([d.status for d in cases])
    stops = [i for i, d in enumerate(cases) if d.stop]
    assert len(stops) >= 60 and all(cases[i].status < 0 for i in stops)
    whole = lambda d: (len(d.batches), 0)
    # status 0 before the stop record, the intended status with it ...
    before = spec(cases, layout, cut=lambda d: d.stop or whole(d))
    assert (before.statuses() == 0).all(), [d.name for d, st in zip(cases, before.statuses()) if st]
    at = spec(cases, layout, cut=lambda d: (d.stop[0], d.stop[1] + 1) if d.stop else whole(d))
    bad = [(d.name, int(st)) for d, st in zip(cases, at.statuses()) if st != d.status]
    assert not bad, bad
    # ... and the records behind it, the later batch included, change nothing
    o = run(SpecOracle(s["n_keys"], threads=16), s, batches)
    np.testing.assert_array_equal(o.statuses(), want)
    np.testing.assert_array_equal(o.digest(), at.digest())
    for i in stops:
        assert o.read_doc(i) == at.read_doc(i), cases[i].name
        assert at.read_doc(i) != before.read_doc(i) or cases[i].status in (MTE_E_CLIENT_RANGE, MTE_E_INSERT_FAILED)
    # the segment counts around the window advances and tier changes
    trace = se.nsegs_trace(s)
    for i, d in enumerate(cases):
        assert trace[i, 0] == d.n, d.name
        for k, delta in d.checks:
            assert trace[i, k + 1] - trace[i, k] == delta, (d.name, k, trace[i, k:k + 2])
        if hasattr(d, "up"):
            n, at = d.up  # n -> n + 3 segments inside one block of 64 records
            assert trace[i, at[0]] == n and tier(n) < tier(int(trace[i, at[-1] + 1])), d.name
            assert at[0] // 64 == (at[-1] + 1) // 64 and at[0] % 64 != 0, d.name
        if hasattr(d, "down"):
            n, k = d.down
            assert tier(int(trace[i, k])) > tier(int(trace[i, k + 1])) and k % 64 not in (0, 63), d.name
    return cases, o


@functools.lru_cache(maxsize=None)
def replayed(layout, group):
    """-> (the device engine after both batches, the specification for the same stream)."""
    cases, o = reference(layout)
    if group == 1:
        assert len(cases) <= resident_docs()
        s, batches = build_stream(cases, layout)
        return run(DeviceEngine(s["n_keys"]), s, batches), o
    n = resident_docs() + 1  # more flat documents than pass 1 holds one per wave: two per wave
    assert min(8, (n + resident_docs() - 1) // resident_docs()) == 2
    op = spec(cases, layout, pad_to=n)
    np.testing.assert_array_equal(op.digest()[:len(cases)], o.digest())
    s, batches = build_stream(cases, layout, pad_to=n)
    return run(DeviceEngine(s["n_keys"]), s, batches), op


def test_cases_cover_the_edges():
    cases = all_cases()
    names = {d.name for d in cases}
    for kind in WINDOW_ERRORS:
        for p in EDGES:
            assert f"window_{kind}_at{p}" in names
            d = next(d for d in cases if d.name == f"window_{kind}_at{p}")
            assert d.stop == (0, p)
    assert {len(d.batches[0]) for d in cases if d.name.startswith("edge_len")} >= {1, 63, 64, 65, 127, 128, 129, 200}
    assert sum(d.name.startswith("props_") for d in cases) == (len(TEXT_SETS) + 1) * (len(MARKER_SETS) + 1)
    assert {len(s) for s in prop_sets("packed")[0]} >= {1, 2, 3, 5}


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("which", GROUPS)
def test_gpu_block_decode(which, layout, group):
    cases, _ = reference(layout)
    d, o = replayed(layout, group)
    docs = [i for i, c in enumerate(cases) if c.name.startswith(which + "_")]
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
    assert not failed, f"{len(failed)} of {len(docs)} cases differ: {failed}"


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_block_decode_all_documents(layout, group):
    d, o = replayed(layout, group)
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    np.testing.assert_array_equal(d.digest(), o.digest())
