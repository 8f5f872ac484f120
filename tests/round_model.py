"""Which path the round phases (csrc/mte_round.h) took, read from
`mte_stats.round_bytes`.

`round_bytes` (RoundArgs::acct, summed by mte_stats_get) is counted with
statistics off too, is zeroed at the start of every launch
(round_phase_loop, mte_engine.hip) and every term of it is added for a
document whose plan is kModeRound.  For a context of ONE document and ONE
batch it is therefore a sum of these terms, restated from the header's own
accounting (pb = 4 * (kFieldPlanes + K) bytes of one segment's planes):

  re-layout   32 len + 4 n_old + (2 pb + 8) kept + 8 nch     mte_round.h:259-264 (rnd_scan_kernel, scatter)
  chain       32 nc + 72 m          (m <= 2 nc + 8)           mte_round.h:986-988 (rnd_resolve_kernel)
  chunk       40 nb + pb (n_before + n_after) + 8             mte_round.h:1141-1142 (rnd_apply_one)
  applied     4 nch                                           mte_round.h:266-268 (rnd_scan_kernel, gather)
  leaves      2 pb nseg + 8 nch                               mte_round.h:448-449 (rnd_gscan_kernel)

so it is 0 exactly when no run of the batch was planned as a round, and the
terms a path adds or leaves out separate the paths whenever the document is
large against the run (the `leaves` term, 2 pb nseg, against the <= 176 len a
run's chains can add).  The model gives closed intervals, not counts: where the
caller knows the layout (one-unit segments, `Layout`) they are points.

A document leaves the arena at the end of every launch (round_phase_loop's
final gather), so a layout is carried only between the runs of one batch: a
run submitted as a batch of its own is always taken from a fresh re-layout.

A carried run whose hot chunk overflows its bucket (rflag 1) and also has no
room (rflag 4) is gathered, re-laid out and refused a second time before it goes
op after op (rnd_post_kernel idles its plan on rflag 4 whatever else is set):
REFUSED_TWICE.  The state is the restatement's either way.

Limits: single-document contexts (round_bytes is summed over the documents)
and statistics off (statistics runs never take the round phases).
"""
import numpy as np

# mte_passes.h
K_ROUND_MIN = 256    # kRoundMin: the shortest run taken
K_RB = 62            # kRB: sub-ops per chunk and run
K_LIVE_FULL = 192    # kLiveFull: a carried chunk past it is re-laid out
K_CH_SLOTS = 256     # kChSlots: rnd_room refuses count + 2 sub-ops > kChSlots
K_MAX_PHASES = 16    # kMaxPhases: the last phase plans no round (rd.last)
K_FILL = 128         # MTE_RND_FILL / kChFill
K_FIELD_PLANES = 6   # kFieldPlanes (mte_kernels.h)
MAX_CLIENTS = 32
OP_INSERT, OP_REMOVE, OP_ANNOTATE = 0, 1, 2
F_MARKER, F_MSG_END, F_REWRITE = 1, 2, 4

# the hypotheses about one run
NOT_PLANNED = "not planned"
REFUSED = "planned, refused before the apply"
TAKEN_FRESH = "taken from a fresh re-layout"
TAKEN_CARRIED = "taken carried"
CARRIED_NO_ROOM = "carried, no room, re-laid out and taken"
CARRIED_FULL = "carried, a chunk past kLiveFull, re-laid out and taken"
REFUSED_TWICE = "carried, no room, re-laid out and refused again"


def plane_bytes(n_keys=0):
    """pb: the engine instantiates K = 0 / 4 / 8 property planes."""
    k = 0 if n_keys == 0 else (4 if n_keys <= 4 else 8)
    return 4 * (K_FIELD_PLANES + k)


def nch_cap(cap):
    return cap // K_FILL + 2  # mte_engine.hip: nch_cap = cap / kChFill + 2


def fresh_nch(kept, cap):
    """rnd_scan_kernel: chunks of a re-layout of `kept` segments."""
    return max(1, min(nch_cap(cap), -(-kept // K_FILL)))


class Iv:
    """A closed interval of byte counts."""

    def __init__(self, lo, hi=None):
        if isinstance(lo, Iv):
            lo, hi = lo.lo, lo.hi
        elif isinstance(lo, (tuple, list)):
            lo, hi = lo
        self.lo, self.hi = int(lo), int(lo if hi is None else hi)
        assert self.lo <= self.hi

    def __add__(self, o):
        o = Iv(o)
        return Iv(self.lo + o.lo, self.hi + o.hi)

    __radd__ = __add__

    def __mul__(self, k):
        assert k >= 0
        return Iv(self.lo * k, self.hi * k)

    __rmul__ = __mul__

    def __contains__(self, x):
        return self.lo <= x <= self.hi

    def disjoint(self, o):
        return self.hi < o.lo or o.hi < self.lo

    def __repr__(self):
        return f"[{self.lo}, {self.hi}]"


# ---- the plan: where a run ends (rnd_plan_kernel's `ok`, mte_round.h:136-138) ----

def run_length(ops, k0, cur_seq, min_seq):
    """The ops from k0 that rnd_plan takes as one candidate run of a new-calc
    document whose header holds (cur_seq, min_seq) at k0."""
    R, M = int(cur_seq), int(ops["min_seq"][k0])
    allowed = F_MSG_END | F_MARKER | F_REWRITE
    below = R
    n = 0
    for k in range(k0, len(ops)):
        o = ops[k]
        fl = int(o["flags"])
        ok = (int(o["ref_seq"]) == R and int(o["min_seq"]) == M and int(o["type"]) <= OP_ANNOTATE and
              int(o["client"]) < MAX_CLIENTS and (fl & F_MSG_END) and not (fl & ~allowed) and int(o["seq"]) > below and
              M >= int(min_seq) and M <= R and int(o["pos1"]) >= 0 and int(o["pos2"]) >= 0)
        if not ok:
            break
        below = int(o["seq"])
        n += 1
    return n


def plan(ops, k0, cur_seq, min_seq, nseg, cap):
    """-> (mode, k1): "round" / "seq" (this stretch op after op) as rnd_plan
    decides (mte_round.h:150-163) in any phase but the launch's 16th."""
    n = run_length(ops, k0, cur_seq, min_seq)
    room = nseg + 3 * n + 2 <= cap
    if n >= K_ROUND_MIN and room:
        return "round", k0 + n
    if n >= K_ROUND_MIN:
        return "seq", k0 + n
    return "seq", len(ops)


# ---- a chunk layout of one-unit segments and the resolve on it -----------------

class Facts:
    """What a run's resolve does on one layout: per chunk the sub-ops (nb),
    segments added (ins), units added and removed."""

    def __init__(self, layout, nb, ins, units_in, units_out, failed, dead):
        self.layout, self.nb, self.ins, self.units_in, self.units_out = layout, nb, ins, units_in, units_out
        self.failed = failed    # index of the op that inserts past the end (rflag 2), or None
        self.dead = dead        # [(chunk, seq, units)] tombstones the run makes
        self.subops = int(nb.sum())
        self.touched = int((nb > 0).sum())
        t = nb > 0
        self.apply_segs = int((2 * layout.cnt[t] + ins[t]).sum())
        self.over = bool((nb > K_RB).any())                                   # rflag 1 (rnd_emit)
        self.no_room = bool((layout.cnt + 2 * nb > K_CH_SLOTS).any())        # rflag 4 (rnd_room_kernel, carried only)


class Layout:
    """Per chunk the segment count and the visible length (the round-start
    column entry), for documents of one-unit segments: an insert of one unit adds
    one segment to its chunk and a remove adds none.  Tombstones are kept per
    chunk as (seq, units)."""

    def __init__(self, cnt, vis, dead=None):
        self.cnt = np.asarray(cnt, np.int64).copy()
        self.vis = np.asarray(vis, np.int64).copy()
        self.dead = list(dead or [])
        self.nch = len(self.cnt)

    @classmethod
    def fresh(cls, kept, cap, alive=None):
        """rnd_move / rnd_cols: `kept` segments at fill = ceil(kept / nch) per
        chunk; alive: per kept segment (document order) whether it is visible."""
        nch = fresh_nch(kept, cap)
        fill = -(-kept // nch) if nch else 1
        cnt = np.clip(kept - np.arange(nch) * fill, 0, fill)
        if alive is None:
            vis = cnt.copy()
        else:
            alive = np.asarray(alive, np.int64)
            assert len(alive) == kept
            vis = np.array([alive[q * fill:(q + 1) * fill].sum() for q in range(nch)], np.int64)
        return cls(cnt, vis)

    @property
    def nseg(self):
        return int(self.cnt.sum())

    def full(self):
        return bool((self.cnt > K_LIVE_FULL).any())  # rnd_live_kernel / rnd_plan_kernel

    def resolve(self, ops):
        """rnd_serial_op (mte_round.h:579-633; rnd_block gives the same
        sub-ops) per client on its own copy of the column."""
        nch = self.nch
        nb = np.zeros(nch, np.int64)
        ins = np.zeros(nch, np.int64)
        uin = np.zeros(nch, np.int64)
        uout = np.zeros(nch, np.int64)
        cols, dead, failed = {}, [], None
        stopped = set()
        for k, o in enumerate(ops):
            c = int(o["client"])
            if c in stopped:
                continue
            col = cols.setdefault(c, self.vis.copy())
            incl = np.cumsum(col)
            total = int(incl[-1]) if nch else 0
            p1, p2, typ = int(o["pos1"]), int(o["pos2"]), int(o["type"])
            if typ == OP_INSERT:
                i = int(np.searchsorted(incl, p1, "left"))  # the first chunk with prefix >= pos
                if p1 > total or i >= nch:
                    failed = k if failed is None else failed
                    stopped.add(c)  # the chain stops at its failed op
                    continue
                n = 1 if int(o["flags"]) & F_MARKER else p2
                nb[i] += 1
                ins[i] += 1
                uin[i] += max(n, 0)
                col[i] += max(n, 0)
                continue
            b1, b2 = min(p1, p2), max(p1, p2)
            i = int(np.searchsorted(incl, b1, "right"))     # the first chunk with prefix > b1
            if i >= nch:
                continue
            if b1 == b2:
                if int(incl[i] - col[i]) < b1:
                    nb[i] += 1
                continue
            while i < nch:
                st, en = int(incl[i] - col[i]), int(incl[i])
                if st >= b2:
                    break
                if col[i] > 0:
                    nb[i] += 1
                    if typ == OP_REMOVE:
                        ov = min(b2, en) - max(b1, st)
                        col[i] -= ov
                        uout[i] += ov
                        dead.append((i, int(o["seq"]), ov))
                i += 1
        return Facts(self, nb, ins, uin, uout, failed, dead)

    def after(self, facts):
        """The layout once the run is applied (no two clients of the run may
        remove the same unit: the caller's inputs guarantee it and the twins
        check the totals against the restatement)."""
        return Layout(self.cnt + facts.ins, self.vis + facts.units_in - facts.units_out,
                      self.dead + facts.dead)


# ---- the terms --------------------------------------------------------------------

def t_relayout(length, n_old, kept, nch, pb):
    return Iv(32 * length + 4 * n_old + (2 * pb + 8) * kept + 8 * nch)


def t_chains(length, subops):
    return 32 * length + 72 * Iv(subops)


def t_apply(subops, segs, touched, pb):
    return 40 * Iv(subops) + pb * Iv(segs) + 8 * Iv(touched)


def t_applied(nch):
    return Iv(4 * nch)


def t_leaves(nseg, nch, pb):
    return 2 * pb * Iv(nseg) + 8 * nch


def loose_facts(length, clients, kept, n_after, nch):
    """Bounds for a run on a layout the caller does not know chunk by chunk:
    (subops, apply_segs, touched) as intervals.  m <= 2 nc + 8 per chain; the
    touched chunks' segments before lie in [0, kept], their growth is the
    document's."""
    s_hi = sum(2 * nc + 8 for nc in clients.values())
    grow = max(n_after - kept, 0)
    return Iv(0, s_hi), Iv(grow, 2 * kept + grow), Iv(0, min(nch, s_hi))


def run_interval(hyp, length, pb, *, n_old=None, kept=None, nch=None, facts=None, first=None,
                 old_nseg=None, old_nch=None, carried=False, complete=True):
    """The bytes one run adds under `hyp`, without the final `leaves` term.

    facts: (subops, apply_segs, touched) on the layout the run is applied on
    (each an int or an interval); first: the same on the carried layout for the
    refused first attempt of CARRIED_NO_ROOM; n_old / kept / nch: the re-layout's
    flat segments before, kept, and chunks; old_nseg / old_nch: the carried
    layout that leaves (CARRIED_*, or REFUSED with carried=True).  REFUSED_TWICE
    is a sum of these (Doc.run) and has no branch here.  complete:
    no chain of a REFUSED run failed (a bucket overflow, rflag 1: m counts on
    past kRB, so the chains' 72 m is there in full)."""
    if hyp == NOT_PLANNED:
        return Iv(0)
    s, segs, touched = facts
    if hyp == REFUSED:
        # every chain's records and sub-ops; a failed chain (rflag 2) stops early
        out = t_chains(length, s if complete else Iv(0, Iv(s).hi))
        if carried:
            return out + t_leaves(old_nseg, old_nch, pb)  # rnd_post_kernel: gathered first
        return out + t_relayout(length, n_old, kept, nch, pb)
    body = t_chains(length, s) + t_apply(s, segs, touched, pb) + t_applied(nch)
    if hyp == TAKEN_CARRIED:
        return body
    body = body + t_relayout(length, n_old, kept, nch, pb)
    if hyp == TAKEN_FRESH:
        return body
    body = body + t_leaves(old_nseg, old_nch, pb)
    if hyp == CARRIED_FULL:
        return body
    if hyp == CARRIED_NO_ROOM:
        return body + t_chains(length, first[0])
    raise ValueError(hyp)


class Doc:
    """One document of one-unit segments through a batch under a hypothesised
    path: the bytes of each run and the layout it leaves.  `n` is the flat
    planes' segment count; rseq (optional, document order) the loaded
    segments' removedSeq, 0 for a visible one."""

    def __init__(self, n, cap, n_keys=0, rseq=None):
        self.n, self.cap, self.pb = int(n), int(cap), plane_bytes(n_keys)
        self.rseq = None if rseq is None else np.asarray(rseq, np.int64)  # exact until the first run
        self.tomb = []       # (seq, units) of tombstones whose place in the flat planes is not modelled
        self.layout = None   # set while the arena holds the document
        self.total = Iv(0)

    def _fresh(self, M):
        """Re-layout of the flat planes with zamboni at M -> (layout, n_old, kept)."""
        n_old = self.n
        if self.rseq is not None:
            keep = (self.rseq == 0) | (self.rseq > M)
            return Layout.fresh(int(keep.sum()), self.cap, alive=(self.rseq[keep] == 0)), n_old, int(keep.sum())
        assert all(s <= M for s, _ in self.tomb), "a tombstone above M at a place the model does not know"
        kept = n_old - sum(u for _, u in self.tomb)
        return Layout.fresh(kept, self.cap), n_old, kept

    def _leave(self):
        lay = self.layout
        self.n, self.layout, self.rseq = lay.nseg, None, None
        self.tomb = [(s, u) for _, s, u in lay.dead]
        return t_leaves(lay.nseg, lay.nch, self.pb)

    def run(self, ops, hyp):
        """One run under `hyp` -> its interval; the document moves on."""
        ops = np.asarray(ops)
        length, M = len(ops), int(ops["min_seq"][0])
        pb = self.pb
        if hyp in (NOT_PLANNED, REFUSED, REFUSED_TWICE):
            out = Iv(0)
            if hyp == REFUSED_TWICE:
                # rflag 4 beside rflag 1: rnd_post_kernel gathers the document and idles
                # its plan, the next phase re-lays it out and the resolve refuses it again
                old = self.layout
                first = old.resolve(ops)
                self._leave()
                lay, n_old, kept = self._fresh(M)
                f = lay.resolve(ops)
                out = (t_chains(length, first.subops) + t_leaves(old.nseg, old.nch, pb) +
                       run_interval(REFUSED, length, pb, facts=(f.subops, 0, 0), n_old=n_old, kept=kept, nch=lay.nch,
                                    complete=f.failed is None))
            elif hyp == REFUSED and self.layout is not None:
                f = self.layout.resolve(ops)
                out = run_interval(REFUSED, length, pb, facts=(f.subops, 0, 0), carried=True,
                                   old_nseg=self.layout.nseg, old_nch=self.layout.nch, complete=f.failed is None)
                self._leave()  # rnd_post_kernel: gathered first
            elif hyp == REFUSED:
                lay, n_old, kept = self._fresh(M)
                f = lay.resolve(ops)
                out = run_interval(REFUSED, length, pb, facts=(f.subops, 0, 0), n_old=n_old, kept=kept, nch=lay.nch,
                                   complete=f.failed is None)
            elif self.layout is not None:
                out = self._leave()  # rnd_live_kernel: the next run is not a round
            # op after op on the flat planes: one segment per insert; the
            # tombstones it makes and drops are not modelled (no re-layout may follow)
            self.n += int((ops["type"] == OP_INSERT).sum())
            self.rseq = None
            if (ops["type"] == OP_REMOVE).any() or self.tomb:
                self.tomb = self.tomb + [(2 ** 31, 0)]
            self.total = self.total + out
            return out
        if hyp == TAKEN_FRESH:
            assert self.layout is None
            lay, n_old, kept = self._fresh(M)
            f = lay.resolve(ops)
            out = run_interval(hyp, length, pb, n_old=n_old, kept=kept, nch=lay.nch,
                               facts=(f.subops, f.apply_segs, f.touched))
        elif hyp == TAKEN_CARRIED:
            lay = self.layout
            f = lay.resolve(ops)
            out = run_interval(hyp, length, pb, nch=lay.nch, facts=(f.subops, f.apply_segs, f.touched))
        else:
            old = self.layout
            first = old.resolve(ops)
            self._leave()
            lay, n_old, kept = self._fresh(M)
            f = lay.resolve(ops)
            out = run_interval(hyp, length, pb, n_old=n_old, kept=kept, nch=lay.nch,
                               facts=(f.subops, f.apply_segs, f.touched), first=(first.subops, 0, 0),
                               old_nseg=old.nseg, old_nch=old.nch)
        self.layout = lay.after(f)
        self.rseq = None
        self.facts = f
        self.total = self.total + out
        return out

    def end(self):
        """The launch ends: a carried document leaves the arena."""
        if self.layout is not None:
            self.total = self.total + self._leave()
        return self.total


def assert_path(measured, expected, rivals):
    """measured lies in `expected`, and `expected` is disjoint from every rival
    (a property of the inputs, which the CPU twins assert with measured=None)."""
    expected = Iv(expected)
    for name, r in (rivals.items() if isinstance(rivals, dict) else enumerate(rivals)):
        assert expected.disjoint(Iv(r)), f"rival {name} {Iv(r)} overlaps the expected {expected}"
    if measured is not None:
        assert float(measured) == int(measured) and int(measured) in expected, \
            f"round_bytes {measured} outside {expected}; rivals {rivals}"
