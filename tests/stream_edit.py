"""Edits of a generated op stream (the dict gen.generate returns), in numpy.

The generator's streams reach only some of the engine's data-selected variants:
its annotate values are <= 48, its sets carry 1-2 keys, it never sets
MTE_F_REWRITE and only marker inserts set markerId.  Each edit here changes
value ids, property sets or flags only, never a position, a length or a
sequence number, so the edited stream is as valid for the specification (which
has no layouts) as the generated one.  Every function returns a new stream and
leaves its argument untouched.
"""
import numpy as np

from fluidframework_amd.abi import (F_LOCAL, F_MARKER, F_REWRITE, NO_PROPS, OP_ANNOTATE, OP_INSERT, PROP_DTYPE,
                                    PROPSET_DTYPE)

N_KEYS = 4
KEY_CLIENT, KEY_BOLD, KEY_COLOR, KEY_MARKER_ID = 0, 1, 2, 3
# value ids a widened set gives an added key: the generator's own ids of keys
# 0-2 (mte_gen.cpp fixed_propsets), eight small ids for key 3, and null
_FILL = {KEY_CLIENT: list(range(1, 9)) + [0], KEY_BOLD: list(range(33, 41)) + [0],
         KEY_COLOR: list(range(41, 49)) + [0], KEY_MARKER_ID: list(range(49, 57)) + [0]}


def _with_batch(stream, **kw):
    out = dict(stream)
    out["batch"] = dict(stream["batch"], **kw)
    return out


def annotate_records(ops):
    """Indices of the sequenced annotate records."""
    return np.flatnonzero((ops["type"] == OP_ANNOTATE) & ((ops["flags"] & F_LOCAL) == 0))


def marker_records(ops):
    """Indices of the marker inserts that carry a property set."""
    return np.flatnonzero((ops["type"] == OP_INSERT) & ((ops["flags"] & F_MARKER) != 0) & (ops["b"] != NO_PROPS))


def _entries(batch, psi):
    ps = batch["propsets"][psi]
    pe = batch["props"][int(ps["first"]):int(ps["first"]) + int(ps["count"])]
    return [(int(k), int(v)) for k, v in zip(pe["key"], pe["value"])]


def _append_sets(batch, sets):
    """The batch's property tables with `sets` (lists of (key, value)) appended
    -> (propsets, props, index of the first new set)."""
    ps, pe = batch["propsets"], batch["props"]
    cnt = np.array([len(s) for s in sets], np.uint32)
    nps = np.zeros(len(sets), PROPSET_DTYPE)
    nps["count"] = cnt
    nps["first"] = len(pe) + np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32) if len(sets) else 0
    flat = [e for s in sets for e in s]
    npe = np.array(flat, PROP_DTYPE) if flat else np.zeros(0, PROP_DTYPE)
    return np.concatenate([ps, nps]), np.concatenate([pe, npe]), len(ps)


def _extended(entries, keys, want, salt, front=False):
    """`entries` with keys of `keys` it lacks added up to `want` entries."""
    have = {k for k, _ in entries}
    extra = [(k, _FILL[k][(salt * 7 + 3 * k + want) % 9]) for k in keys if k not in have][: max(0, want - len(entries))]
    return extra + entries if front else entries + extra


def remap_values(stream, key, fn):
    """Value ids of `key` in the batch's property table through `fn` (an array
    function); 0 (null) stays 0."""
    pe = stream["batch"]["props"].copy()
    m = (pe["key"] == key) & (pe["value"] != 0)
    new = np.asarray(fn(pe["value"][m].astype(np.int64)))
    assert (new > 0).all()
    pe["value"][m] = new.astype(np.uint32)
    return _with_batch(stream, props=pe)


def widen_propsets(stream, every, keys=(KEY_CLIENT, KEY_BOLD, KEY_COLOR), marker_sets=False):
    """Every `every`-th sequenced annotate gets its set widened with the keys of
    `keys` it lacks, to 3 entries and (with 4 keys) to 4 in turn; the added
    entries follow the set's own, nulls among them.  marker_sets: every marker
    insert's set gets keys 1-2 or 0-2 in front of its own, so its markerId is
    the third or fourth entry."""
    b = stream["batch"]
    ops = b["ops"].copy()
    ann = annotate_records(ops)[::every]
    wants = (3, 4) if len(keys) >= 4 else (3,)
    olds = np.unique(ops["a"][ann])
    sets, table = [], np.zeros((len(wants), int(olds.max()) + 1 if len(olds) else 1), np.int64)
    for w, want in enumerate(wants):
        for old in olds.tolist():
            table[w, old] = len(sets)
            sets.append(_extended(_entries(b, old), keys, want, old))
    mk = marker_records(ops) if marker_sets else np.zeros(0, np.int64)
    mk_base = len(sets)
    for i, r in enumerate(mk.tolist()):
        front = (KEY_BOLD, KEY_COLOR) if i % 2 == 0 else (KEY_CLIENT, KEY_BOLD, KEY_COLOR)
        own = _entries(b, int(ops["b"][r]))
        sets.append(_extended(own, front, len(own) + len(front), i, front=True))
    ps, pe, base = _append_sets(b, sets)
    ops["a"][ann] = base + table[np.arange(len(ann)) % len(wants), ops["a"][ann]]
    ops["b"][mk] = base + mk_base + np.arange(len(mk))
    return _with_batch(stream, ops=ops, propsets=ps, props=pe)


def set_rewrite(stream, every):
    """MTE_F_REWRITE on every `every`-th sequenced annotate record."""
    ops = stream["batch"]["ops"].copy()
    ops["flags"][annotate_records(ops)[::every]] |= F_REWRITE
    return _with_batch(stream, ops=ops)


def touch_side_key_from(stream, frac, key=KEY_MARKER_ID):
    """Annotates after `frac` of each document's ops also carry `key` (small
    ids and null), so from there on text holds the key that only markers set."""
    b = stream["batch"]
    ops = b["ops"].copy()
    offs = b["op_offsets"].astype(np.int64)
    n = np.diff(offs)
    start = np.repeat(offs[:-1] + np.round(n * frac).astype(np.int64), n)
    ann = annotate_records(ops)
    ann = ann[ann >= start[ann]]
    olds = np.unique(ops["a"][ann])
    sets, table = [], np.zeros((3, int(olds.max()) + 1 if len(olds) else 1), np.int64)
    for w in range(3):
        for old in olds.tolist():
            table[w, old] = len(sets)
            own = _entries(b, old)
            sets.append(own + ([] if key in {k for k, _ in own} else [(key, _FILL[key][(old + 4 * w) % 9])]))
    ps, pe, base = _append_sets(b, sets)
    ops["a"][ann] = base + table[np.arange(len(ann)) % 3, ops["a"][ann]]
    return _with_batch(stream, ops=ops, propsets=ps, props=pe)


def prune_props(batch):
    """The batch with only the property sets its records use (renumbered).  The
    engine sizes its pass-1 layout from every id of a submitted table, used or
    not (mte_submit), so a batch cut out of a stream carries its own table."""
    ops = batch["ops"].copy()
    ann = annotate_records(ops)
    ins = np.flatnonzero((ops["type"] == OP_INSERT) & (ops["b"] != NO_PROPS))
    used = np.unique(np.concatenate([ops["a"][ann], ops["b"][ins]]).astype(np.int64))
    ps_old = batch["propsets"][used]
    cnt = ps_old["count"].astype(np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(used) else np.zeros(0, np.int64)
    src = np.repeat(ps_old["first"].astype(np.int64) - first, cnt) + np.arange(int(cnt.sum()))
    ps = np.zeros(len(used), PROPSET_DTYPE)
    ps["first"], ps["count"] = first, cnt
    new_id = np.full(len(batch["propsets"]) + 1, NO_PROPS, np.int64)
    new_id[used] = np.arange(len(used))
    ops["a"][ann] = new_id[ops["a"][ann]]
    ops["b"][ins] = new_id[ops["b"][ins]]
    return dict(batch, ops=ops, propsets=ps, props=batch["props"][src])


# ---- what a stream selects ----------------------------------------------------

def pass1_layout(tables, n_keys=N_KEYS, pack_env=True):
    """The pass-1 property layout launch_replay picks for a 4-key context
    (mte_engine.hip, `if constexpr (K == 4)`) after the tables in `tables`:
    (props, text_propsets) per mte_load_docs / mte_submit call, text_propsets
    the sets a text segment or an annotate used.  -> "packed", "side<k>" or
    "unpacked".  max_vid_k and key_text only grow."""
    assert n_keys == 4
    max_vid = np.zeros(8, np.int64)
    key_text = np.zeros(8, bool)
    for props, text_sets in tables:
        for k in range(8):
            v = props["value"][props["key"] == k]
            if len(v):
                max_vid[k] = max(max_vid[k], int(v.max()))
        for keys in text_sets:
            key_text[list(keys)] = True
    side, pack = None, pack_env
    for k in range(4):
        if not pack or max_vid[k] < 256:
            continue
        if side is None and not key_text[k]:
            side = k
        else:
            pack = False
    pack = pack and not max_vid[4:].any()
    if not pack:
        return "unpacked"
    return "packed" if side is None else f"side{side}"


def batch_tables(batch):
    """(props, keys of the sets text inserts and annotates use) of one batch."""
    ops = batch["ops"]
    ann = annotate_records(ops)
    txt = np.flatnonzero((ops["type"] == OP_INSERT) & ((ops["flags"] & F_MARKER) == 0) & (ops["b"] != NO_PROPS))
    used = np.unique(np.concatenate([ops["a"][ann], ops["b"][txt]]).astype(np.int64))
    keys = set()
    for psi in used.tolist():
        keys |= {k for k, _ in _entries(batch, psi)}
    return batch["props"], [keys]


def stream_layout(stream, pack_env=True):
    return pass1_layout([batch_tables(stream["batch"])], stream["n_keys"], pack_env)


def text_ids_at_least(batch, lo):
    """How many annotate records set a value id >= lo."""
    ops = batch["ops"]
    ann = annotate_records(ops)
    big = np.zeros(len(batch["propsets"]), bool)
    for psi in np.unique(ops["a"][ann]).tolist():
        big[psi] = any(v >= lo for _, v in _entries(batch, psi))
    return int(big[ops["a"][ann]].sum())


def wide_sets_applied(batch, lo=3):
    """How many annotate and marker-insert records carry a set of >= lo entries."""
    ops = batch["ops"]
    cnt = batch["propsets"]["count"]
    return int((cnt[ops["a"][annotate_records(ops)]] >= lo).sum() + (cnt[ops["b"][marker_records(ops)]] >= lo).sum())


def docs_with_cleared_markers(engine, docs, key=KEY_MARKER_ID):
    """Documents that hold a marker without its `key` property.  In a stream
    whose every marker is inserted with that key and whose annotates never name
    it, only a rewrite over the marker clears it."""
    hit = set()
    for doc in docs:
        segs, props, _ = engine.read_segments(doc)
        if ((segs["kind"] != 0) & (props[:, key] == 0)).any():
            hit.add(doc)
    return hit


def docs_with_rewritten_markers(stream, steps=12):
    """The documents in which a rewrite covered a marker, counted from the flat
    restatement: the stream replayed in `steps` batches, a cleared marker looked
    for after each (markers are short-lived: the final state alone shows few)."""
    from fluidframework_amd import gen
    from oracle import OracleEngine
    o = OracleEngine(stream["n_keys"], threads=8)
    gen.load_stream(o, stream)
    hit = set()
    for k in range(steps):
        o.apply_batch(gen.cut_ops(stream, k / steps, (k + 1) / steps))
        hit |= docs_with_cleared_markers(o, range(o.n_docs))
    return hit


# ---- the variants the flat-pass tests replay ---------------------------------

REWRITE_EVERY = 2


def small_marker_ids(stream):
    """markerId below 256 (64 + seq in the generator)."""
    return remap_values(stream, KEY_MARKER_ID, lambda v: 64 + v % 128)


def big_colors(stream):
    return remap_values(stream, KEY_COLOR, lambda v: v + 300)


def one_color_id(stream, to):
    return remap_values(small_marker_ids(stream), KEY_COLOR, lambda v: np.where(v == 44, to, v))


ALL_KEYS = (KEY_CLIENT, KEY_BOLD, KEY_COLOR, KEY_MARKER_ID)


def sticky_batches(stream, cuts=(0.0, 0.25, 0.6, 1.0)):
    """Three batches of one context that walk packed -> side key -> unpacked:
    the generator's markerId is 64 + seq, below 256 in the first quarter of 600
    ops and above after it, and the last batch's colors are ids >= 256.  Each
    batch carries only its own property sets (prune_props)."""
    from fluidframework_amd import gen
    big = big_colors(stream)
    return [prune_props(gen.cut_ops(big if k == 2 else stream, cuts[k], cuts[k + 1])) for k in range(3)]

# name -> (edit, the layout it forces)
LAYOUT_CASES = {
    "packed": (small_marker_ids, "packed"),
    "side": (lambda s: s, "side3"),
    "unpacked": (big_colors, "unpacked"),
    "id255": (lambda s: one_color_id(s, 255), "packed"),
    "id256": (lambda s: one_color_id(s, 256), "unpacked"),
    "wide_packed": (lambda s: small_marker_ids(widen_propsets(s, 3, ALL_KEYS, marker_sets=True)), "packed"),
    "wide_side": (lambda s: widen_propsets(s, 3, marker_sets=True), "side3"),
    "wide_unpacked": (lambda s: big_colors(widen_propsets(s, 3, ALL_KEYS, marker_sets=True)), "unpacked"),
    "rewrite_packed": (lambda s: set_rewrite(small_marker_ids(s), REWRITE_EVERY), "packed"),
    "rewrite_side": (lambda s: set_rewrite(s, REWRITE_EVERY), "side3"),
    "rewrite_unpacked": (lambda s: set_rewrite(big_colors(s), REWRITE_EVERY), "unpacked"),
}


# ---- capacity -----------------------------------------------------------------

def nsegs_trace(stream, before=()):
    """-> int64[n_docs, max ops + 1]: the segments each document holds before
    its op i (column i) in the flat restatement, tombstones included; after its
    last op the count repeats.  before: batches applied ahead of the traced one."""
    from fluidframework_amd import gen
    from oracle import OracleEngine
    b = stream["batch"]
    offs = b["op_offsets"].astype(np.int64)
    cnt = np.diff(offs)
    nd, steps = len(cnt), int(cnt.max()) if len(cnt) else 0
    o = OracleEngine(stream["n_keys"], threads=1)
    gen.load_stream(o, stream)
    for earlier in before:
        o.apply_batch(earlier)
    out = np.zeros((nd, steps + 1), np.int64)
    out[:, 0] = [o.nsegs(d) for d in range(nd)]
    for i in range(steps):
        has = cnt > i
        sub_offs = np.concatenate([[0], np.cumsum(has)]).astype(np.uint64)
        ops = b["ops"][offs[:-1][has] + i]
        # the step's own text: a restatement keeps every batch's text
        txt = np.flatnonzero((ops["type"] == OP_INSERT) & ((ops["flags"] & F_MARKER) == 0))
        pieces = [b["text"][int(ops["a"][r]):int(ops["a"][r]) + int(ops["pos2"][r])] for r in txt]
        ops["a"][txt] = np.concatenate([[0], np.cumsum([len(p) for p in pieces])[:-1]]) if len(txt) else 0
        text = np.concatenate(pieces) if pieces else b["text"][:0]
        o.apply_batch(dict(b, ops=ops, op_offsets=sub_offs, text=text))
        out[:, i + 1] = [o.nsegs(d) for d in range(nd)]
    return out


def first_ops(stream, counts):
    """The stream with only the first counts[d] ops of document d."""
    b = stream["batch"]
    offs = b["op_offsets"].astype(np.int64)
    counts = np.minimum(np.asarray(counts, np.int64), np.diff(offs))
    idx = np.concatenate([np.arange(offs[d], offs[d] + counts[d]) for d in range(len(counts))])
    new_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return _with_batch(stream, ops=b["ops"][idx], op_offsets=new_offs)


def ops_before_capacity(trace, cap, after=False):
    """How many ops of each document a flat pass applies in a context of `cap`
    segments.  One op can add two segments.  A pass that looks before the op
    takes it while the document leaves room for them (n_k + 2 <= cap) and stops
    the document for good at the first op that finds less; a pass that looks
    after it (`after`) stops at the first op that would leave less
    (n_k+1 + 2 > cap)."""
    full = (trace[:, 1:] if after else trace[:, :-1]) + 2 > cap
    return np.where(full.any(axis=1), full.argmax(axis=1), trace.shape[1] - 1)


def ops_peaking_at(trace, peak):
    """The longest prefix of each document's ops over which it never holds more
    than `peak` segments."""
    over = trace > peak
    return np.where(over.any(axis=1), over.argmax(axis=1) - 1, trace.shape[1] - 1)

