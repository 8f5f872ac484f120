"""Generated streams with tile labels on their markers (TEST INFRASTRUCTURE).

fluidframework_amd/gen.py's markers carry refType 1 and only a markerId.  For
the findTile tests every marker insert is rewritten, deterministically from its
sequence number (seq % 5), to cycle over

  0  referenceTileLabels ["pg"]
  1  referenceTileLabels ["li"]
  2  referenceTileLabels ["pg", "li"]
  3  no referenceTileLabels
  4  refType 2 (NestBegin, no Tile bit) with referenceTileLabels ["pg"]: never a tile

on both sides alike: the packed batch (label_stream, a fifth property key) and
the messages the reference replays (labelled_msgs).  The markerId stays.
"""
import json

import numpy as np

from fluidframework_amd import gen
from fluidframework_amd.abi import F_MARKER, OP_INSERT, PROP_DTYPE, PROPSET_DTYPE
from fluidframework_amd.messages import stream_doc_msgs
from fluidframework_amd.packing import TILE_LABELS_KEY, Interner

TILE_KEY = gen.N_KEYS  # the plane of "referenceTileLabels"
N_KEYS = gen.N_KEYS + 1
KEY_NAMES = gen.KEY_NAMES + [TILE_LABELS_KEY]
# value ids 49 .. 63 are free in the generator's table (mteg_value_json)
LABEL_VALUES = {49: ["pg"], 50: ["li"], 51: ["pg", "li"]}
CASE_VALUE = [49, 50, 51, 0, 49]  # per seq % 5
CASE_REFTYPE = [1, 1, 1, 1, 2]
LABELS = ["pg", "li", "zz"]


def value_json(vid):
    if vid in LABEL_VALUES:
        return json.dumps(LABEL_VALUES[vid], separators=(",", ":"))
    return gen.value_json(vid)


def label_stream(st):
    """The stream with its marker inserts rewritten (five property keys)."""
    b = st["batch"]
    ops = b["ops"].copy()
    ps, pe = b["propsets"], b["props"]
    mk = np.flatnonzero((ops["type"] == OP_INSERT) & (ops["flags"] & F_MARKER != 0))
    case = ops["seq"][mk] % 5
    ops["pos2"][mk] = np.array(CASE_REFTYPE)[case]
    new_ps, new_pe = [], []
    for i, c in zip(mk, case):
        old = ps[int(ops["b"][i])]
        ent = [tuple(x) for x in pe[int(old["first"]):int(old["first"]) + int(old["count"])]]
        if CASE_VALUE[c]:
            ent.append((TILE_KEY, CASE_VALUE[c]))
        ops["b"][i] = len(ps) + len(new_ps)
        new_ps.append((len(pe) + len(new_pe), len(ent)))
        new_pe.extend(ent)
    out = dict(st)
    out["n_keys"] = N_KEYS
    out["batch"] = dict(b, ops=ops,
                        propsets=np.concatenate([ps, np.array(new_ps, PROPSET_DTYPE).reshape(-1)]),
                        props=np.concatenate([pe, np.array(new_pe, PROP_DTYPE).reshape(-1)]))
    return out


def labelled_msgs(st, d):
    """Document d of the *unlabelled* stream as messages, with the same rewrite."""
    msgs = stream_doc_msgs(st, d)
    for m in msgs:
        c = m[5]
        if c and c.get("type") == 0 and isinstance(c.get("seg"), dict) and "marker" in c["seg"]:
            case = m[1] % 5
            c["seg"]["marker"]["refType"] = CASE_REFTYPE[case]
            if CASE_VALUE[case]:
                c["seg"].setdefault("props", {})[TILE_LABELS_KEY] = LABEL_VALUES[CASE_VALUE[case]]
    return msgs


def interner(max_vid):
    """An Interner holding the generator's keys and value ids [1, max_vid] as the
    labelled stream uses them, so engine.find_tiles and decode_props work on it."""
    it = Interner(N_KEYS)
    for name in KEY_NAMES:
        it.key(name)
    for vid in range(1, max_vid + 1):
        j = value_json(vid)
        it.value_json.append(j if j is not None else "null")
        if j is not None:
            it.values[j] = vid
    for vid in LABEL_VALUES:
        it.note_value(TILE_KEY, vid)
    return it


def stream_interner(st):
    return interner(int(st["batch"]["props"]["value"].max()))


def checkpoints(st, parts=4):
    """-> (batches, msgs): batch k of `parts` (gen.cut_ops, cut on message ends)
    and, per document, the number of messages applied after each batch (a
    generated record is one message, messages.stream_doc_msgs)."""
    batches = [gen.cut_ops(st, k / parts, (k + 1) / parts) for k in range(parts)]
    nd = len(st["inits"])
    msgs = np.zeros((nd, parts), np.int64)
    for k, b in enumerate(batches):
        o = b["op_offsets"].astype(np.int64)
        msgs[:, k] = o[1:] - o[:-1]
    return batches, np.cumsum(msgs, axis=1)


def generate(S):
    """The unlabelled stream of a vectors set."""
    return gen.generate(S["config"], n_docs=S["n_docs"], ops_per_doc=S["ops_per_doc"], **S["params"])


def rle(xs):
    """[v0, n0, v1, n1, ...]"""
    out = []
    for x in xs:
        if out and out[-2] == x:
            out[-1] += 1
        else:
            out += [x, 1]
    return out


def unrle(r):
    out = []
    for v, n in zip(r[0::2], r[1::2]):
        out += [v] * n
    return out
