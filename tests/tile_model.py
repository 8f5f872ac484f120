"""MergeTree.findTile (mergeTree.ts:1135-1163) stated flat over a read_doc view:
the visible segments in order as (len, kind, props), kind = 0 text, 1 + refType
marker, props decoded to a dict.  TEST INFRASTRUCTURE."""
TILE_LABELS_KEY = "referenceTileLabels"


def find_tile(segs, start_pos, label, preceding=True):
    """-> None | (pos, refType, props): preceding, the last matching marker at a
    position <= start_pos; following, the first at a position >= start_pos, for
    start_pos < length only."""
    length = sum(ln for ln, _, _ in segs)
    hit, p = None, 0
    for ln, kind, props in segs:
        labels = props.get(TILE_LABELS_KEY)
        if ln > 0 and kind and ((kind - 1) & 1) and isinstance(labels, list) and label in labels:
            if preceding and p <= start_pos:
                hit = (p, kind - 1, props)
            if not preceding and start_pos <= p and start_pos < length:
                return (p, kind - 1, props)
        p += ln
    return hit


def tile_answers(segs, label, preceding):
    """find_tile's position (-1: None) for every start position the vectors
    record, in one sweep: preceding p in [0, length] then length + 5, following
    p in [0, length).  Equal to find_tile position by position (the tests check
    a sample); it only saves the rescan per position."""
    length = sum(ln for ln, _, _ in segs)
    marks, p = [], 0
    for ln, kind, props in segs:
        labels = props.get(TILE_LABELS_KEY)
        if ln > 0 and kind and ((kind - 1) & 1) and isinstance(labels, list) and label in labels:
            marks.append(p)
        p += ln
    out, i = [], 0
    if preceding:
        for q in list(range(length + 1)) + [length + 5]:
            while i < len(marks) and marks[i] <= q:
                i += 1
            out.append(marks[i - 1] if i else -1)
    else:
        for q in range(length):
            while i < len(marks) and marks[i] < q:
                i += 1
            out.append(marks[i] if i < len(marks) else -1)
    return out


def decoded_segs(view, interner):
    """read_doc()["segs"] with the property planes decoded."""
    return [(ln, kind, interner.decode_props(pl)) for ln, kind, pl in view["segs"]]


def text_with_placeholders(view):
    """getTextWithPlaceholders (MergeTreeTextHelper.ts:49-74, placeholder " ")."""
    out, t = [], 0
    for ln, kind, _ in view["segs"]:
        if kind:
            out.append(" " * ln)
        else:
            out.append(view["text"][t:t + ln])
            t += ln
    return "".join(out)
