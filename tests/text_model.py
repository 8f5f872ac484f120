"""MergeTreeTextHelper.getText (MergeTreeTextHelper.ts:20-74) and
Client.getPropertiesAtPosition (client.ts:1133-1141) stated flat over a read_doc
view: the visible segments in order as (len, kind, props), kind = 0 text,
1 + refType marker, and the text units of the text segments.  TEST
INFRASTRUCTURE."""
from fluidframework_amd.packing import units_to_str, utf16_units


def get_text(view, start=0, end=None, placeholders=False):
    """The units at positions p of the view with start <= p < min(end, length):
    a text unit gives itself, a marker position nothing or, with placeholders,
    one space."""
    end = view["length"] if end is None else end
    units = view.get("_units")  # positions count UTF-16 code units
    if units is None:
        units = view["_units"] = utf16_units(view["text"])
    out, p, t = [], 0, 0
    for ln, kind, _ in view["segs"]:
        lo, hi = max(p, start), min(p + ln, end)
        if hi > lo:
            if kind == 0:
                out.append(units_to_str(units[t + lo - p:t + hi - p]))
            elif placeholders:
                out.append(" " * (hi - lo))
        if kind == 0:
            t += ln
        p += ln
    return "".join(out)


def segment_at(view, pos):
    """-> None | (kind, property planes) of the segment with P <= pos < P + L."""
    p = 0
    for ln, kind, planes in view["segs"]:
        if p <= pos < p + ln:
            return kind, planes
        p += ln
    return None
