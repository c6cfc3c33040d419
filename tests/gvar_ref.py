"""Reference of the variable-font definitions (DESIGN.md "Variable fonts") in plain Python floats and elementwise numpy: every
product, quotient and sum is one IEEE double operation of its own, in the order the definition fixes, so the result is
comparable bit for bit.  It works from what a test hands to the writers of tests/gvar_cases.py -- glyphs as lists of contours
of ``(x, y, on)``, tuples as dicts or as ``(scalar, [(index, dx, dy)])`` -- never from parsed bytes, and it looks for a point's
neighbours by walking the contour, not by searching a sorted list."""
import math

from tests import ttf_ref as R


def f2dot14(v: float) -> float:
    """`v` as the writers store it."""
    return round(v * 16384) / 16384.0


def normalise(axis, segment_map, value: float) -> float:
    """`axis`: ``(tag, minimum, default, maximum)``; `segment_map`: ``[(from, to)]`` or None."""
    _tag, lo, default, hi = axis
    v = min(max(float(value), lo), hi)
    if v == default:
        n = 0.0
    elif v < default:
        n = (v - default) / (default - lo)
    else:
        n = (v - default) / (hi - default)
    if segment_map:
        pairs = [(f2dot14(k), f2dot14(m)) for k, m in segment_map]
        hit = [m for k, m in pairs if k == n]
        if hit:
            n = hit[0]
        else:
            below = [(k, m) for k, m in pairs if k < n]
            above = [(k, m) for k, m in pairs if k > n]
            if below and above:
                (ka, va), (kb, vb) = below[-1], above[0]
                n = va + (vb - va) * (n - ka) / (kb - ka)
    return math.floor(n * 16384 + 0.5) / 16384


def location(axes, maps, user: dict) -> tuple:
    """The normalised coordinates, per axis, of ``{tag: user value}``."""
    return tuple(normalise(axis, m, user.get(axis[0], axis[2])) for axis, m in zip(axes, maps))


def scalar(t: dict, coords) -> float:
    """The scalar of the tuple description `t` at the normalised `coords`."""
    s = 1.0
    for a, n in enumerate(coords):
        peak = f2dot14(t["peak"][a])
        if peak == 0:
            continue
        if n == peak:
            continue
        if t.get("start") is None:
            if n == 0 or n < min(0.0, peak) or n > max(0.0, peak):
                return 0.0
            s = s * (n / peak)
        else:
            start, end = f2dot14(t["start"][a]), f2dot14(t["end"][a])
            if n <= start or n >= end:
                return 0.0
            s = s * ((n - start) / (peak - start) if n < peak else (end - n) / (end - peak))
    return s


def _axis(cp, cq, ci, dp, dq):
    if cp == cq:
        return dp if dp == dq else 0.0
    (c1, d1), (c2, d2) = ((cp, dp), (cq, dq)) if cp < cq else ((cq, dq), (cp, dp))
    if ci <= c1:
        return d1
    if ci >= c2:
        return d2
    s = (d2 - d1) / (c2 - c1)
    prod = (ci - c1) * s
    return d1 + prod


def tuple_delta(glyph, entries) -> list:
    """``[(dx, dy)]`` per point of `glyph` (a list of contours) in one tuple with the entries ``[(local index, dx, dy)]``."""
    stored = {i: (float(dx), float(dy)) for i, dx, dy in entries}
    pts = [(float(x), float(y)) for c in glyph for x, y, _on in c]
    out = [(0.0, 0.0)] * len(pts)
    f = 0
    for c in glyph:
        members = list(range(f, f + len(c)))
        f += len(c)
        touched = [i for i in members if i in stored]
        if not touched:
            continue
        for i in members:
            if i in stored:
                out[i] = stored[i]
                continue
            before, after = [t for t in touched if t < i], [t for t in touched if t > i]
            p = before[-1] if before else touched[-1]
            q = after[0] if after else touched[0]
            out[i] = tuple(_axis(pts[p][e], pts[q][e], pts[i][e], stored[p][e], stored[q][e]) for e in (0, 1))
    return out


def deltas(atlas, tuples) -> list:
    """Per glyph of `atlas` the list of ``(Dx, Dy)`` per point: the sum over the glyph's tuples ``(scalar, entries)`` in order."""
    out = []
    for glyph, glyph_tuples in zip(atlas, tuples):
        total = [(0.0, 0.0)] * sum(len(c) for c in glyph)
        for s, entries in glyph_tuples:
            one = tuple_delta(glyph, entries)
            total = [(tx + s * dx, ty + s * dy) for (tx, ty), (dx, dy) in zip(total, one)]
        out.append(total)
    return out


def flat(per_glyph):
    import numpy as np

    rows = [d for g in per_glyph for d in g]
    return np.array(rows, dtype=np.float64).reshape(-1, 2)


def varied(atlas, tuples) -> list:
    """`atlas` with every point moved by its delta: contours of ``(x + Dx, y + Dy, on)``, floats."""
    out = []
    for glyph, total in zip(atlas, deltas(atlas, tuples)):
        moved, k = [], 0
        for c in glyph:
            moved.append([(float(x) + total[k + i][0], float(y) + total[k + i][1], on) for i, (x, y, on) in enumerate(c)])
            k += len(c)
        out.append(moved)
    return out


def outline_var(atlas, tuples, parts):
    """`ttf_ref.outline` of the varied points."""
    return R.outline(varied(atlas, tuples), parts)


# ---- a font description at a location: what the parser and the instance are held against ---------------------------------
def point_count(glyph) -> int:
    return len(glyph["components"]) if isinstance(glyph, dict) else sum(len(c) for c in glyph)


def live(glyph, glyph_variations, coords) -> list:
    """``[(scalar, {point number: (dx, dy)})]`` of a glyph's tuple descriptions at `coords`: scalar 0 dropped, "all points"
    spelled out."""
    out = []
    for t in glyph_variations:
        s = scalar(t, coords)
        if s == 0.0:
            continue
        points = t.get("points")
        if points is None:
            points = range(point_count(glyph) + 4)
        out.append((s, {p: d for p, d in zip(points, t["deltas"]) if p < point_count(glyph) + 4}))
    return out


def device_tuples(glyphs, variations, coords) -> list:
    """Per glyph the ``(scalar, entries)`` the device gets at `coords`: phantom points stripped (composites: nothing)."""
    out = []
    for glyph, gv in zip(glyphs, variations):
        n = 0 if isinstance(glyph, dict) else point_count(glyph)
        out.append([(s, sorted((p, d[0], d[1]) for p, d in stored.items() if p < n)) for s, stored in live(glyph, gv, coords)])
    return out


def advance(glyphs, advances, variations, coords, gid) -> float:
    """The ``hmtx`` advance plus the sum of ``scalar * (dx[n + 1] - dx[n])``."""
    n, total = point_count(glyphs[gid]), 0.0
    for s, stored in live(glyphs[gid], variations[gid], coords):
        total = total + s * (float(stored.get(n + 1, (0, 0))[0]) - float(stored.get(n, (0, 0))[0]))
    return float(advances[gid]) + total


def flatten(glyphs, variations, coords, gid):
    """`ttf_ref.flatten` with the offsets of every composite's components moved by their summed deltas."""
    g = glyphs[gid]
    if not isinstance(g, dict):
        return [(gid, *R.IDENTITY)] if any(len(c) for c in g) else []
    tuples = live(g, variations[gid], coords)
    out = []
    for k, comp in enumerate(g["components"]):
        m = list(R.component_matrix(comp))
        sx = sy = 0.0
        for s, stored in tuples:
            if k in stored:
                sx = sx + s * float(stored[k][0])
                sy = sy + s * float(stored[k][1])
        m[4], m[5] = m[4] + sx, m[5] + sy
        for simple, *child in flatten(glyphs, variations, coords, comp["glyph"]):
            out.append((simple, *(float(v) for v in R.compose(child, m))))
    return out


def string_parts(glyphs, cmap, advances, kern, variations, coords, text):
    """`ttf_ref.string_parts` at a location: (atlas of varied glyphs, parts without scales, total advance)."""
    atlas = [[] if isinstance(g, dict) else g for g in glyphs]
    atlas = varied(atlas, device_tuples(glyphs, variations, coords))
    parts, pen, prev = [], 0.0, None
    for ch in text:
        gid = cmap.get(ord(ch), 0)
        if prev is not None:
            pen += (kern or {}).get((prev, gid), 0)
        parts.extend((simple, tuple(m), pen) for simple, *m in flatten(glyphs, variations, coords, gid))
        pen += advance(glyphs, advances, variations, coords, gid)
        prev = gid
    return atlas, parts, pen
