"""Reference of the TrueType outline pass (svgr_glyf_outline; DESIGN.md "TrueType fonts") in elementwise numpy: every product
and every sum is a ufunc call of its own on float64 -- no ``@`` / ``dot``, which may fuse -- in the order the definition
fixes, so the result is comparable bit for bit.  It works from the points a test hands to the font builder (lists of contours
of ``(x, y, on)``), never from parsed bytes."""
import numpy as np

PATH_LINE, PATH_CUBIC, PATH_CLOSED = 0, 2, 4
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _place(m, pen, sx, sy, x, y):
    m00, m01, m10, m11, dx, dy = (np.float64(v) for v in m)
    xp = (m00 * x + m10 * y) + dx
    yp = (m01 * x + m11 * y) + dy
    return (xp + np.float64(pen)) * np.float64(sx), yp * np.float64(sy)


def contour(points, m=IDENTITY, pen=0.0, sx=1.0, sy=1.0):
    """(types, params (k, 8)) of one contour; None for fewer than 2 points."""
    n = len(points)
    if n < 2:
        return None
    x = np.array([p[0] for p in points], dtype=np.float64)
    y = np.array([p[1] for p in points], dtype=np.float64)
    on = np.array([bool(p[2]) for p in points])
    xp, yp, on_p = np.roll(x, 1), np.roll(y, 1), np.roll(on, 1)
    xn, yn, on_n = np.roll(x, -1), np.roll(y, -1), np.roll(on, -1)
    half = np.float64(0.5)
    # the quadratic of an off-curve point
    ax, ay = np.where(on_p, xp, (xp + x) * half), np.where(on_p, yp, (yp + y) * half)
    bx, by = np.where(on_n, xn, (x + xn) * half), np.where(on_n, yn, (y + yn) * half)
    p0x, p0y = _place(m, pen, sx, sy, ax, ay)
    qx, qy = _place(m, pen, sx, sy, x, y)
    p1x, p1y = _place(m, pen, sx, sy, bx, by)
    third, two_thirds = np.float64(1.0) / np.float64(3), np.float64(2.0) / np.float64(3)
    cubic = np.stack([p0x, p0y, third * p0x + two_thirds * qx, third * p0y + two_thirds * qy,
                      two_thirds * qx + third * p1x, two_thirds * qy + third * p1y, p1x, p1y], axis=1)
    # the line of an on-curve point with an on-curve next
    lx, ly = _place(m, pen, sx, sy, xn, yn)
    line = np.stack([qx, qy, lx, ly, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)], axis=1)
    emits = ~on | on_n
    rows = np.where(on[:, None], line, cubic)[emits]
    types = np.where(on, PATH_LINE, PATH_CUBIC)[emits]
    # the closing line, of length 0, at the chain's start
    if on[0]:
        s = (x[0], y[0])
    elif on[n - 1]:
        s = (x[n - 1], y[n - 1])
    else:
        s = ((x[n - 1] + x[0]) * half, (y[n - 1] + y[0]) * half)
    cx, cy = _place(m, pen, sx, sy, np.float64(s[0]), np.float64(s[1]))
    close = np.array([[cx, cy, cx, cy, 0.0, 0.0, 0.0, 0.0]])
    return np.concatenate([types, [PATH_CLOSED]]).astype(np.int32), np.concatenate([rows, close])


def outline(atlas, parts):
    """(types int32, params (n, 8) float64, sizes int32) of `parts` = ``[(glyph index, m, pen, sx, sy)]`` over `atlas`, a list
    of glyphs as lists of contours."""
    types, params, sizes = [np.zeros(0, np.int32)], [np.zeros((0, 8))], []
    for g, m, pen, sx, sy in parts:
        for points in atlas[g]:
            got = contour(points, m, pen, sx, sy)
            if got is None:
                continue
            types.append(got[0])
            params.append(got[1])
            sizes.append(len(got[0]))
    return np.concatenate(types), np.concatenate(params), np.array(sizes, dtype=np.int32)


def compose(child, parent):
    """The matrix of a component `child` inside a composite that is itself placed by `parent` (both ``(m00, m01, m10, m11, dx,
    dy)``, a point going to ``(m00 x + m10 y + dx, m01 x + m11 y + dy)``): child first, then parent."""
    c00, c01, c10, c11, cdx, cdy = (np.float64(v) for v in child)
    p00, p01, p10, p11, pdx, pdy = (np.float64(v) for v in parent)
    return (c00 * p00 + c01 * p10, c00 * p01 + c01 * p11, c10 * p00 + c11 * p10, c10 * p01 + c11 * p11,
            (cdx * p00 + cdy * p10) + pdx, (cdx * p01 + cdy * p11) + pdy)


def component_matrix(comp):
    """``(m00, m01, m10, m11, dx, dy)`` of a builder's component description (a component placed by point matching: offset 0)."""
    scale = comp.get("scale")
    q = [round(v * 16384) / 16384.0 for v in ((scale,) if isinstance(scale, (int, float)) else tuple(scale or ()))]
    if len(q) == 4:      # xscale, scale01, scale10, yscale
        m = q
    elif len(q) == 2:
        m = [q[0], 0.0, 0.0, q[1]]
    elif len(q) == 1:
        m = [q[0], 0.0, 0.0, q[0]]
    else:
        m = [1.0, 0.0, 0.0, 1.0]
    dx, dy = (0, 0) if comp.get("match") is not None else (comp.get("dx", 0), comp.get("dy", 0))
    return (*[float(v) for v in m], float(dx), float(dy))


def flatten(glyphs, gid):
    """``[(simple glyph id, m00, m01, m10, m11, dx, dy)]`` of glyph `gid` of the builder's glyph list (no cycles, please)."""
    g = glyphs[gid]
    if not isinstance(g, dict):
        return [(gid, *IDENTITY)] if any(len(c) for c in g) else []
    out = []
    for comp in g["components"]:
        for simple, *m in flatten(glyphs, comp["glyph"]):
            out.append((simple, *(float(v) for v in compose(m, component_matrix(comp)))))
    return out


def string_parts(glyphs, cmap, advances, kern, text):
    """(atlas, parts without scales, total advance) of `text`: pens from the advances and the kerning (TrueType's sign: the
    value is added to the pen), one glyph per character, glyph 0 for an unmapped one.  The atlas is `glyphs` itself, composites
    as empty glyphs."""
    atlas = [[] if isinstance(g, dict) else g for g in glyphs]
    parts, pen, prev = [], 0.0, None
    for ch in text:
        gid = cmap.get(ord(ch), 0)
        if prev is not None:
            pen += (kern or {}).get((prev, gid), 0)
        parts.extend((simple, tuple(m), pen) for simple, *m in flatten(glyphs, gid))
        pen += advances[gid]
        prev = gid
    return atlas, parts, pen
