"""Reference of the CFF outline pass (svgr_cff_outline) in elementwise numpy: every product and every sum is a
ufunc call of its own on float64 -- no ``@`` / ``dot``, which may fuse -- in the order the definition fixes, so the result is
comparable bit for bit.  It works from the contours a test states (lists of ``(x, y, kind)``), never from parsed bytes; what a
charstring decodes to is stated by the cases themselves (tests/cff_cases.py)."""
import numpy as np

PATH_LINE, PATH_CUBIC, PATH_CLOSED = 0, 2, 4
MOVE, LINE, C1, C2, CURVE = 0, 1, 2, 3, 4
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _place(m, pen, sx, sy, x, y):
    m00, m01, m10, m11, dx, dy = (np.float64(v) for v in m)
    xp = (m00 * x + m10 * y) + dx
    yp = (m01 * x + m11 * y) + dy
    return (xp + np.float64(pen)) * np.float64(sx), yp * np.float64(sy)


def contour(points, m=IDENTITY, pen=0.0, sx=1.0, sy=1.0):
    """(types, params (k, 8)) of one contour; None for a lone MOVE (or no point)."""
    n = len(points)
    if n < 2:
        return None
    kind = np.array([p[2] for p in points])
    assert kind[0] == MOVE and (kind[1:] != MOVE).all()
    X, Y = _place(m, pen, sx, sy, np.array([p[0] for p in points], dtype=np.float64), np.array([p[1] for p in points], dtype=np.float64))
    zero = np.zeros(n)
    back = lambda v, k: np.roll(v, k)   # noqa: E731  (v[a - k]; the rows that wrap are never taken)
    line = np.stack([back(X, 1), back(Y, 1), X, Y, zero, zero, zero, zero], axis=1)
    cubic = np.stack([back(X, 3), back(Y, 3), back(X, 2), back(Y, 2), back(X, 1), back(Y, 1), X, Y], axis=1)
    emits = (kind == LINE) | (kind == CURVE)
    rows = np.where((kind == LINE)[:, None], line, cubic)[emits]
    types = np.where(kind == LINE, PATH_LINE, PATH_CUBIC)[emits]
    close = np.array([[X[n - 1], Y[n - 1], X[0], Y[0], 0.0, 0.0, 0.0, 0.0]])   # from the last point to the first
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


def string_parts(glyphs, cmap, advances, kern, text):
    """(atlas, parts without scales, total advance) of `text` over decoded `glyphs` (lists of contours): pens from the advances
    and the kerning (the ``kern`` table's sign: the value is added to the pen), one glyph per character, glyph 0 for an unmapped
    one; an empty glyph has no part."""
    parts, pen, prev = [], 0.0, None
    for ch in text:
        gid = cmap.get(ord(ch), 0)
        if prev is not None:
            pen += (kern or {}).get((prev, gid), 0)
        if glyphs[gid]:
            parts.append((gid, IDENTITY, pen))
        pen += advances[gid]
        prev = gid
    return glyphs, parts, pen
