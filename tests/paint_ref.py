"""numpy restatement of Path.fill's pattern branch (what svgr_pattern_fill computes per pixel, include/svgr.h), and the four
gradients of the tall-box tests (tests/test_gpu_filter_paint_seams.py) with the restated determinant of the focal form.  Written
from the header's description of the reference's operations, not from the kernel; test infrastructure only."""
from fractions import Fraction

import numpy as np

_fma = np.frompyfunc(lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c)), 3, 1)


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic: float(Fraction) rounds to nearest even); finite inputs."""
    return np.asarray(_fma(a, b, c), dtype=np.float64)


def xform(m6, p0, p1):
    """Transform.__call__ in the fma form of csrc/svgr_core.h's xform_point: fma(p1, m1, p0 * m0) + m2."""
    return fma(p1, m6[1], p0 * m6[0]) + m6[2], fma(p1, m6[4], p0 * m6[3]) + m6[5]


def pattern_canvas(pat, tile):
    """The (pw, ph, 4) pattern canvas: zero except for the tile at tile_bbox, clipped to [0, 1] (and to the canvas)."""
    canvas = np.zeros(tuple(pat["pat_shape"]) + (4,))
    x, y, rows, cols = pat["tile_bbox"]
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + rows, canvas.shape[0]), min(y + cols, canvas.shape[1])
    if x1 > x0 and y1 > y0:
        canvas[x0:x1, y0:y1] = np.clip(tile[x0 - x:x1 - x, y0 - y:y1 - y], 0.0, 1.0)
    return canvas


def pattern_fill(pat, tile, mask, bbox):
    """out (rows, cols, 4) over the pixel grid of bbox = (r0, c0, rows, cols); pat: dict(inv_m6, fwd_m6, cell, min_xy, pat_shape,
    tile_bbox) as svgr_pattern.  Raises IndexError where numpy does: an offset outside the canvas, on either side."""
    r0, c0, rows, cols = bbox
    i, j = np.indices((rows, cols)).astype(np.float64)
    ux, uy = xform(pat["inv_m6"], i + (r0 + 0.5), j + (c0 + 0.5))
    cx, cy, cw, ch = pat["cell"]
    tx, ty = xform(pat["fwd_m6"], np.remainder(ux - cx, cw), np.remainder(uy - cy, ch))
    ox, oy = tx.astype(int) - pat["min_xy"][0], ty.astype(int) - pat["min_xy"][1]
    return pattern_canvas(pat, tile)[ox, oy] * mask[..., None]   # (numpy's own indexing: negative offsets wrap once)


def pattern_geometry(lin, cell, tile_xy, tile_shape, translate=(0.0, 0.0)):
    """svgr_pattern's fields the way paint.pattern_fill derives them from the repeat transform's 2 x 2 part `lin`: the inverse
    (with `translate`, the fill's own translation, folded in), the forward map without translation, and the canvas of the
    transformed cell's corners truncated like ndarray.astype(int)."""
    lin = np.asarray(lin, dtype=np.float64)
    x, y, w, h = cell
    corners = np.array([[0, 0], [w, 0], [0, h], [w, h]], dtype=np.float64) @ lin.T
    mx, my = corners.max(axis=0).astype(int)
    nx, ny = corners.min(axis=0).astype(int)
    inv = np.linalg.inv(lin)
    t = -inv @ np.asarray(translate, dtype=np.float64)
    return dict(inv_m6=[inv[0, 0], inv[0, 1], t[0], inv[1, 0], inv[1, 1], t[1]], fwd_m6=[lin[0, 0], lin[0, 1], 0.0, lin[1, 0], lin[1, 1], 0.0],
                cell=[float(v) for v in cell], min_xy=[int(nx), int(ny)], pat_shape=[int(mx - nx) + 1, int(my - ny) + 1],
                tile_bbox=[int(tile_xy[0]) - int(nx), int(tile_xy[1]) - int(ny), int(tile_shape[0]), int(tile_shape[1])])


# -- the gradients of the tall boxes ---------------------------------------------------------------------------------------------
# k_gradient_fill / k_gradient_detneg launch min(rows, 32768) block rows and stride over the rest: a box of 32770 rows takes a
# second trip in block rows 0 and 1 (rows 32768 and 32769).  The boxes start at (-3, 11): pixel [i, j] has its centre at the
# device point (i - 2.5, j + 11.5).
TALL_ROWS, TALL_R0, TALL_C0 = 32770, -3, 11
FIRST_SECOND_TRIP_ROW = 32768
STOPS = [(0.0, (0.9, 0.1, 0.05, 1.0)), (0.35, (0.1, 0.6, 0.2, 0.7)), (1.0, (0.05, 0.15, 0.8, 0.9))]
LONG_STOPS = [(0.0, (0.8, 0.2, 0.1, 1.0)), (0.7, (0.1, 0.5, 0.3, 0.6)), (3.0, (0.2, 0.1, 0.7, 0.9))]
_SCALED = [[1.0 / 64, 0.0, 1.5], [0.0, 0.25, -2.25], [0.0, 0.0, 1.0]]   # device -> user: rows to [1.4, 513.5], columns to [0.6, 64.8]
_U0 = float(TALL_R0 + FIRST_SECOND_TRIP_ROW)   # the device row coordinate between the centres of rows 32767 and 32768
# "focal_detneg": the focus F = (U0, 11.25) lies on the line row = U0, which touches the circle (radius R = 158218, centre
# (U0 - R, 11.25 + L), L = 65536) at (U0, 11.25 + L): one of the two tangents from F.  det >= 0 on the double cone between the
# tangents, which opens by 2 atan(R / L) = 135 degrees from the direction of growing columns towards smaller rows.  All pixel
# centres lie right of F (by 0.25, 1.25, ...), so every centre below U0 is in the cone's first half, with an offset > 0 (2.7 at
# most).  Beyond U0 (by 0.5 and 1.5: rows 32768 and 32769) a centre is outside the cone, det < 0, where its distance beyond U0 is
# less than its distance right of F, and in the mirrored half otherwise: det >= 0 with an offset < 0 -- pixels that are masked
# only because some other pixel has det < 0.
_L, _R, _FV = 65536.0, 158218.0, TALL_C0 + 0.25
GRADIENTS = {
    "linear": dict(kind="linear", user=_SCALED, spread="pad", stops=STOPS, p0=(1.0, -1.0), p1=(514.0, 70.0)),
    "radial": dict(kind="radial", user=_SCALED, spread="reflect", stops=STOPS, center=(200.0, 10.0), radius=150.0),
    "focal_inside": dict(kind="radial", user=_SCALED, spread="pad", stops=STOPS, center=(256.0, 30.0), radius=400.0, fcenter=(250.0, 20.0),
                         fradius=5.0),
    "focal_detneg": dict(kind="radial", user=np.identity(3).tolist(), spread="pad", stops=LONG_STOPS, center=(_U0 - _R, _FV + _L),
                         radius=_R, fcenter=(_U0, _FV), fradius=None),
}


def tall_box(cols):
    return (TALL_R0, TALL_C0, TALL_ROWS, cols)


def oracle_kwargs(g):
    """The geometry keywords of oracle.gradient_image."""
    if g["kind"] == "linear":
        return dict(p0=np.array(g["p0"]), p1=np.array(g["p1"]))
    return dict(center=np.array(g["center"]), radius=g["radius"], fcenter=None if g.get("fcenter") is None else np.array(g["fcenter"]),
                fradius=g.get("fradius"))


def focal_det(g, bbox):
    """det = b^2 - a c of the focal form at every pixel centre of bbox (the header's S:1619-1626, plain numpy)."""
    r0, c0, rows, cols = bbox
    i, j = np.indices((rows, cols)).astype(np.float64)
    m = np.asarray(g["user"], dtype=np.float64)
    px, py = i + (r0 + 0.5), j + (c0 + 0.5)
    x, y = m[0, 0] * px + m[0, 1] * py + m[0, 2], m[1, 0] * px + m[1, 1] * py + m[1, 2]
    fr = g.get("fradius") or 0.0
    cd = np.array(g["center"]) - np.array(g["fcenter"])
    rd = g["radius"] - fr
    b = (x - g["fcenter"][0]) * cd[0] + (y - g["fcenter"][1]) * cd[1] + fr * rd
    c = (x - g["fcenter"][0]) ** 2 + (y - g["fcenter"][1]) ** 2 - fr * fr
    return b * b - ((cd ** 2).sum() - rd * rd) * c
