"""The dasher's test inputs, shared by tests/test_dash_host.py (which checks them against the conditions of dash_ref's
docstring, on the CPU) and tests/test_gpu_dash.py (which runs them through the C ABI).  A case is
(name, (types, params, sizes), dashes, offset, path_length, exact): `exact` marks integer-length lines with integer dashes,
whose arithmetic is the same under every association (boundaries may then sit on joints)."""
import numpy as np

from tests import dash_ref as R

S = 1024   # segments one workgroup of the dasher's scans covers (svgr_dash_scan_segments; the GPU test checks the value)

# Largest distance between the control points of the end-to-end document's dashed cubic ("M4,40 C20,20 40,60 60,40", dashes
# 5 3) as dash_ref computes them in float64 and in long double, in user units (= pixels), measured on the CPU
# (tests/test_dash_host.py::test_cubic_outline_distance_is_as_recorded measures it again).  The device's outline may lie
# 4 x that from dash_ref's float64 one (tests/test_gpu_dash.py).
CUBIC_DISTANCE = 7.105427357601002e-15


def stairs(n, closed=False):
    """n axis-aligned lines of integer lengths 1..5: a staircase (closed: back to the start by the closing line, whose length is
    not an integer -- such cases are not marked exact)."""
    pts, x, y = [(0, 0)], 0, 0
    for i in range(n):
        step = 1 + (i * 7 + 3) % 5
        if i % 2 == 0:
            x += step
        else:
            y += step
        pts.append((x, y))
    return R.polyline(pts, closed)


def cubic_chain(n, seed, scale=40.0):
    """n smooth cubics, end to end."""
    rng = np.random.default_rng(seed)
    segs, p = [], np.array([0.0, 0.0])
    for _ in range(n):
        d = rng.uniform(0.3, 1.0, 2) * scale
        c1 = p + d * rng.uniform(0.2, 0.5) + rng.uniform(-0.2, 0.2, 2) * scale
        c2 = p + d * rng.uniform(0.6, 0.9) + rng.uniform(-0.2, 0.2, 2) * scale
        e = p + d
        segs.append((R.CUBIC, [*p, *c1, *c2, *e]))
        p = e
    return segs


def mixed_chain(n, seed):
    rng = np.random.default_rng(seed)
    segs, p = [], np.array([0.0, 0.0])
    for c in cubic_chain(n, seed + 1000):
        q = np.array(c[1]).reshape(4, 2) - np.array(c[1][:2]) + p
        if rng.random() < 0.5:
            segs.append((R.LINE, [*q[0], *q[3]]))
        else:
            segs.append((R.CUBIC, list(q.reshape(8))))
        p = q[3]
    return segs


def _length(path):
    d = {}
    R.dash(*path, [1.0, 1.0], detail=d)
    return d["length"]


def fixed_cases():
    out = []
    rect = R.polyline([(0, 0), (100, 0), (100, 50), (0, 50)], closed=True)
    for n in (1, 2, 3, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1):
        out.append((f"lines{n}", stairs(n), [3, 2], 1, 0, True))
    for n in (1, 2, 3, 63, 64, 65, S + 1):
        path = R.from_segments(cubic_chain(n, n))
        L = _length(path)
        out.append((f"cubics{n}", path, [L * 0.13 / min(4, max(1, n // 64)), L * 0.07 / min(4, max(1, n // 64))], L * 0.01, 0, False))
    for n in (3, 65, S - 1, S, 2 * S + 1):
        path = R.from_segments(mixed_chain(n, n))
        L = _length(path)
        out.append((f"mix{n}", path, [L * 0.11 / min(4, max(1, n // 64)), L * 0.05 / min(4, max(1, n // 64))], L * 0.0073, 0, False))
    out.append(("subpaths65", R.concat(*[R.polyline([(0, 3 * i), (7 + i % 3, 3 * i)]) for i in range(65)]), [2, 1], 0, 0, True))
    out.append(("pieces4000", R.polyline([(0, 0), (1000, 0)]), [0.25, 0.25], 0, 0, True))
    for m in (1, 2, 3, 8, 64):
        out.append((f"pattern{m}", stairs(40), [1 + (i * 3) % 4 for i in range(m)], 2, 0, True))
    out.append(("closed_whole", rect, [400, 10], 0, 0, True))
    out.append(("closed_whole_offset", rect, [400, 10], -50, 0, True))
    out.append(("closed_merge", rect, [25, 10], 0, 0, True))
    out.append(("closed_merge_corner", rect, [30, 20], 5, 0, True))
    # a merged dash whose pieces lie on both sides of a workgroup's reach: a closed square ring of S + 8 unit lines, whose
    # trailing dash ends in segment S + 7 and whose leading dash begins in segment 0
    n_side = (S + 8) // 4 + 1
    ring = [(i, 0) for i in range(n_side)] + [(n_side - 1, i) for i in range(1, n_side)] + \
           [(n_side - 1 - i, n_side - 1) for i in range(1, n_side)] + [(0, n_side - 1 - i) for i in range(1, n_side - 1)]
    out.append(("closed_merge_seam", R.polyline(ring, closed=True), [7, 4], 3, 0, True))
    out.append(("offset_negative", stairs(20), [4, 3], -10, 0, True))
    out.append(("offset_huge", stairs(20), [4, 3], 7 * 10 ** 9 + 2, 0, True))
    out.append(("path_length", R.polyline([(0, 0), (64, 0), (64, 64)]), [8, 8], 4, 64, True))   # (scale 2: exact)
    out.append(("zero_dashes", stairs(20), [0, 3, 2, 1], 0, 0, True))
    out.append(("zero_segments", R.polyline([(0, 0), (0, 0), (10, 0), (10, 0), (10, 10), (10, 10)]), [3, 2], 0, 0, True))
    out.append(("inflection", R.from_segments([(R.CUBIC, [0, 0, 60, 90, 30, -70, 100, 10])]), [9.3, 4.1], 1.7, 0, False))
    out.append(("loop", R.from_segments([(R.CUBIC, [0, 0, 120, 80, -20, 80, 100, 0])]), [11.7, 3.9], 0.9, 0, False))
    out.append(("near_cusp", R.from_segments([(R.CUBIC, [0, 0, 100, 60.5, 0, 60, 100, 0])]), [8.9, 5.3], 2.1, 0, False))
    out.append(("all_zero_length", R.polyline([(5, 5), (5, 5), (5, 5)]), [3, 2], 0, 0, True))
    return out


def fuzz_cases(n_paths=200, seed=20260101):
    """Seeded: `n_paths` paths of <= 40 segments, lines and cubics, open and closed, one or two subpaths."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_paths):
        parts = []
        for _ in range(int(rng.integers(1, 3))):
            n = int(rng.integers(1, 21))
            segs = mixed_chain(n, int(rng.integers(1 << 30)))
            parts.append(R.from_segments(segs, closed=bool(rng.random() < 0.4)))
        path = R.concat(*parts)
        L = _length(path)
        m = int(rng.integers(1, 6))
        dashes = list(rng.uniform(0.01, 0.2, m) * L)
        out.append((f"fuzz{i}", path, dashes, float(rng.uniform(-1, 2) * L * 0.1), 0, False))
    return out
