"""The marker pass's test inputs, shared by tests/test_marker_host.py (the per-lane header on the CPU) and
tests/test_gpu_markers.py (svgr_path_markers through the C ABI).  A case is (name, (types, params, sizes), seg_vertex or None).
The shapes sit at the seams of the launch geometry: B segments per workgroup of the classify / table / emit kernels, S per
workgroup of the scans (the GPU test checks both values against the library)."""
import numpy as np

from tests import dash_cases as D
from tests import marker_ref as R

B = 256    # svgr_marker_block_segments
S = 1024   # svgr_dash_scan_segments


def raw(segments, end=None):
    """(types, params, sizes) of one subpath of [(type, numbers)], with a terminating line of type `end` (None: none)."""
    types = [t for t, _q in segments]
    params = [list(map(float, q)) + [0.0] * (8 - len(q)) for _t, q in segments]
    if end is not None:
        first, last = params[0], params[-1]
        e = (last[6], last[7]) if types[-1] == R.CUBIC else (last[2], last[3])
        types.append(end)
        params.append([e[0], e[1], first[0], first[1], 0, 0, 0, 0])
    return types, params, [len(types)]


def lines(points):
    return [(R.LINE, [*a, *b]) for a, b in zip(points, points[1:])]


def stair_points(n, x=0, y=0):
    """n + 1 points of a staircase with steps of integer lengths 1..5."""
    pts = [(x, y)]
    for i in range(n):
        step = 1 + (i * 7 + 3) % 5
        x, y = (x + step, y) if i % 2 == 0 else (x, y + step)
        pts.append((x, y))
    return pts


def with_repeats(points, start, count):
    """`points` with point `start` repeated `count` more times: `count` zero-length segments that begin at segment `start`."""
    return points[:start + 1] + [points[start]] * count + points[start + 1:]


def by_count(n, what):
    """A path of exactly n segments: "stairs" n lines, no terminator; "cubics" n - 1 cubics and an UNCLOSED line; "mix" n - 1 lines and
    cubics and a CLOSED line (n = 1: the lone segment)."""
    if what == "stairs":
        return raw(lines(stair_points(n)))
    segs = D.cubic_chain(max(n - 1, 1), n) if what == "cubics" else D.mixed_chain(max(n - 1, 1), n)
    return raw(segs, None if n == 1 else (R.UNCLOSED if what == "cubics" else R.CLOSED))


def fixed_cases():
    out = []
    for n in (1, 2, B - 1, B, B + 1, S - 1, S, S + 1, 2 * S + 1):
        for what in ("stairs", "cubics", "mix"):
            out.append((f"{what}{n}", by_count(n, what), None))
    for name, seam in (("B", B), ("S", S)):
        # zero-length segments seam - 6 .. seam + 5 inside one subpath: those behind the seam look backwards across it
        out.append((f"degenerate_run_back_{name}", raw(lines(with_repeats(stair_points(seam + 20), seam - 6, 12)), R.UNCLOSED), None))
        # a subpath that begins at segment seam - 6 with 12 zero-length segments: those in front of the seam look forwards across it
        head = raw(lines(stair_points(seam - 6)))
        tail = raw(lines(with_repeats(stair_points(10, 3, 900), 0, 12)), R.CLOSED)
        out.append((f"degenerate_run_forward_{name}", R.concat(head, tail), None))
        # a subpath boundary exactly on the seam: the first subpath is closed and its closing line is segment seam - 1
        out.append((f"boundary_on_{name}", R.concat(raw(lines(stair_points(seam - 1)), R.CLOSED), raw(lines(stair_points(9, 7, 700)), R.UNCLOSED)), None))
        # a wholly degenerate subpath (segments seam - 3 .. seam + 2) between two ordinary ones: (1, 0), borrowed from neither
        dot = raw(lines([(50, 60)] * 7))
        out.append((f"degenerate_subpath_on_{name}", R.concat(raw(lines(stair_points(seam - 3))), dot, raw(lines(stair_points(10, 5, 800)))), None))
        # a closed subpath whose first segment is segment 3 and whose closing line is segment seam + 8
        ring = raw(lines(stair_points(seam + 5, 20, 20)), R.CLOSED)
        out.append((f"closed_across_{name}", R.concat(raw(lines(stair_points(3))), ring), None))
        # ... and one whose last point is its first: the closing line is degenerate and borrows backwards
        pts = stair_points(seam + 4, 20, 20)
        out.append((f"closed_degenerate_across_{name}", R.concat(raw(lines(stair_points(3))), raw(lines(pts + [pts[0]]), R.CLOSED)), None))
        # unflagged segments seam - 4 .. seam + 3, and every third segment elsewhere flagged, as arcs in three pieces are
        path = raw(D.cubic_chain(seam + 30, seam), R.UNCLOSED)
        flags = [1 if (i % 3 == 2 and not seam - 4 <= i < seam + 4) or i >= seam + 29 else 0 for i in range(seam + 31)]
        out.append((f"vertex_flags_across_{name}", path, flags))
    out.append(("tiny", raw(lines([(0, 0), (1e-170, 0), (1e-170, 1e-170), (3e-170, 2e-170)]), R.UNCLOSED), None))
    out.append(("huge", raw(lines([(-1e150, -1e150), (1e150, -1e150), (1e150, 1e150), (-0.5e150, 0.25e150)]), R.CLOSED), None))
    out.append(("tiny_and_huge_cubics", raw([(R.CUBIC, [0, 0, 1e-170, 0, 1e-170, 2e-170, 0, 3e-170]),
                                             (R.CUBIC, [0, 3e-170, 1e150, 1e150, -1e150, 1e150, 1e150, -1e150])], R.UNCLOSED), None))
    return out


def fuzz_cases(n_paths=200, seed=20260218):
    """Seeded: `n_paths` paths of one or two subpaths of <= 20 lines and cubics, open and closed, a third of them with runs of
    zero-length segments put in, a quarter with vertex flags."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_paths):
        parts = []
        for _ in range(int(rng.integers(1, 3))):
            segs = D.mixed_chain(int(rng.integers(1, 21)), int(rng.integers(1 << 30)))
            if rng.random() < 1 / 3:
                for _ in range(int(rng.integers(1, 4))):
                    k = int(rng.integers(0, len(segs) + 1))
                    q = segs[k][1] if k < len(segs) else None
                    p = q[:2] if q is not None else (segs[-1][1][6:8] if segs[-1][0] == R.CUBIC else segs[-1][1][2:4])
                    zero = (R.LINE, [*p, *p]) if rng.random() < 0.5 else (R.CUBIC, [*p, *p, *p, *p])
                    segs[k:k] = [zero] * int(rng.integers(1, 4))
            parts.append(raw(segs, R.CLOSED if rng.random() < 0.4 else R.UNCLOSED))
        path = R.concat(*parts)
        flags = None
        if rng.random() < 0.25:
            flags = [int(v) for v in rng.integers(0, 2, len(path[0]))]
        out.append((f"fuzz{i}", path, flags))
    return out
