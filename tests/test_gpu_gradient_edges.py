"""The gradient paint servers at their value edges, on the GPU, on every route: `grad_colour_user` (stops, spread, the
focal form's mask) as `k_gradient_fill` runs it on a caller's points and on a fill's pixel grid, and as the tile kernel's
gradient variant runs it inside a batch; `k_gradient_detneg` / `k_grad_detneg`, whose one flag decides about a whole layer.
The cases are tests/grad_cases.py (every finite offset exact in binary64, neighbouring stops 0.1 or more apart in every
channel), the expected values the reference's own (tests/golden/gradedge_kat.npz, gen_golden.py --only gradedge).  Tolerances
as in test_gpu_gradient_fills / test_gpu_gradients_with_many_stops / test_gradient_fills_inside_the_batch_...: 1e-13 by
points, 1e-11 and the float32 contract for a fill, 1e-12 between the two routes of this package."""
import copy

import numpy as np
import pytest

from tests import grad_cases as gc
from tests.util import assert_close64, assert_f32_1ulp, load, meta

pytestmark = pytest.mark.gpu

TOL_POINTS, TOL_FILL, TOL_ROUTES = 1e-13, 1e-11, 1e-12
WORST = {}   # route -> worst absolute error seen (all asserted where they were measured)


def _close(route, got, want, atol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape == want.shape:
        err = np.abs(got - want).max(initial=0.0)
        WORST[route] = max(WORST.get(route, 0.0), float(err) if np.isfinite(err) else float("inf"))
    assert_close64(got, want, atol=atol, what=what)


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def fixture():
    z = load("gradedge_kat.npz")
    m = meta(z)
    assert [p["name"] for p in m["points"]] == [c["name"] for c in gc.POINT_CASES]
    assert [g["name"] for g in m["grid"]] == [c["name"] for c in gc.GRID_CASES]
    starts = np.concatenate([[0], np.cumsum([p["n"] for p in m["points"]])])
    return z, m, starts


def _paint(S, c, stops=None):
    return gc.make_paint(S, c["geom"], gc.stops_at(c["stops"]) if stops is None else stops, c["spread"])


@pytest.fixture(scope="module")
def per_node(S):
    """Path.fill of every pixel-grid case (k_gradient_detneg + k_gradient_fill with the path's mask), drawn once."""
    out = []
    for c in gc.GRID_CASES:
        layer, _hull = S.Path.from_svg(c["path"]).fill(gc.make_transform(S, c["tr"]), _paint(S, c), viewport=c["viewport"],
                                                       linear_rgb=c["linear_rgb"])
        out.append((tuple(int(v) for v in layer.offset), bool(layer.linear_rgb), bool(layer.pre_alpha), np.array(layer.image)))
    return out


# ------------------------------------------------------------------------------------------ points route
@pytest.mark.parametrize("i", range(len(gc.POINT_CASES)), ids=[c["name"] for c in gc.POINT_CASES])
def test_gradient_at_points_equals_the_reference(S, fixture, i):
    """Grad*.fill on the caller's points (svgr_gradient_eval -> k_gradient_fill with `pts`), both colour spaces."""
    z, _m, starts = fixture
    c = gc.POINT_CASES[i]
    pts = np.array(c["pts"], dtype=np.float64)
    paint = _paint(S, c)
    for lin, key in ((True, "points_lin"), (False, "points_srgb")):
        want = z[key][starts[i]:starts[i + 1]]
        got = paint.fill(pts, linear_rgb=lin)
        bad = np.flatnonzero(~(np.abs(got - want).max(axis=1) <= TOL_POINTS))
        _close("points", got, want, TOL_POINTS, f"{c['name']} linear_rgb={lin}: points {bad[:8].tolist()} = {pts[bad[:8]].tolist()}")


# ------------------------------------------------------------------------------------------ pixel-grid routes
_GRID_IDS = [c["name"] for c in gc.GRID_CASES]


@pytest.mark.parametrize("i", range(len(gc.GRID_CASES)), ids=_GRID_IDS)
def test_per_node_fill_equals_the_reference(fixture, per_node, i):
    z, m, _starts = fixture
    rec, (offset, linear_rgb, pre_alpha, image) = m["grid"][i], per_node[i]
    assert list(offset) == rec["offset"] and list(image.shape[:2]) == rec["shape"]
    assert linear_rgb == rec["linear_rgb"] and pre_alpha
    want = z[f"g{i}_image"]
    _close("per node", image, want, TOL_FILL, f"{rec['name']} per node")
    assert_f32_1ulp(image.astype(np.float32), want, what=f"{rec['name']} per node")
    assert np.abs(want).max() > 0.2


@pytest.mark.parametrize("i", range(len(gc.GRID_CASES)), ids=_GRID_IDS)
def test_batched_fill_equals_the_reference_and_the_per_node_route(S, fixture, per_node, monkeypatch, i):
    """The same leaf in a group with a solid leaf that shares no pixel with it (a group of one leaf is drawn node by node): a
    batch entry (k_grad_detneg + the tile kernel's gradient variant) -- but for 33 stops, which the batch declines, so that the
    group draws it node by node.  Against the two recorded fills side by side, and against Path.fill."""
    from svgrasterize_amd import paint as paint_mod
    from svgrasterize_amd import scene as sc

    z, m, _starts = fixture
    c, rec = gc.GRID_CASES[i], m["grid"][i]
    tr = gc.make_transform(S, c["tr"])
    doc = S.Scene.group([S.Scene.fill(S.Path.from_svg(c["path"]), _paint(S, c)),
                         S.Scene.fill(S.Path.from_svg(c["solid"]), np.array(gc.SOLID_PAINT))])
    per_node_fills = []
    monkeypatch.setattr(sc, "_BATCH_GRADS", True)
    monkeypatch.setattr(paint_mod, "gradient_fill", lambda *a, _f=paint_mod.gradient_fill: per_node_fills.append(1) or _f(*a))
    leaves = sc._batchable_leaves(doc, tr, c["linear_rgb"])
    assert (leaves is not None) == c.get("batched", True)
    assert leaves is None or (len(leaves) == 2 and leaves[0][6] is not None and leaves[1][6] is None)
    layer, _hull = doc.render(tr, viewport=c["viewport"], linear_rgb=c["linear_rgb"])
    assert len(per_node_fills) == (0 if c.get("batched", True) else 1)   # (the batch drew it, not Path.fill behind the scenes)
    image = np.array(layer.image)
    # the expected layer of the group: the two recorded fills, which share no pixel, over the union of their boxes
    grad, solid = z[f"g{i}_image"], z[f"s{i}_image"]
    (gr, gcol), (sr, scol) = rec["offset"], rec["solid_offset"]
    r0, c0 = min(gr, sr), min(gcol, scol)
    r1, c1 = max(gr + grad.shape[0], sr + solid.shape[0]), max(gcol + grad.shape[1], scol + solid.shape[1])
    want = np.zeros((r1 - r0, c1 - c0, 4))
    want[gr - r0:gr - r0 + grad.shape[0], gcol - c0:gcol - c0 + grad.shape[1]] = grad
    want[sr - r0:sr - r0 + solid.shape[0], scol - c0:scol - c0 + solid.shape[1]] = solid
    assert [int(v) for v in layer.offset] == [r0, c0] and image.shape == want.shape
    assert bool(layer.linear_rgb) == rec["linear_rgb"] and layer.pre_alpha
    _close("batched", image, want, TOL_FILL, f"{rec['name']} batched")
    _close("batched vs per node", image[gr - r0:gr - r0 + grad.shape[0], gcol - c0:gcol - c0 + grad.shape[1]], per_node[i][3], TOL_ROUTES,
           f"{rec['name']} batched vs per node")


def test_the_flag_of_the_focal_form_decides_about_the_whole_layer(fixture, per_node):
    """What the three flag layers are for, said on the pictures themselves: with one pixel of det < 0 -- the first of the
    layer, or the last of 16 800 -- every pixel of negative r(t) is transparent; without one, they all keep the first stop's colour."""
    _z, m, _starts = fixture
    by_name = {rec["name"]: per_node[i][3] for i, rec in enumerate(m["grid"])}
    # (flag-first and flag-none end, flag-last begins with the unpainted margin row of the path's layer)
    assert (by_name["flag-first"][1:, 0, 3] == 0).all() and (by_name["flag-first"][1:-1, 1:, 3] > 0).all()
    assert (by_name["flag-last"][:, :-1, 3] == 0).all() and (by_name["flag-last"][1:-1, -1, 3] > 0).all()
    assert by_name["flag-last"][-1, -1, 3] == 0
    assert (by_name["flag-none"][:-1, :, 3] > 0).all()


# ------------------------------------------------------------------------------------------ stops edited in place
def test_a_second_fill_after_the_stops_were_edited_in_place(S, monkeypatch):
    """The reference keeps nothing between fills (S:1671-1695 converts the stops every time): after an entry of the stops list
    is replaced and a colour array is written in place, the same paint object draws the new stops -- by points, per node and as a
    batch entry -- exactly as a fresh gradient with those stops does."""
    from svgrasterize_amd import paint as paint_mod

    c = gc.GRID_CASES[0]
    tr, path, pts = gc.make_transform(S, c["tr"]), S.Path.from_svg(c["path"]), np.array([[10.5 + 4 * k, 3.0] for k in range(-2, 20)])
    stops = gc.stops_at([0.0, 0.5, 1.0])
    paint = _paint(S, c, stops)
    solid = S.Scene.fill(S.Path.from_svg(c["solid"]), np.array(gc.SOLID_PAINT))
    doc = S.Scene.group([S.Scene.fill(path, paint), solid])
    per_node_fills = []
    monkeypatch.setattr(paint_mod, "gradient_fill", lambda *a, _f=paint_mod.gradient_fill: per_node_fills.append(1) or _f(*a))

    def draw(paint, doc):
        out = [np.array(paint.fill(pts, linear_rgb=lin)) for lin in (True, False)]
        out += [np.array(path.fill(tr, paint, viewport=c["viewport"], linear_rgb=lin)[0].image) for lin in (True, False)]
        before = len(per_node_fills)
        out += [np.array(doc.render(tr, viewport=c["viewport"], linear_rgb=lin)[0].image) for lin in (True, False)]
        assert len(per_node_fills) == before   # (the group was drawn as a batch)
        return out

    first = draw(paint, doc)
    stops[1] = (0.25, gc.colour(5))
    stops[0][1][:] = gc.colour(7)
    second = draw(paint, doc)
    fresh_paint = _paint(S, c, copy.deepcopy(stops))
    fresh = draw(fresh_paint, S.Scene.group([S.Scene.fill(path, fresh_paint), solid]))
    for k, (a, b, old) in enumerate(zip(second, fresh, first)):
        assert np.array_equal(a, b), f"route {k}: the edited stops were not drawn"
        assert np.abs(a - old).max() > 0.05


def test_zz_the_worst_error_of_every_route():
    """(a report, printed last: the worst error of every route this process ran; every one of them was asserted above)"""
    for route, w in WORST.items():
        print(f"worst error [{route}]: {w:.3e}")
    tol = {"points": TOL_POINTS, "per node": TOL_FILL, "batched": TOL_FILL, "batched vs per node": TOL_ROUTES}
    assert all(w <= tol[route] for route, w in WORST.items())
