"""The gradient edge cases (tests/grad_cases.py) on the host: the case list does what it claims -- offsets exact in binary64,
pixels exactly on stops, the focal form's flag hanging on one pixel --, the numpy restatement of Grad*.fill
(oracle.gradient_points) answers every recorded points case as the reference did, and the stops memo of paint.py hands over
the stops as they are now."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from tests import grad_cases as gc
from tests.util import assert_close64, load, meta


@pytest.fixture(scope="module")
def fixture():
    z = load("gradedge_kat.npz")
    return z, meta(z)


def _stops_in(case, linear_rgb):
    """The case's stops in the target colour space (grad_stops_colorspace, S:1686-1695): offsets, colours."""
    stops = gc.stops_at(case["stops"])
    return np.array([o for o, _ in stops]), np.array([orc.paint_for_fill(c, linear_rgb) for _, c in stops])


def test_the_case_list_and_the_fixture_agree(fixture):
    _z, m = fixture
    assert [p["name"] for p in m["points"]] == [c["name"] for c in gc.POINT_CASES]
    assert [g["name"] for g in m["grid"]] == [c["name"] for c in gc.GRID_CASES]
    for c, rec in zip(gc.POINT_CASES + gc.GRID_CASES, m["points"] + m["grid"]):
        assert gc.digest(c) == rec["digest"], c["name"]
    assert len({c["name"] for c in gc.POINT_CASES + gc.GRID_CASES}) == len(gc.POINT_CASES) + len(gc.GRID_CASES)
    z = fixture[0]
    n = sum(p["n"] for p in m["points"])
    assert z["points_lin"].shape == z["points_srgb"].shape == (n, 4)
    assert all(p["n"] == len(c["pts"]) <= 400 for p, c in zip(m["points"], gc.POINT_CASES))
    assert all(g["shape"][0] * g["shape"][1] < 20000 for g in m["grid"])
    for key in z.files:   # (every reference output is finite: nothing has to be left out of a comparison)
        if key != "meta":
            assert np.isfinite(z[key]).all(), key


def test_neighbouring_stop_colours_differ_in_every_channel():
    """... by 0.1 or more, alpha included, and premultiplied colours stay inside their alpha: a pixel on the wrong side of a
    stop comparison is wrong by 1e-1 against tolerances of 1e-11."""
    cols = np.array([gc.colour(k) for k in range(34)])
    assert (np.abs(np.diff(cols, axis=0)) >= 0.1).all()
    assert (cols[:, :3] <= cols[:, 3:]).all() and (cols > 0).all() and (cols <= 1).all()
    assert len({c.tobytes() for c in cols}) == len(cols)
    for c in gc.POINT_CASES + gc.GRID_CASES:
        assert 1 <= len(c["stops"]) <= len(cols)
    counts = {len(c["stops"]) for c in gc.POINT_CASES}
    assert {1, 2, 32, 33} <= counts


def test_the_restatement_equals_every_recorded_points_result(fixture):
    """oracle.gradient_points (numpy, the reference's operations by points) against the reference's Grad*.fill in both colour
    spaces.  The same numpy expressions on the same inputs; the stop colours come from the C restatement of the colour
    conversion, whose pow may differ from numpy's by an ulp of a value below 1: 1e-14 leaves room for a few of those."""
    z, m = fixture
    at, worst = 0, 0.0
    with np.errstate(all="ignore"):
        for c, rec in zip(gc.POINT_CASES, m["points"]):
            pts = np.array(c["pts"], dtype=np.float64)
            for lin, key in ((True, "points_lin"), (False, "points_srgb")):
                off, col = _stops_in(c, lin)
                got = orc.gradient_points(c["geom"]["kind"], pts, c["spread"], off, col, **gc.geom_kwargs(c["geom"]))
                want = z[key][at:at + rec["n"]]
                worst = max(worst, float(np.abs(got - want).max()))
                assert_close64(got, want, atol=1e-14, what=f"{c['name']} linear_rgb={lin}")
            at += rec["n"]
    print(f"restatement vs reference, points: worst {worst:.3e}")


def test_the_offsets_of_the_points_cases_are_exact():
    """The float offset of every finite point (before the spread) IS its value in rational arithmetic, square roots included:
    no rounding happened on the way, so none can differ between the reference's numpy and the device's fma forms.  Points with
    det < 0 are the masked ones.  Every stop of a case's list is hit exactly, and so are both of its ulp neighbours where the
    geometry can carry them."""
    checked = 0
    with np.errstate(all="ignore"):
        for c in gc.POINT_CASES:
            if not c["exact"]:
                continue
            pts = np.array(c["pts"], dtype=np.float64)
            off, mask = orc.gradient_offsets(c["geom"]["kind"], pts, **gc.geom_kwargs(c["geom"]))
            finite = np.isfinite(pts).all(axis=1)
            for i in np.flatnonzero(finite):
                want = gc.exact_offset(c["geom"], pts[i, 0], pts[i, 1])
                if want is None:
                    assert mask is not None and not mask[i], (c["name"], i)
                    continue
                assert math.isfinite(off[i]) and Fraction(float(off[i])) == want, (c["name"], i, pts[i], off[i], want)
                checked += 1
            hit = set(off[finite].tolist())
            name = c["name"].split("-")[0]
            if name in gc.GEOMS:
                probed = set(c["stops"]) if len(c["stops"]) <= 8 else set(c["stops"][-2:])   # (n - 2 and n - 1 of the long lists)
                if name == "conc":   # (its points 4 o + 2 are exact for the dyadic stops only: 0.8 is left to the other forms)
                    probed = {s for s in probed if Fraction(s).denominator <= 32}
                assert probed <= hit, (c["name"], sorted(probed - hit))
                assert (~finite).sum() >= 6   # (and the non-finite coordinates ride along)
                if name != "conc":
                    for s in probed:
                        above = gc.RADIAL_FLOOR if s == 0.0 and name == "rad4" else float(np.nextafter(s, np.inf))
                        assert above in hit, (c["name"], s)
                        assert s == 0.0 and name == "rad4" or float(np.nextafter(s, -np.inf)) in hit, (c["name"], s)
    assert checked > 3000


def test_the_focal_probe_has_its_zero_determinant():
    """c = (0, 0), r = 3, f = (5, 0), fr = 0: det = 9 pdx^2 - 16 pdy^2 is exactly 0 at (1, 3), where the offset is 1.25 -- a stop
    -- positive at (0, 3) and negative at (1, 3.5); the points beyond the focus have offsets at or below the threshold 0."""
    kw = gc.geom_kwargs(gc._FOCAL)
    pts = np.array(gc._FOCAL_SAFE + [gc._FOCAL_NEG])
    pd = pts - kw["fcenter"]
    det = 9 * pd[:, 0] ** 2 - 16 * pd[:, 1] ** 2
    assert det[0] == 0.0 and det[1] == 0.0 and det[2] == 81.0 and det[-1] < 0 and (det[:-1] >= 0).all()
    off, mask = orc.gradient_offsets("radial", pts[:-1], **kw)
    assert mask is None and off[0] == 1.25 and 1.25 in gc._FOCAL_STOPS and (off[-3:] <= 0).all() and (off[:-3] > 0).all()
    off, mask = orc.gradient_offsets("radial", pts, **kw)
    assert mask.tolist() == [True] * 6 + [False] * 4
    # fr == r: the mask exists, but no offset is excluded (S:1642)
    off, mask = orc.gradient_offsets("radial", np.array(gc._FOCAL_EQ_PTS), **gc.geom_kwargs(gc._FOCAL_EQ))
    assert off[0] == -0.25 and mask.tolist() == [True] * 6 + [False]


def _grid_offsets(c, rec):
    bbox = rec["offset"] + rec["shape"]
    px = gc.pixel_centres(c["tr"], bbox)
    return px, orc.gradient_offsets(c["geom"]["kind"], px, **gc.geom_kwargs(c["geom"]))


def test_pixel_centres_are_what_the_inverse_transform_gives(fixture):
    """The axis swap and the swap scaled by 2 with a dyadic translation have exact inverses: user_tr(grad_pixels(bbox))
    (S:1027, S:1653-1658) is the dyadic arithmetic of grad_cases.pixel_centres, bit for bit."""
    import svgrasterize_amd as S

    _z, m = fixture
    for c, rec in zip(gc.GRID_CASES, m["grid"]):
        r0, c0, rows, cols = rec["offset"] + rec["shape"]
        xs, ys = np.indices((rows, cols)).astype(np.float64)
        dev = np.concatenate([xs[..., None], ys[..., None]], axis=2) + [r0 + 0.5, c0 + 0.5]
        got = gc.make_transform(S, c["tr"]).invert(dev)
        assert np.array_equal(got, gc.pixel_centres(c["tr"], (r0, c0, rows, cols))), c["name"]


def test_the_flag_layers_hang_on_one_pixel(fixture):
    """Three layers of one two-circle gradient: exactly one pixel with det < 0, the first of its layer; exactly one, the last
    of a layer of more than 64 * 256 pixels and more than 256 columns; none.  The determinants are far from zero (so their signs
    are no matter of rounding), and every layer has painted pixels at or below the exclusion threshold: the flag decides about
    pixels far from the one that sets it."""
    z, m = fixture
    flags = [(i, c) for i, c in enumerate(gc.GRID_CASES) if "detneg" in c]
    assert [c["detneg"] for _i, c in flags] == [[0], [40 * 420 - 1], []]
    for i, c in flags:
        rec = m["grid"][i]
        px = gc.pixel_centres(c["tr"], rec["offset"] + rec["shape"])
        kw = gc.geom_kwargs(c["geom"])
        cd, pd, rd = kw["center"] - kw["fcenter"], px - kw["fcenter"], kw["radius"]
        a = (cd ** 2).sum() - rd ** 2
        assert a == 0.125
        b = (pd * cd).sum(axis=-1)
        det = (b * b - a * (pd ** 2).sum(axis=-1)).ravel()
        assert np.flatnonzero(det < 0).tolist() == c["detneg"], c["name"]
        assert (np.abs(det) > 1.0).all()
        off, mask = orc.gradient_offsets("radial", px, **kw)
        image = z[f"g{i}_image"]
        below = (off <= 0.0) & (det.reshape(off.shape) >= 0)
        assert below.sum() >= 7
        if c["detneg"]:
            assert (image[below] == 0).all() and (image[..., 3] > 0).sum() >= 7
        else:
            assert mask is None and (image[:-1][below[:-1]][:, 3] > 0).all()   # (the last row is the layer's unpainted margin)
    rec = m["grid"][flags[1][0]]
    assert rec["shape"] == [40, 420] and rec["shape"][0] * rec["shape"][1] > 64 * 256 and rec["shape"][1] > 256


def test_every_pixel_grid_case_has_pixels_on_a_stop_and_on_both_sides(fixture):
    """Among the painted pixels of every linear and radial layer: one whose offset (after the spread) IS a stop, one below that
    stop and one above it.  For the linear cases the offsets are (col - col0) / 64 or / 16 exactly; for the radial ones the centre
    row, the centre column and the (3, 4) pixels are on stops.  (The three flag layers are about the determinant, not the stops.)"""
    z, m = fixture
    seen = 0
    for i, (c, rec) in enumerate(zip(gc.GRID_CASES, m["grid"])):
        if "detneg" in c:
            continue
        px, (off, mask) = _grid_offsets(c, rec)
        assert mask is None
        off = orc.gradient_spread(off, c["spread"])
        painted = z[f"g{i}_image"][..., 3] > 0
        assert painted.sum() > 0.5 * painted.size
        o = off[painted]
        on = [s for s in set(c["stops"]) if (o == s).any() and (o < s).any() and (o > s).any()]
        assert on, c["name"]
        if c["geom"]["kind"] == "linear":
            period = 64 if "64" in c["name"] or c["name"].startswith("n3") else 16
            assert np.array_equal(off * period, np.round(off * period)), c["name"]   # every offset a multiple of 1 / period
            if c["spread"] == "pad":
                assert len(on) == len(set(c["stops"])), c["name"]                  # every stop has its pixel
        else:
            cy, cx = np.argwhere((px == c["geom"]["center"]).all(axis=-1))[0]
            raw = orc.gradient_offsets("radial", px, **gc.geom_kwargs(c["geom"]))[0]
            assert raw[cy, cx] == 0 and raw[cy + 3, cx + 4] == 1.25 and raw[cy, cx + 2] == 0.5 and raw[cy - 1, cx] == 0.25
        seen += 1
    assert seen == 8


def test_repeat_and_reflect_layers_cross_every_integer_offset(fixture):
    _z, m = fixture
    for c, rec in zip(gc.GRID_CASES, m["grid"]):
        if c["name"].startswith("lin16"):
            _px, (off, _mask) = _grid_offsets(c, rec)
            want = {-2.0, -1.0, 0.0, 1.0, 2.0, 3.0} if "cut" not in c["name"] else {-1.0, 0.0, 1.0, 2.0}
            assert want <= set(off.ravel().tolist()), c["name"]


def test_which_leaves_the_case_list_expects_in_the_batch():
    assert [c["name"] for c in gc.GRID_CASES if not c.get("batched", True)] == ["n33"]
    assert len(gc.STOP_LISTS["n32"]) == 32 and len(gc.STOP_LISTS["n33"]) == 33


# ------------------------------------------------------------------------------------------ the stops memo
def _handed_over(g):
    n = g.n_stops
    return (np.array((C.c_double * n).from_address(g.stop_off)), np.array((C.c_double * (4 * n)).from_address(g.stop_rgba)).reshape(n, 4))


@pytest.mark.parametrize("linear_rgb", [True, False])
def test_stops_edited_in_place_reach_the_abi(linear_rgb):
    """The reference keeps nothing between fills: after an entry of the stops list is replaced in place, and after a stop's
    colour array is written in place, `paint.abi` hands over the new offsets and colours (needs no device)."""
    import svgrasterize_amd as S
    from svgrasterize_amd.geometry import solid_paint

    def want(stops):
        return np.array([o for o, _ in stops]), np.array([solid_paint(np.array(c), linear_rgb) for _, c in stops])

    stops = gc.stops_at([0.0, 0.5, 1.0])
    for paint in (S.GradLinear(np.array([0.0, 0.0]), np.array([1.0, 0.0]), stops, None, "pad", False, None),
                  S.GradRadial(np.array([0.0, 0.0]), 4.0, None, None, stops, None, "pad", False, None)):
        g, keep = paint.abi(S.Transform(), linear_rgb)
        for got, exp in zip(_handed_over(g), want(stops)):
            assert np.array_equal(got, exp)
        stops[1] = (0.25, gc.colour(5))                   # an entry replaced in place
        g, keep = paint.abi(S.Transform(), linear_rgb)
        off, col = _handed_over(g)
        assert off.tolist() == [0.0, 0.25, 1.0]
        assert np.array_equal(col, want(stops)[1])
        stops[0][1][:] = gc.colour(7)                     # a colour array written in place
        g, keep = paint.abi(S.Transform(), linear_rgb)
        assert np.array_equal(_handed_over(g)[1], want(stops)[1]) and np.array_equal(_handed_over(g)[1][0], want([(0.0, gc.colour(7))])[1][0])
        stops.append((1.5, gc.colour(9)))                 # an entry more
        g, keep = paint.abi(S.Transform(), linear_rgb)
        assert g.n_stops == 4 and _handed_over(g)[0].tolist() == [0.0, 0.25, 1.0, 1.5]
        # and the same contents again: the same arrays (the memo still is one)
        g2, keep2 = paint.abi(S.Transform(), linear_rgb)
        assert g2.stop_off == g.stop_off and g2.stop_rgba == g.stop_rgba
        del stops[3]
        stops[1] = (0.5, gc.colour(1))
        stops[0][1][:] = gc.colour(0)
        del keep, keep2
