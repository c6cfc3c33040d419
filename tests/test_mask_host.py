"""Luminance-masked groups in differentiable compositing on the host: csrc/svgr_mask.h compiled by g++ (tests/mask_harness.cpp)
against the oracle's layers, the numpy restatement (tests/mask_ref.py), the group harness for a program without masks, central
differences of every input, the one-sided points of the mask's value by value, and every refusal of the program's check and of
the numpy forms of svgrasterize_amd.diff (which refuse before any library call: no device is needed)."""
import numpy as np
import pytest

from tests import gradpaint_cases as G
from tests import group_cases as GK
from tests import mask_cases as K
from tests import mask_ref as R
from tests.mask_cases import grp

SUMS = ("paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,with_bg", K.ALL)
def test_forward_is_the_oracles_layers(name, with_bg):
    """Equal.  Only "mask_generic", whose transforms and geometry are not dyadic, is within 1e-13 as in test_group_host.py: the
    oracle's affine map and dot product are BLAS calls.  The restatement: equal everywhere."""
    c = K.case(name, with_bg)
    image = K.harness_forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"])
    want = K.oracle_image(c["cover"], c["paints"], c["gp"], c["tree"], c["bg"], c["origin"])
    if c["dyadic"]:
        assert np.array_equal(image, want), float(np.abs(image - want).max())
    else:
        assert np.abs(image - want).max() <= 1e-13, float(np.abs(image - want).max())
    assert np.array_equal(_bits(image), _bits(R.forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"])))


def _mask_canvases(c):
    parked = {}
    R.forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"], parked=parked)
    return parked


def test_the_cases_cover_what_they_claim():
    assert K.harness().mkh_depth() == R.DEPTH == GK.harness().grh_depth() == 4
    seen = {}
    for name in K.CASES:
        gr = K.case(name, False)["gr"]
        level = deepest = 0
        at = {}   # level of every HOLD and END_MASK
        for q, op in enumerate(gr.items[:, 0]):
            if op in (2, 3, 4):
                at[q] = level
            level += 1 if op == 1 else (-1 if op in (2, 3, 4) else 0)
            deepest = max(deepest, level)
        seen[name] = (deepest, int((gr.items[:, 0] == 3).sum()), len(gr.opacity), np.diff(gr.clip_off).tolist(), max(at.values()))
    assert seen["plain"] == (1, 1, 0, [], 1) and seen["opacity_clip"] == (1, 1, 1, [2], 1)
    assert seen["mask_in_mask"][:2] == (2, 2) and seen["pair_in_target"][:2] == (2, 2) and seen["depth4"] == (4, 1, 2, [], 4)
    assert K.case("mask_linear", False)["gp"].kind.tolist() == [0, 0, 1, 0] and K.case("mask_generic", False)["gp"].kind.tolist() == [0, 1, 0, 0, 1, 2]
    assert K.mask_planes(K.case("mask_linear", False)["tree"]) == [2] and K.mask_planes(K.case("mask_generic", False)["tree"]) == [4, 5]
    assert K.mask_planes(K.case("mask_in_mask", False)["tree"]) == [2, 3, 4] and K.mask_planes(K.case("pair_in_target", False)["tree"]) == [3, 5]
    assert K.case("empty_mask", False)["gr"].items[1:6, 0].tolist() == [1, 0, 3, 1, 4]
    assert K.case("empty_target", False)["gr"].items[1:6, 0].tolist() == [1, 3, 1, 0, 4]
    assert [n for n in K.CASES if not K.case(n, False)["dyadic"]] == ["mask_generic"]
    # no pixel on a kink: alpha away from the threshold, 0 and 1, every straight channel away from 0 and 1
    for name, with_bg in K.ALL:
        for q, M in _mask_canvases(K.case(name, with_bg)).items():
            if name in K.BY_VALUE:
                assert not M.any()
                continue
            al = M[..., 3]
            assert (np.abs(al - R.ALPHA_MIN) > 1e-6).all() and (al > R.ALPHA_MIN).all() and (al < 1 - 1e-6).all(), (name, q)
            x = M[..., :3] / al[..., None]
            assert (x > 1e-6).all() and (x < 1 - 1e-6).all(), (name, q)


@pytest.mark.parametrize("name,with_bg", GK.ALL)
def test_a_program_without_masks_is_the_grouped_composition(name, with_bg):
    c = GK.case(name, with_bg)
    want = GK.harness_forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"])
    assert np.array_equal(_bits(K.harness_forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"])), _bits(want))
    want_cover, want_sums = GK.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    grad_cover, sums = K.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    assert np.array_equal(_bits(grad_cover), _bits(want_cover))
    for k in SUMS:
        assert np.array_equal(_bits(sums[k]), _bits(want_sums[k])), k
    # and the check gives the same device form
    msg, dev, n_clips, n_pairs, last = K.harness_check(c["gr"], len(c["cover"]))
    want_msg, want_dev, want_clips = GK.harness_check(c["gr"], len(c["cover"]))
    assert msg is None and want_msg is None and np.array_equal(dev, want_dev) and n_clips == want_clips and (n_pairs, last) == (0, -1)


@pytest.mark.parametrize("name,with_bg", K.ALL)
def test_backward_is_the_restatement(name, with_bg):
    c = K.case(name, with_bg)
    grad_cover, sums = K.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    ref_cover, ref_sums, tol = R.backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    assert np.array_equal(_bits(grad_cover), _bits(ref_cover)), float(np.abs(grad_cover - ref_cover).max())
    for k in SUMS:
        err = np.abs(sums[k] - ref_sums[k])
        assert (err <= tol[k]).all(), f"{k}: off by {err.max():.3e}"
    clip = c["gr"].clip_planes
    assert not sums["paints"][clip].any() and not sums["m6"][clip].any() and not sums["geom"][clip].any()
    assert np.isfinite(grad_cover).all() and all(np.isfinite(v).all() for v in sums.values())


@pytest.mark.parametrize("name,with_bg", K.ALL)
def test_backward_is_the_derivative(name, with_bg):
    c = K.case(name, with_bg)
    grad_cover, sums = K.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    fd, tol = K.central_differences(c)
    got = dict(sums, cover=grad_cover)
    worst = 0.0
    for k in K.NAMES:
        assert got[k].shape == fd[k].shape, k
        if not got[k].size:
            continue
        err = np.abs(got[k] - fd[k])
        worst = max(worst, float((err / tol[k]).max()))
        assert (err <= tol[k]).all(), f"{k}: off by {err.max():.3e}, {float((err / tol[k]).max()):.3f} of the tolerance"
    print(f"{name} bg={with_bg}: worst error {worst:.3f} of the tolerance")


def test_gradients_reach_the_masks_paints_geometry_stops_planes_and_the_targets_opacity():
    c = K.case("mask_generic", True)   # target 1 (linear), 2; clip 3; mask 4 (linear), 5 (radial)
    grad_cover, sums = K.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    off = c["gp"].path_stop_off
    for p in (4, 5):
        assert np.abs(grad_cover[p]).max() > 1e-3                                # the mask's planes
        assert np.abs(sums["paints"][p][:3]).min() > 1e-4                        # its paints
        assert np.abs(sums["m6"][p]).max() > 1e-4 and np.abs(sums["geom"][p][:3]).min() > 1e-5   # its gradient's geometry
        assert np.abs(sums["stop_pos"][off[p]:off[p + 1]]).max() > 1e-4 and np.abs(sums["stop_rgba"][off[p]:off[p + 1]]).max() > 1e-4
    # (k = sum w_c M_c where nothing clips: the alpha of the mask's BOTTOM fill does not enter, that of the fill over it does)
    assert abs(sums["paints"][4][3]) < 1e-12 and abs(sums["paints"][5][3]) > 1e-4
    assert np.abs(sums["opacity"]).min() > 1e-3                                  # the target's opacity
    assert np.abs(grad_cover[3]).max() > 1e-3                                    # the clip under a mask
    c = K.case("plain", False)
    grad_cover, sums = K.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    assert np.abs(grad_cover[3]).max() > 1e-3 and np.abs(sums["paints"][3][:3]).min() > 1e-4


# ------------------------------------------------------------------------------------------------ one-sided points by value
W = np.array(R.W)


def _value(M):
    """(k, dk/dM) of the header, checked against the restatement bit for bit."""
    k, d = K.harness_value(M)
    M = np.asarray(M, dtype=np.float64)
    assert _bits(k) == _bits(R.mask_value(M)) and np.array_equal(_bits(d), _bits(R.mask_value_vjp(M)))
    assert np.isfinite(k) and np.isfinite(d).all()
    return k, d


def test_a_mask_canvas_of_zero():
    k, d = _value([0.0, 0.0, 0.0, 0.0])
    assert k == 0.0 and not d.any()


def test_opaque_white_passes_the_gradient_at_the_closed_ends():
    k, d = _value([1.0, 1.0, 1.0, 1.0])
    lum = R.mask_value(np.array([1.0, 1.0, 1.0, 1.0]))
    assert k == lum and abs(k - 0.9999) <= 2.0 ** -52   # (the renderer's three coefficients add up to 0.9999, not to 1)
    assert np.array_equal(d[:3], W)                       # x = 1 is inside the closed interval: the paint still moves
    assert abs(d[3] - (lum - W.sum())) <= 2.0 ** -52      # alpha = 1 too: lum - sum w x
    k, d = _value([1.0, 1.0, 1.0, 1.0 + 2.0 ** -40])      # just beyond: the alpha's clip is flat, the channels are inside
    assert d[3] < 0 and abs(d[3] + W.sum()) < 1e-9


def test_alpha_at_the_threshold_takes_the_forwards_branch():
    al = 0.0001
    M = np.array([0.5 * al, 0.25 * al, 0.75 * al, al])
    k, d = _value(M)                                      # not above the threshold: nothing is divided, x_c = M_c
    assert k == R.mask_value(M) and np.array_equal(d[:3], W * al)
    x = M[:3]
    assert abs(k - float((W * x).sum()) * al) <= 1e-20 and abs(d[3] - float((W * x).sum())) <= 1e-20
    up = np.nextafter(al, 1.0)
    M = np.array([0.5 * up, 0.25 * up, 0.75 * up, up])
    k, d = _value(M)                                      # the next double: divided
    assert abs(k - float((W * np.array([0.5, 0.25, 0.75])).sum()) * up) <= 1e-18
    assert np.allclose(d[:3], W, rtol=1e-12) and abs(d[3]) <= 1e-12   # k = sum w M_c here: no dependence on alpha


def test_a_channel_that_clips():
    M = np.array([0.6, 0.2, 0.1, 0.5])                    # M_0 > alpha: x_0 = 1.2 clips to 1
    k, d = _value(M)
    assert d[0] == 0.0 and d[1] > 0 and d[2] > 0
    want = (W[0] * 1.0 + W[1] * 0.4 + W[2] * 0.2) * 0.5
    assert abs(k - want) <= 1e-15
    assert abs(d[3] - W[0]) <= 1e-15                       # k = w_0 al + w_1 M_1 + w_2 M_2 here
    M = np.array([-0.1, 0.2, 0.1, 0.5])                   # and below 0
    k, d = _value(M)
    assert d[0] == 0.0 and abs(k - (W[1] * 0.4 + W[2] * 0.2) * 0.5) <= 1e-15


def test_a_mask_of_zero_under_a_non_empty_target():
    """k = 0 from a BLACK mask (x = 0, alpha > 0): the image is the backdrop, nothing reaches the target, and the mask's paint
    still has a gradient: x_c = 0 is inside the closed interval.  (A mask canvas of 0 has no first-order term at all: below the
    alpha threshold k = lum(M) M_3 is of second order in M, test_a_mask_canvas_of_zero.)"""
    rng = np.random.default_rng(201)
    cover, paints, g = GK.M.random_planes(rng, 4, 5, 7), GK.M.random_paints(rng, 4), rng.standard_normal((5, 7, 4))
    cover[1], cover[2] = rng.uniform(0.2, 0.9, (5, 7)), rng.uniform(0.2, 0.9, (5, 7))
    paints[2] = (0.0, 0.0, 0.0, 0.8)
    gp = G.make_gp([None] * 4)
    tree = [0, grp([1], opacity=0.7, mask=[2]), 3]
    gr = K.program(tree)
    image = K.harness_forward(cover, paints, gp, gr, K.BG)
    without = GK.harness_forward(np.ascontiguousarray(cover[[0, 3]]), paints[[0, 3]], G.make_gp([None] * 2), GK.program([0, 1]), K.BG)
    assert np.array_equal(image, without)
    grad_cover, sums = K.harness_backward(cover, paints, gp, gr, g, K.BG)
    ref_cover, _rs, _tol = R.backward(cover, paints, gp, gr, g, K.BG)
    assert np.array_equal(_bits(grad_cover), _bits(ref_cover))
    assert np.isfinite(grad_cover).all() and all(np.isfinite(v).all() for v in sums.values())
    assert not grad_cover[1].any() and not sums["paints"][1].any() and sums["opacity"][0] == 0.0   # nothing reaches the target
    assert not grad_cover[2].any()                       # black at any coverage is k = 0
    assert np.abs(sums["paints"][2][:3]).min() > 1e-3    # but its colour moves the image
    h = 2.0 ** -12
    for ch in range(3):   # one-sided: k = sum w_c M_c is linear in the colour from 0 up
        hi = paints.copy()
        hi[2, ch] += h
        fd = float((g * (R.forward(cover, hi, gp, gr, K.BG, fused=False) - R.forward(cover, paints, gp, gr, K.BG, fused=False))).sum()) / h
        assert abs(sums["paints"][2][ch] - fd) <= 1e-9 * max(1.0, abs(fd)), ch


def test_depth_four_is_the_deepest_program_with_masks():
    c = K.case("depth4", False)
    assert K.harness_check(c["gr"], len(c["cover"]))[0] is None
    tree = [grp([0, grp([1, grp([2, grp([3, grp([4], mask=[5])])])])])]
    msg = K.harness_check(K.program(tree), 6)[0]
    assert msg is not None and "deeper" in msg
    tree = [grp([0, grp([1, grp([2, grp([3], mask=[4, grp([5])])])])])]   # the mask's group counts
    msg = K.harness_check(K.program(tree), 6)[0]
    assert msg is not None and "deeper" in msg


# ------------------------------------------------------------------------------------------------ refusals
def _gr(items, clip_off=(0,), clip_planes=(), opacity=()):
    return K.GR(np.array(items, dtype=np.int32).reshape(-1, 4), np.array(clip_off, dtype=np.int32), np.array(clip_planes, dtype=np.int32),
                np.array(opacity, dtype=np.float64))


# 4 planes: a fill, a target of one fill with an opacity and a clip of one plane, a mask of one fill
GOOD = _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,))
BAD = {
    "unknown op": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [5, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "hold followed by a fill": _gr([[1, 2, 0, 0], [0, 1, 0, 0], [3, 0, 0, 0], [0, 0, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "hold followed by a plain group": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [2, 4, -1, -1]], (0, 1), (2,), (0.5,)),
    "hold as the last item": _gr([[0, 0, 0, 0], [0, 3, 0, 0], [1, 4, 0, 0], [0, 1, 0, 0], [3, 2, 0, 0]], (0, 1), (2,), (0.5,)),
    "end_mask without a hold": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "end_mask after a fill": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0], [0, 3, 0, 0], [1, 6, 0, 0], [4, 5, 0, 0]], (0, 1), (2,), (0.5,)),
    "end_mask names another begin": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "hold names another begin": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 0, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "mask closed by end": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [2, 4, -1, -1]], (0, 1), (2,), (0.5,)),
    "target crosses its mask": _gr([[0, 0, 0, 0], [1, 4, 0, 0], [0, 1, 0, 0], [1, 6, 0, 0], [3, 1, 0, 0], [0, 3, 0, 0], [4, 3, 0, 0]], (0, 1), (2,), (0.5,)),
    "opacity slot out of range": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 1, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "opacity slot unused": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, -1, 0], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "clip out of range": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 1], [1, 6, 0, 0], [0, 3, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "plane twice": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 1, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "plane filled and clipped": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 2, 0, 0], [4, 4, 0, 0]], (0, 1), (2,), (0.5,)),
    "mask not closed": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [3, 1, 0, 0], [1, 6, 0, 0], [0, 3, 0, 0], [0, 3, 0, 0]], (0, 1), (2,), (0.5,)),
}


def test_the_headers_check_refuses_every_bad_program():
    msg, dev, n_clips, n_pairs, last = K.harness_check(GOOD, 4)
    assert msg is None and (n_clips, n_pairs, last) == (1, 1, 6)
    assert dev.tolist() == [[0, 0, 0, 0], [5, 0, 0, 0], [0, 1, 0, 0], [3, 0, 0, 0], [6, 1, 0, 0], [0, 3, 0, 0], [4, 1, 0, 0]]
    for what, gr in BAD.items():
        assert K.harness_check(gr, 4)[0] is not None, what
    assert "last item" in K.harness_check(BAD["hold as the last item"], 4)[0]
    assert "does not follow a HOLD" in K.harness_check(BAD["end_mask without a hold"], 4)[0]
    assert "HOLD is not followed" in K.harness_check(BAD["hold followed by a plain group"], 4)[0]
    assert K.harness_check(GOOD, 4, n_groups=3)[0] is not None and K.harness_check(GOOD, 4, n_groups=1)[0] is not None
    assert K.harness_check(GOOD, 4, n_opacities=2)[0] is not None and K.harness_check(GOOD, 4, n_clip_planes=2)[0] is not None
    assert K.harness_check(GOOD, 5)[0] is not None and K.harness_check(GOOD, 3)[0] is not None
    # the second pair of a program is pair 1, kept above the op
    gr = K.program([grp([0], mask=[1]), grp([2], opacity=0.5, mask=[3])])
    msg, dev, _c, n_pairs, last = K.harness_check(gr, 4)
    assert msg is None and n_pairs == 2 and last == 11 and dev[6:, 0].tolist() == [5 | 8, 0, 3 | 8, 6 | 8, 0, 4 | 8]
    assert dev[6:, 1].tolist() == [2, 2, 2, 3, 3, 3] and dev[9, 2] == 2 and dev[11, 2] == 2
    # everything group_program_check refuses
    from tests.test_group_host import BAD as GROUP_BAD

    for what, gr in GROUP_BAD.items():
        assert K.harness_check(gr, 3)[0] is not None, what


def _tree_of(diff, children):
    return [diff.Group(_tree_of(diff, c[1]), c[2], c[3], None if c[4] is None else _tree_of(diff, c[4])) if isinstance(c, tuple) else c for c in children]


def test_mask_program_is_the_cases_program_and_group_program_refuses_a_mask():
    from svgrasterize_amd import diff

    for name in K.CASES:
        c = K.case(name, False)
        tree = _tree_of(diff, c["tree"])
        got = diff.mask_program(tree)
        assert isinstance(got, diff.Groups) and got.items.dtype == np.int32 and got.opacity.dtype == np.float64
        for a, b in zip(got, c["gr"]):
            assert np.array_equal(a, b), name
        with pytest.raises(ValueError, match="mask_program"):
            diff.group_program(tree)
    for name in GK.CASES:   # a tree without masks: group_program's output
        c = GK.case(name, False)

        def tree_of(children):
            return [diff.Group(tree_of(k[1]), k[2], k[3]) if isinstance(k, tuple) else k for k in children]

        tree = tree_of(c["tree"])
        for a, b in zip(diff.mask_program(tree), diff.group_program(tree)):
            assert np.array_equal(a, b) and a.dtype == b.dtype, name
    for bad in (3, [1.5], [[0]], ["a"], diff.Group([0]), [diff.Group([0], mask=[1.5])]):
        with pytest.raises(TypeError):
            diff.mask_program(bad)
    with pytest.raises(ValueError):
        diff.mask_program([diff.Group([0], clip=[], mask=[1])])
    assert repr(diff.Group([0], 0.5, [1])) == "Group([0], opacity=0.5, clip=[1])" and "mask=[2]" in repr(diff.Group([0], mask=[2]))


def test_the_numpy_forms_refuse_before_any_library_call(monkeypatch):
    from svgrasterize_amd import _abi, diff
    from tests.test_group_host import BAD as GROUP_BAD

    def no_context(*_a, **_k):
        raise AssertionError("a refusal must come before any device work")

    monkeypatch.setattr(_abi.Context, "get", staticmethod(no_context))
    monkeypatch.setattr(diff, "group_depth", lambda: 4)
    rng = np.random.default_rng(7)
    cover, paints = GK.M.random_planes(rng, 4, 4, 5), GK.M.random_paints(rng, 4)
    gp = diff.GradientPaints(*G.make_gp([None] * 4))
    good = diff.Groups(*GOOD)
    g = np.zeros((4, 5, 4))

    def both(groups, kind, cover=cover, paints=paints, gp=gp, g=g):
        with pytest.raises(kind):
            diff.compose_masked(cover, paints, gp, groups)
        with pytest.raises(kind):
            diff.compose_masked_backward(cover, paints, gp, groups, g)

    for what, gr in BAD.items():
        both(diff.Groups(*gr), ValueError)
    gp3 = diff.GradientPaints(*G.make_gp([None] * 3))
    for what, gr in GROUP_BAD.items():
        if what != "unknown op":   # (op 3 is a HOLD here; the program is refused all the same, below)
            both(diff.Groups(*gr), ValueError, cover=cover[:3], paints=paints[:3], gp=gp3)
    both(diff.Groups(*GROUP_BAD["unknown op"]), ValueError, cover=cover[:3], paints=paints[:3], gp=gp3)
    deep = diff.Groups(*K.program([grp([0, grp([1, grp([2, grp([3], mask=[4, grp([5])])])])])]))
    both(deep, ValueError, cover=GK.M.random_planes(rng, 6, 4, 5), paints=GK.M.random_paints(rng, 6), gp=diff.GradientPaints(*G.make_gp([None] * 6)))
    both(good._replace(opacity=np.array([np.nan])), ValueError)
    both(good._replace(opacity=np.array([0.5, 0.5])), ValueError)
    both(good._replace(opacity=np.array([0.5], dtype=np.float32)), TypeError)
    both(good._replace(items=good.items.astype(np.float64)), TypeError)
    both(good._replace(items=good.items.reshape(-1)), ValueError)
    both(tuple(good), TypeError)
    both(None, TypeError)
    both(good, ValueError, cover=cover[:3])
    both(good, TypeError, cover=cover.astype(np.float16))
    both(good, ValueError, paints=paints[:2])
    with pytest.raises(ValueError):
        diff.compose_masked_backward(cover, paints, gp, good, np.zeros((4, 5, 3)))
    with pytest.raises(TypeError):
        diff.compose_masked_backward(cover, paints, gp, good, g.astype(np.float32))
    with pytest.raises(ValueError):
        diff.compose_masked(cover, paints, gp, good, origin=(1,))
    with pytest.raises(ValueError):
        diff.compose_masked(cover, paints, gp, good, bg=(0, 0, 0))
    # the grouped forms still refuse a program with masks
    with pytest.raises(ValueError):
        diff.compose_grouped(cover, paints, gp, good)
    # and the topology the masked forms accept is the program itself
    gtopo, n_groups = diff._mask_topology(good, 4, 1)
    assert n_groups == 2 and np.array_equal(gtopo[0], GOOD.items)
