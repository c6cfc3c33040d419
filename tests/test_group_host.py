"""Isolated groups in differentiable compositing on the host: csrc/svgr_group.h compiled by g++ (tests/group_harness.cpp) against
the oracle's layers, the numpy restatement (tests/group_ref.py), the gradient-paint harness for a program without groups, central
differences of every input, the one-sided and degenerate points by value, and every refusal of the program's check and of the
numpy forms of svgrasterize_amd.diff (which refuse before any library call: no device is needed)."""
import numpy as np
import pytest

from tests import gradpaint_cases as G
from tests import group_cases as K
from tests import group_ref as R
from tests.group_cases import grp

SUMS = ("paints", "m6", "geom", "stop_pos", "stop_rgba", "opacity")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name,with_bg", K.ALL)
def test_forward_is_the_oracles_layers(name, with_bg):
    """Equal.  Only "gradient_generic", whose transforms and geometry are not dyadic, is within 1e-13 as in
    test_gradpaint_host.py: the oracle's affine map and dot product are BLAS calls.  The restatement: equal everywhere."""
    c = K.case(name, with_bg)
    image = K.harness_forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"])
    want = K.oracle_image(c["cover"], c["paints"], c["gp"], c["tree"], c["bg"], c["origin"])
    if c["dyadic"]:
        assert np.array_equal(image, want), float(np.abs(image - want).max())
    else:
        assert np.abs(image - want).max() <= 1e-13, float(np.abs(image - want).max())
    assert np.array_equal(image, R.forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"]))


def test_the_cases_cover_what_they_claim():
    depth = K.harness().grh_depth()
    assert depth == R.DEPTH == 4
    seen = {}
    for name in K.CASES:
        gr = K.case(name, False)["gr"]
        level = deepest = 0
        for op in gr.items[:, 0]:
            level += 1 if op == 1 else (-1 if op == 2 else 0)
            deepest = max(deepest, level)
        seen[name] = (deepest, len(gr.opacity), np.diff(gr.clip_off).tolist())
    assert seen["flat"] == (0, 0, []) and seen["opacity"] == (1, 1, []) and seen["clip1"] == (1, 0, [1]) and seen["clip3"] == (1, 0, [3])
    assert seen["both"] == (1, 1, [2]) and seen["nested"][0] == 2 and seen["nested3"] == (3, 2, [2]) and seen["depth4"][0] == depth
    assert K.case("empty", False)["gr"].items[1:3, 0].tolist() == [1, 2]
    assert K.case("gradient_in_clip", False)["gp"].kind.tolist() == [0, 1, 1, 0, 0] and K.case("gradient_generic", False)["gp"].kind.tolist() == [0, 1, 2, 0, 0]
    assert [n for n in K.CASES if not K.case(n, False)["dyadic"]] == ["gradient_generic"]


@pytest.mark.parametrize("with_bg", (False, True))
def test_a_program_without_groups_is_the_painted_composition(with_bg):
    c = K.case("flat", with_bg)
    want = G.harness_forward(c["cover"], c["paints"], c["gp"], c["bg"], c["origin"])
    assert np.array_equal(_bits(K.harness_forward(c["cover"], c["paints"], c["gp"], c["gr"], c["bg"], c["origin"])), _bits(want))
    want_cover, want_sums, _used = G.harness_backward(c["cover"], c["paints"], c["gp"], c["g"], c["bg"], c["origin"])
    grad_cover, sums = K.harness_backward(c["cover"], c["paints"], c["gp"], c["gr"], c["g"], c["bg"], c["origin"])
    assert np.array_equal(_bits(grad_cover), _bits(want_cover))
    for k in want_sums:
        assert np.array_equal(_bits(sums[k]), _bits(want_sums[k])), k
    assert sums["opacity"].shape == (0,)


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
    if len(c["gr"].clip_planes) and name != "empty":
        assert np.abs(grad_cover[c["gr"].clip_planes]).max() > 1e-3   # (the clip planes do get a gradient)
    if len(c["gr"].opacity) and name != "empty":
        assert np.abs(sums["opacity"]).min() > 1e-3


# ------------------------------------------------------------------------------------------------ one-sided and degenerate points
def _run(cover, paints, tree, g, bg=None):
    gp, gr = G.make_gp([None] * len(cover)), K.program(tree)
    image = K.harness_forward(cover, paints, gp, gr, bg)
    grad_cover, sums = K.harness_backward(cover, paints, gp, gr, g, bg)
    ref_cover, ref_sums, _tol = R.backward(cover, paints, gp, gr, g, bg)
    assert np.array_equal(_bits(image), _bits(R.forward(cover, paints, gp, gr, bg)))
    assert np.array_equal(_bits(grad_cover), _bits(ref_cover))
    assert np.isfinite(image).all() and np.isfinite(grad_cover).all() and all(np.isfinite(v).all() for v in sums.values())
    return image, grad_cover, sums, ref_sums


def _planes(seed, n):
    rng = np.random.default_rng(seed)
    return K.M.random_planes(rng, n, 5, 7), K.M.random_paints(rng, n), rng.standard_normal((5, 7, 4))


def test_an_opacity_of_zero_hides_the_group_and_still_has_a_derivative():
    cover, paints, g = _planes(101, 3)
    image, grad_cover, sums, _ref = _run(cover, paints, [0, grp([1], opacity=0.0), 2], g, K.BG)
    without, _gc, _s, _r = _run(np.ascontiguousarray(cover[[0, 2]]), paints[[0, 2]], [0, 1], g, K.BG)
    assert np.array_equal(image, without)
    assert not grad_cover[1].any() and not sums["paints"][1].any()
    # d / d o at o = 0 is the group's own image against the adjoint of the canvas it lands on: not 0
    h = 2.0 ** -20
    gp = G.make_gp([None] * 3)
    hi = R.forward(cover, paints, gp, K.program([0, grp([1], opacity=h), 2]), K.BG)
    lo = R.forward(cover, paints, gp, K.program([0, grp([1], opacity=-h), 2]), K.BG)
    fd = float((g * (hi - lo)).sum()) / (2 * h)
    assert abs(sums["opacity"][0]) > 1e-2 and abs(sums["opacity"][0] - fd) <= 1e-9 * max(1.0, abs(fd))


def test_an_opacity_of_one_is_a_plain_isolated_group():
    cover, paints, g = _planes(102, 3)
    image, grad_cover, sums, _ref = _run(cover, paints, [0, grp([1, 2], opacity=1.0)], g)
    plain, plain_cover, plain_sums, _r = _run(cover, paints, [0, grp([1, 2])], g)
    assert np.array_equal(_bits(image), _bits(plain)) and np.array_equal(_bits(grad_cover), _bits(plain_cover))
    assert np.array_equal(_bits(sums["paints"]), _bits(plain_sums["paints"])) and sums["opacity"][0] != 0.0


def test_clip_planes_of_exactly_zero_and_one():
    cover, paints, g = _planes(103, 4)
    cover[2, :, :3] = 0.0      # the first clip plane: nothing through here, but for the second plane
    cover[2, :, 3:5] = 1.0     # everything through
    cover[3, :2] = 0.0
    cover[3, 2:4] = 1.0
    image, grad_cover, _sums, _ref = _run(cover, paints, [0, grp([1], clip=[2, 3])], g)
    gp = G.make_gp([None] * 4)
    k = R._mask(cover, K.program([0, grp([1], clip=[2, 3])]), 0)[0]
    assert (k[:2, :3] == 0.0).all() and (k[2:4] == 1.0).all()
    under = R.forward(np.ascontiguousarray(cover[:1]), paints[:1], G.make_gp([None]), K.program([0]))
    assert np.array_equal(image[:2, :3], under[:2, :3])                     # k == 0: the backdrop alone
    open_ = R.forward(np.ascontiguousarray(cover[:2]), paints[:2], G.make_gp([None] * 2), K.program([0, grp([1])]))
    assert np.array_equal(image[2:4], open_[2:4])                           # k == 1: the unclipped group
    assert not grad_cover[1][:2, :3].any()                                  # nothing reaches a fill under a mask of 0
    assert not grad_cover[2][2:4].any()                                     # m_2's factor 1 - m_3 is 0 where the second plane is 1
    assert np.abs(grad_cover[3][:2, :3]).max() > 0                          # where k == 0 the planes still have a derivative
    c = dict(cover=cover, paints=paints, gp=gp, gr=K.program([0, grp([1], clip=[2, 3])]), bg=None, origin=(0, 0), g=g)
    fd, tol = K.central_differences(c)
    assert (np.abs(grad_cover - fd["cover"]) <= tol["cover"]).all()


def test_an_opaque_group_over_an_opaque_backdrop():
    cover, paints, g = _planes(104, 3)
    cover[0], cover[1] = 1.0, 1.0
    paints[0], paints[1] = (0.2, 0.4, 0.6, 1.0), (0.7, 0.1, 0.3, 1.0)
    image, grad_cover, sums, _ref = _run(cover, paints, [0, grp([1, 2], opacity=1.0)], g, K.BG)
    assert (image[..., 3] == 1.0).all()
    assert not grad_cover[0].any() and not sums["paints"][0].any()          # nothing of the backdrop shows: u_g == 0, no division
    c = dict(cover=cover, paints=paints, gp=G.make_gp([None] * 3), gr=K.program([0, grp([1, 2], opacity=1.0)]), bg=K.BG, origin=(0, 0), g=g)
    fd, tol = K.central_differences(c)
    got = dict(cover=grad_cover, paints=sums["paints"], opacity=sums["opacity"])
    for k in got:
        assert (np.abs(got[k] - fd[k]) <= tol[k]).all(), k


def test_depth_four_is_the_deepest_program():
    tree, n = K._deep(4)
    cover, paints, g = _planes(105, n)
    _image, _gc, sums, _ref = _run(cover, paints, tree, g)
    assert sums["opacity"].shape == (4,) and sums["opacity"].all()
    tree5, n5 = K._deep(5)
    msg, _dev, _n = K.harness_check(K.program(tree5), n5)
    assert msg is not None and "deeper" in msg


# ------------------------------------------------------------------------------------------------ refusals
def _gr(items, clip_off=(0,), clip_planes=(), opacity=()):
    return K.GR(np.array(items, dtype=np.int32).reshape(-1, 4), np.array(clip_off, dtype=np.int32), np.array(clip_planes, dtype=np.int32),
                np.array(opacity, dtype=np.float64))


GOOD = _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,))   # 3 planes: a fill, a group of one fill, a clip plane
BAD = {
    "unknown op": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [3, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "fill out of range": _gr([[0, 3, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "fill negative": _gr([[0, -1, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "plane twice": _gr([[0, 1, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "plane filled and clipped": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 2, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "begin names no end": _gr([[0, 0, 0, 0], [1, 2, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "begin past the end": _gr([[0, 0, 0, 0], [1, 4, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "end names another begin": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 0, 0, 0]], (0, 1), (2,), (0.5,)),
    "end without begin": _gr([[0, 0, 0, 0], [2, 1, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "opacity slot out of range": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 1, 0]], (0, 1), (2,), (0.5,)),
    "opacity slot unused": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, -1, 0]], (0, 1), (2,), (0.5,)),
    "clip out of range": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 1]], (0, 1), (2,), (0.5,)),
    "clip plane out of range": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (0, 1), (3,), (0.5,)),
    "clip without a plane": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [2, 1, 0, 0]], (0, 0), (), (0.5,)),
    "clip_off from one": _gr([[0, 0, 0, 0], [1, 3, 0, 0], [0, 1, 0, 0], [2, 1, 0, 0]], (1, 1), (2,), (0.5,)),
    "plane unused": _gr([[0, 0, 0, 0], [1, 2, 0, 0], [2, 1, 0, 0]], (0, 1), (2,), (0.5,)),
    "crossed groups": _gr([[1, 2, 0, 0], [1, 3, 0, 0], [2, 0, -1, -1], [2, 1, -1, -1], [0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0]]),
}


def test_the_headers_check_refuses_every_bad_program():
    msg, dev, n_clips = K.harness_check(GOOD, 3)
    assert msg is None and n_clips == 1 and dev.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [2, 0, 0, 0]]
    for what, gr in BAD.items():
        assert K.harness_check(gr, 3)[0] is not None, what
    assert K.harness_check(GOOD, 3, n_groups=2)[0] is not None and K.harness_check(GOOD, 3, n_groups=0)[0] is not None
    assert K.harness_check(GOOD, 3, n_opacities=2)[0] is not None and K.harness_check(GOOD, 3, n_clip_planes=2)[0] is not None
    assert K.harness_check(GOOD, 4)[0] is not None and K.harness_check(GOOD, 2)[0] is not None
    tree5, n5 = K._deep(5)
    assert "deeper" in K.harness_check(K.program(tree5), n5)[0]
    tree4, n4 = K._deep(4)
    assert K.harness_check(K.program(tree4), n4)[0] is None


def test_group_program_is_the_cases_program():
    from svgrasterize_amd import diff

    def tree_of(children):
        return [diff.Group(tree_of(c[1]), c[2], c[3]) if isinstance(c, tuple) else c for c in children]

    for name in K.CASES:
        c = K.case(name, False)
        got = diff.group_program(tree_of(c["tree"]))
        assert isinstance(got, diff.Groups) and got.items.dtype == np.int32 and got.opacity.dtype == np.float64
        for a, b in zip(got, c["gr"]):
            assert np.array_equal(a, b), name
    for bad in (3, [1.5], [[0]], ["a"], diff.Group([0])):
        with pytest.raises(TypeError):
            diff.group_program(bad)
    with pytest.raises(ValueError):
        diff.group_program([diff.Group([0], clip=[])])


def test_the_numpy_forms_refuse_before_any_library_call(monkeypatch):
    from svgrasterize_amd import _abi, diff

    def no_context(*_a, **_k):
        raise AssertionError("a refusal must come before any device work")

    monkeypatch.setattr(_abi.Context, "get", staticmethod(no_context))
    monkeypatch.setattr(diff, "group_depth", lambda: 4)
    rng = np.random.default_rng(7)
    cover, paints = K.M.random_planes(rng, 3, 4, 5), K.M.random_paints(rng, 3)
    gp = diff.GradientPaints(*G.make_gp([None] * 3))
    good = diff.Groups(*GOOD)
    g = np.zeros((4, 5, 4))

    def both(groups, kind, cover=cover, paints=paints, gp=gp, g=g):
        with pytest.raises(kind):
            diff.compose_grouped(cover, paints, gp, groups)
        with pytest.raises(kind):
            diff.compose_grouped_backward(cover, paints, gp, groups, g)

    for what, gr in BAD.items():
        both(diff.Groups(*gr), ValueError)
    tree5, n5 = K._deep(5)
    deep = diff.Groups(*K.program(tree5))
    both(deep, ValueError, cover=K.M.random_planes(rng, n5, 4, 5), paints=K.M.random_paints(rng, n5), gp=diff.GradientPaints(*G.make_gp([None] * n5)))
    both(good._replace(opacity=np.array([np.nan])), ValueError)
    both(good._replace(opacity=np.array([np.inf])), ValueError)
    both(good._replace(opacity=np.array([0.5, 0.5])), ValueError)
    both(good._replace(opacity=np.array([[0.5]])), ValueError)
    both(good._replace(opacity=np.array([0.5], dtype=np.float32)), TypeError)
    both(good._replace(items=good.items.astype(np.float64)), TypeError)
    both(good._replace(items=good.items.reshape(-1)), ValueError)
    both(good._replace(clip_off=np.array([0.0, 1.0])), TypeError)
    both(tuple(good), TypeError)
    both(None, TypeError)
    both(good, ValueError, cover=cover[:2])
    both(good, TypeError, cover=cover.astype(np.float16))
    both(good, ValueError, paints=paints[:2])
    with pytest.raises(ValueError):
        diff.compose_grouped_backward(cover, paints, gp, good, np.zeros((4, 5, 3)))
    with pytest.raises(TypeError):
        diff.compose_grouped_backward(cover, paints, gp, good, g.astype(np.float32))
    with pytest.raises(ValueError):
        diff.compose_grouped(cover, paints, gp, good, origin=(1,))
    with pytest.raises(ValueError):
        diff.compose_grouped(cover, paints, gp, good, bg=(0, 0, 0))
