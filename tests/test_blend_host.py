"""CPU-side checks of mix-blend-mode and isolation: the loader's BLEND nodes, the arithmetic of csrc/svgr_core.h (host build,
tests/blend_harness.cpp) against the numpy restatement in tests/blend_ref.py, analytic cases of the spec's formulas, and the
Scene API around the new node (repr, to_path, dump / load).  No GPU needed."""
import json
import warnings

import numpy as np
import pytest

from svgrasterize_amd import layer as LY
from svgrasterize_amd import scene as SC
from svgrasterize_amd.geometry import Transform
from svgrasterize_amd.svg import svg_scene_from_str
from tests import blend_ref as R


@pytest.fixture(scope="module")
def bh():
    return R.harness()


def _load(body, **kw):
    text = (f'<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="40" height="30">'
            f'{body}</svg>')
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        scene, ids, _size = svg_scene_from_str(text, **kw)
    return scene, ids, [str(w.message) for w in caught]


def _nodes(scene, kind):
    """Every node of `kind` in the tree, depth first."""
    out = []

    def walk(node):
        k, args = node
        if k == kind:
            out.append(node)
        if k == SC.RENDER_GROUP:
            for child in args:
                walk(child)
        elif k in (SC.RENDER_OPACITY, SC.RENDER_TRANSFORM, SC.RENDER_FILTER, SC.RENDER_BLEND):
            walk(args[0])
        elif k in (SC.RENDER_CLIP, SC.RENDER_MASK):
            walk(args[0])
            walk(args[1])

    walk(scene)
    return out


def _top_children(scene):
    """The children of the document's top GROUP (under the outer svg's transform, if any)."""
    while scene[0] == SC.RENDER_TRANSFORM:
        scene = scene[1][0]
    assert scene[0] == SC.RENDER_GROUP
    return scene[1]


BACK = '<rect width="40" height="30" fill="#808080"/>'


# -- loader --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ['mix-blend-mode="multiply"', 'style="mix-blend-mode: multiply"',
                                  'style="fill: red; mix-blend-mode:MULTIPLY"', 'mix-blend-mode=" Multiply "'])
def test_loader_blend_node(form):
    scene, _, warned = _load(f'{BACK}<rect x="5" y="5" width="10" height="10" fill="red" {form}/>')
    assert not warned
    children = _top_children(scene)
    assert len(children) == 2 and children[1][0] == SC.RENDER_BLEND
    target, mode = children[1][1]
    assert mode == LY.BLEND_MULTIPLY == R.CODE["multiply"] and target[0] == SC.RENDER_FILL


@pytest.mark.parametrize("name", R.MODES[1:])
def test_loader_every_mode(name):
    scene, _, warned = _load(f'{BACK}<circle cx="10" cy="10" r="5" style="mix-blend-mode:{name.upper()}"/>')
    assert not warned
    (node,) = _nodes(scene, SC.RENDER_BLEND)
    assert node[1][1] == R.CODE[name] == LY.BLEND_MODES[name]


def test_loader_normal_is_no_attribute():
    plain, _, _ = _load(f'{BACK}<rect x="5" y="5" width="10" height="10" fill="red"/>')
    for form in ('mix-blend-mode="normal"', 'style="mix-blend-mode: NORMAL"'):
        normal, _, warned = _load(f'{BACK}<rect x="5" y="5" width="10" height="10" fill="red" {form}/>')
        assert not warned and not _nodes(normal, SC.RENDER_BLEND)
        assert repr(normal) == repr(plain)


@pytest.mark.parametrize("value", ["plus-lighter", "plus-darker", "bogus", "multiply2"])
def test_loader_unknown_mode_warns_and_draws_normal(value):
    plain, _, _ = _load(f'{BACK}<rect x="5" y="5" width="10" height="10" fill="red"/>')
    scene, _, warned = _load(f'{BACK}<rect x="5" y="5" width="10" height="10" fill="red" style="mix-blend-mode:{value}"/>')
    assert any("mix-blend-mode" in w for w in warned)
    assert not _nodes(scene, SC.RENDER_BLEND) and repr(scene) == repr(plain)


def test_loader_group_blends_as_one():
    scene, _, _ = _load(f'{BACK}<g style="mix-blend-mode:screen"><rect width="5" height="5"/><rect x="6" width="5" height="5"/></g>')
    children = _top_children(scene)
    assert len(children) == 2 and children[1][0] == SC.RENDER_BLEND
    target = children[1][1][0]
    assert target[0] == SC.RENDER_GROUP and len(target[1]) == 2


def test_loader_isolation():
    body = '<rect width="5" height="5"/><rect width="5" height="5" fill="red" mix-blend-mode="multiply"/>'
    auto, _, _ = _load(f'{BACK}<g style="isolation:auto">{body}</g>')
    spliced, _, _ = _load(f'{BACK}<g>{body}</g>')
    assert repr(auto) == repr(spliced) and len(_top_children(auto)) == 3   # a plain <g> splices into its parent
    iso, _, warned = _load(f'{BACK}<g style="isolation: ISOLATE">{body}</g>')
    assert not warned
    children = _top_children(iso)
    assert len(children) == 2 and children[1][0] == SC.RENDER_GROUP
    assert [c[0] for c in children[1][1]] == [SC.RENDER_FILL, SC.RENDER_BLEND]
    # a lone blended child of an isolated group has nothing to blend with: its target
    lone, _, _ = _load(f'{BACK}<g isolation="isolate"><rect width="5" height="5" fill="red" mix-blend-mode="multiply"/></g>')
    assert not _nodes(lone, SC.RENDER_BLEND) and len(_top_children(lone)) == 2


def test_loader_blend_outside_transform_and_decorations():
    scene, _, _ = _load(f'{BACK}<rect width="5" height="5" opacity="0.5" transform="translate(3, 4)" mix-blend-mode="darken"/>')
    node = _top_children(scene)[1]
    assert node[0] == SC.RENDER_BLEND and node[1][1] == LY.BLEND_DARKEN
    inner = node[1][0]
    assert inner[0] == SC.RENDER_TRANSFORM and inner[1][0][0] == SC.RENDER_OPACITY
    assert np.allclose(np.asarray(inner[1][1].m)[:2, 2], [3, 4])


def test_loader_use_keeps_the_blend():
    scene, ids, _ = _load(f'{BACK}<defs><rect id="r" width="5" height="5" fill="red" mix-blend-mode="hue"/></defs>'
                          '<use xlink:href="#r" x="7" y="2"/>')
    assert ids["r"][0] == SC.RENDER_BLEND
    node = _top_children(scene)[1]
    # the use's translation goes under the blend: the blend stays outermost, among the use's siblings
    assert node[0] == SC.RENDER_BLEND and node[1][1] == LY.BLEND_HUE and node[1][0][0] == SC.RENDER_TRANSFORM


def test_loader_blend_not_inherited():
    scene, _, _ = _load(f'{BACK}<g mix-blend-mode="multiply" fill="red"><rect width="5" height="5"/><g><rect x="6" width="5" height="5"/>'
                        '<rect x="12" width="5" height="5"/></g></g>')
    blends = _nodes(scene, SC.RENDER_BLEND)
    assert len(blends) == 1   # the <g> alone, not its descendants
    assert "mix-blend-mode" not in __import__("svgrasterize_amd").svg._INHERITED


# -- arithmetic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.MODES)
def test_host_build_matches_restatement(bh, name):
    grid = R.premultiplied_grid()
    rng = np.random.default_rng(11)
    for perm in range(3):
        src = grid[rng.permutation(len(grid))]
        got = R.harness_px(bh, name, grid, src)
        want = R.mix_blend_px(name, grid, src)
        assert np.isfinite(got).all()
        # the expressions are the same, in the same order: bit for bit
        assert np.array_equal(got, want), (name, np.abs(got - want).max())


@pytest.mark.parametrize("name", R.MODES)
def test_blend_functions_match_restatement(bh, name):
    rng = np.random.default_rng(2)
    cb = rng.choice([0.0, 0.25, 0.5, 1.0, 0.1, 0.9], (2000, 3))
    cb[1000:] = rng.random((1000, 3))
    cs = rng.permutation(cb)
    assert np.array_equal(R.harness_b(bh, name, cb, cs), R.blend(name, cb, cs))


def test_special_cases_of_the_spec(bh):
    # color-dodge: Cb = 0 -> 0, else Cs = 1 -> 1; color-burn: Cb = 1 -> 1, else Cs = 0 -> 0
    cb = np.array([[0.0, 0.3, 1.0]])
    one, zero = np.ones((1, 3)), np.zeros((1, 3))
    assert np.array_equal(R.harness_b(bh, "color-dodge", cb, one), [[0.0, 1.0, 1.0]])
    assert np.array_equal(R.harness_b(bh, "color-burn", cb, zero), [[0.0, 0.0, 1.0]])
    # soft-light: D(Cb) is the cubic up to 0.25 and sqrt above
    cs = np.full((1, 3), 0.75)
    cbs = np.array([[0.2, 0.25, 0.64]])
    d = np.array([((16 * 0.2 - 12) * 0.2 + 4) * 0.2, ((16 * 0.25 - 12) * 0.25 + 4) * 0.25, 0.8])
    assert np.allclose(R.harness_b(bh, "soft-light", cbs, cs), cbs + 0.5 * (d - cbs), rtol=0, atol=1e-15)


def test_analytic_identities(bh):
    rng = np.random.default_rng(4)
    px = R.premultiplied_grid(5, 512)
    opaque = px.copy()
    opaque[:, 3] = 1.0
    opaque[:, :3] = rng.random((512, 3))
    white, black = np.array([1.0, 1.0, 1.0, 1.0]), np.array([0.0, 0.0, 0.0, 1.0])
    # multiply by white and screen with black leave an opaque backdrop as it is
    for mode, s in (("multiply", white), ("screen", black)):
        got = R.harness_px(bh, mode, opaque, np.broadcast_to(s, opaque.shape))
        assert np.allclose(got, opaque, rtol=0, atol=1e-15), mode
    # difference of a colour with itself is black (opaque: alpha stays 1)
    got = R.harness_px(bh, "difference", opaque, opaque)
    assert np.allclose(got[:, :3], 0.0, atol=1e-15) and np.array_equal(got[:, 3], np.ones(512))
    # normal is source-over, bit for bit
    src = px[rng.permutation(512)]
    over = src[:, :3] + px[:, :3] * (1.0 - src[:, 3:4])
    got = R.harness_px(bh, "normal", px, src)
    assert np.array_equal(got[:, :3], over) and np.array_equal(got[:, 3], src[:, 3] + px[:, 3] * (1.0 - src[:, 3]))
    # over opaque pixels (both alphas 1): luminosity keeps Lum(Cs), color keeps Lum(Cb)
    s_op = opaque[rng.permutation(512)]
    lum = lambda c: 0.3 * c[:, 0] + 0.59 * c[:, 1] + 0.11 * c[:, 2]
    assert np.allclose(lum(R.harness_px(bh, "luminosity", opaque, s_op)), lum(s_op), atol=1e-12)
    assert np.allclose(lum(R.harness_px(bh, "color", opaque, s_op)), lum(opaque), atol=1e-12)
    # hue / saturation keep Lum(Cb) too; every result of the non-separable modes stays in [0, 1]
    for mode in ("hue", "saturation", "color", "luminosity"):
        got = R.harness_px(bh, mode, opaque, s_op)
        assert (got >= -1e-15).all() and (got <= 1 + 1e-15).all(), mode
        if mode in ("hue", "saturation"):
            assert np.allclose(lum(got), lum(opaque), atol=1e-12), mode


def test_alpha_and_transparent_inputs(bh):
    px = R.premultiplied_grid(9, 1024)
    clear = np.zeros(4)
    for mode in R.MODES:
        # a transparent source leaves the backdrop; a transparent backdrop gives the source (up to rounding of cs * 1)
        assert np.array_equal(R.harness_px(bh, mode, px, np.broadcast_to(clear, px.shape)), px), mode
        assert np.array_equal(R.harness_px(bh, mode, np.broadcast_to(clear, px.shape), px), px), mode
        got = R.harness_px(bh, mode, px, px[::-1])
        assert np.array_equal(got[:, 3], px[::-1, 3] + px[:, 3] * (1.0 - px[::-1, 3])), mode   # ao = as + ab (1 - as)


# -- Scene API -----------------------------------------------------------------------------------------------------------------
def _doc_scene():
    scene, _, _ = _load(f'{BACK}<g mix-blend-mode="soft-light"><rect width="5" height="5" fill="red"/>'
                        '<circle cx="9" cy="9" r="3" fill="blue" transform="rotate(10)"/></g>'
                        '<rect x="3" y="3" width="8" height="6" fill="green" style="mix-blend-mode:luminosity"/>')
    return scene


def test_scene_blend_constructor():
    leaf = SC.Scene.fill(_doc_scene().to_path(Transform()), np.array([1.0, 0.0, 0.0, 1.0]))
    assert leaf.blend("normal") is leaf and leaf.blend(0) is leaf
    node = leaf.blend("color-burn")
    assert node == SC.Scene(SC.RENDER_BLEND, (leaf, LY.BLEND_COLOR_BURN)) and SC.RENDER_BLEND == 8
    assert leaf.blend(LY.BLEND_EXCLUSION)[1][1] == 11
    with pytest.raises((ValueError, KeyError)):
        leaf.blend("plus-lighter")
    with pytest.raises(ValueError):
        leaf.blend(16)
    # a transform goes under the blend
    moved = node.transform(Transform().translate(2, 3))
    assert moved[0] == SC.RENDER_BLEND and moved[1][0][0] == SC.RENDER_TRANSFORM


def test_scene_repr_names_the_mode():
    text = repr(_doc_scene())
    assert "BLEND soft-light" in text and "BLEND luminosity" in text


def test_scene_to_path_looks_through_blends():
    scene = _doc_scene()
    plain, _, _ = _load(f'{BACK}<g><rect width="5" height="5" fill="red"/>'
                        '<circle cx="9" cy="9" r="3" fill="blue" transform="rotate(10)"/></g>'
                        '<rect x="3" y="3" width="8" height="6" fill="green"/>')
    tr = Transform().scale(2.0)
    a, b = scene.to_path(tr), plain.to_path(tr)
    assert len(a.subpaths) == len(b.subpaths) == 4
    assert repr(a) == repr(b)


def test_scene_dump_round_trip():
    from svgrasterize_amd import scenedump

    scene = _doc_scene()
    tree, arrays = scenedump.dump_scene(scene)
    text = json.dumps(tree)
    assert '"t": "blend"' in text and '"mode": "soft-light"' in text and '"mode": "luminosity"' in text
    import io

    buf = io.BytesIO()
    np.savez(buf, tree=np.array(text), info=np.array("{}"), **arrays)
    buf.seek(0)
    loaded, _, _ = scenedump.load_scene(buf)
    assert len(_nodes(loaded, SC.RENDER_BLEND)) == 2
    tree2, arrays2 = scenedump.dump_scene(loaded)
    assert scenedump.compare_dumps(tree, arrays, tree2, arrays2) == []


def test_blend_scene_is_never_batch_entries():
    from svgrasterize_amd import displaylist

    scene = _doc_scene()
    assert scene.leaves(Transform()) is None
    assert SC._batchable_leaves_(_nodes(scene, SC.RENDER_BLEND)[1], Transform(), False) is None
    assert displaylist._compile(scene, False) is None
