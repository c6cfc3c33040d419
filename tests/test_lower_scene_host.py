"""diff.lower_scene on the host: a hand-built Scene lowers to exactly the expected program, segments, rules, paints and sources,
and every node kind the differentiable route cannot draw raises and names itself.  No device: nothing here is lazy or dashed."""
import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import diff
from svgrasterize_amd.geometry import solid_paint
from svgrasterize_amd.paint import GradLinear, GradRadial, ImagePaint, Pattern

RED, GREEN, BLUE, GREY = (np.array(c, dtype=np.float64) for c in ((0.8, 0.1, 0.1, 0.9), (0.1, 0.7, 0.2, 1.0), (0.1, 0.2, 0.9, 0.5), (0.4, 0.4, 0.4, 0.7)))
STOPS = [(0.0, np.array([0.9, 0.1, 0.0, 1.0])), (0.4, np.array([0.1, 0.5, 0.2, 0.6])), (1.0, np.array([0.0, 0.1, 0.7, 0.8]))]


def _path(d):
    return S.Path.from_svg(d)


A, B, C_, D, E, F, G_, H_, I_, CL1, CL2, CL3, CL4 = (_path(d) for d in (
    "M1,1 L9,2 L5,9 Z", "M2,2 C6,1 9,5 7,9", "M3,1 L8,1 L8,6 L3,6 Z", "M1,4 L6,3 L4,8 Z", "M2,5 C4,3 8,4 9,8 L3,9 Z", "M4,4 L9,4 L9,9 L4,9 Z",
    "M1,1 L5,1 L5,5 Z", "M2,2 L7,3 L3,8 Z", "M0,0 L10,0 L10,10 L0,10 Z", "M0,0 L6,0 L6,6 L0,6 Z", "M2,2 L9,2 L9,9 L2,9 Z", "M1,1 L8,1 L8,8 Z",
    "M3,0 L10,5 L3,10 Z"))
T1 = S.Transform().translate(1.5, -0.5).scale(1.25)
T2 = S.Transform().rotate(0.3).translate(0.25, 2.0)
T3 = S.Transform().scale(0.5, 2.0)
RENDER = S.Transform().translate(2.0, 1.0).scale(1.5)


def _scene():
    lin = GradLinear((1.0, 2.0), (8.0, 7.0), STOPS, T3, "reflect", False, None)
    return S.Scene.group([
        S.Scene.fill(A, RED, "evenodd"),                                                             # plane 0
        S.Scene.stroke(B, GREEN, 1.5, "round", "bevel").transform(T1),                               # plane 1
        S.Scene.group([S.Scene.fill(C_, BLUE), S.Scene.fill(D, GREY)]),                              # planes 2, 3: flattened
        S.Scene.group([S.Scene.fill(E, RED), S.Scene.fill(F, GREEN)]).opacity(0.5),                  # planes 4, 5 in a group
        S.Scene.group([S.Scene.fill(G_, BLUE), S.Scene.fill(H_, GREY)]).opacity(0.25).clip(S.Scene.fill(CL1, None)),   # clip 6; 7, 8: one level
        S.Scene.fill(I_, RED).clip(S.Scene.group([S.Scene.fill(CL2, None, "evenodd"), S.Scene.fill(CL3, None, "nonzero").transform(T2)])).opacity(0.75),
        # ^ two levels: opacity outside; clip planes 9 (even-odd) and 10 (nonzero, under T2), then plane 11
        S.Scene.fill(CL4, lin).transform(T2).transform(T1),                                          # plane 12: gradient under T1 @ T2
    ])


def test_a_hand_built_scene_lowers_to_the_expected_arrays():
    low = diff.lower_scene(_scene(), RENDER, linear_rgb=True)
    assert isinstance(low, diff.LoweredScene) and isinstance(low.groups, diff.Groups) and isinstance(low.gp, diff.GradientPaints)
    fill, begin, end = diff.OP_FILL, diff.OP_BEGIN, diff.OP_END
    items = [[fill, 0, 0, 0], [fill, 1, 0, 0], [fill, 2, 0, 0], [fill, 3, 0, 0],
             [begin, 7, 0, 0], [fill, 4, 0, 0], [fill, 5, 0, 0], [end, 4, 0, -1],
             [begin, 11, 0, 0], [fill, 7, 0, 0], [fill, 8, 0, 0], [end, 8, 1, 0],
             [begin, 16, 0, 0], [begin, 15, 0, 0], [fill, 11, 0, 0], [end, 13, -1, 1], [end, 12, 2, -1],
             [fill, 12, 0, 0]]
    assert low.groups.items.tolist() == items
    assert low.groups.clip_off.tolist() == [0, 1, 3] and low.groups.clip_planes.tolist() == [6, 9, 10]
    assert low.groups.opacity.tolist() == [0.5, 0.25, 0.75]
    ident = S.Transform()
    t12 = T1 @ T2
    want_paths = [A.transform(ident), B.stroke(1.5, "round", "bevel").transform(T1), C_.transform(ident), D.transform(ident), E.transform(ident),
                  F.transform(ident), CL1.transform(ident), G_.transform(ident), H_.transform(ident), CL2.transform(ident), CL3.transform(T2),
                  I_.transform(ident), CL4.transform(t12)]
    packed = [p.packed() for p in want_paths]
    assert np.array_equal(low.segs, np.concatenate([np.asarray(s).reshape(-1, 8) for s, _k in packed]))
    assert np.array_equal(low.kinds, np.concatenate([k for _s, k in packed])) and low.kinds.dtype == np.uint8
    assert low.path_seg_off.tolist() == np.concatenate([[0], np.cumsum([len(k) for _s, k in packed])]).tolist()
    assert low.rules.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(low.m6, np.tile(RENDER.m6(), (13, 1)))
    solid = {0: RED, 1: GREEN, 2: BLUE, 3: GREY, 4: RED, 5: GREEN, 7: BLUE, 8: GREY, 11: RED}
    for p in range(13):
        want = solid_paint(solid[p], True) if p in solid else (np.ones(4) if p == 12 else np.zeros(4))
        assert np.array_equal(low.paints[p], want), p
    lin = GradLinear((1.0, 2.0), (8.0, 7.0), STOPS, T3, "reflect", False, None)
    gp, rows = diff.gradient_paints([lin], RENDER @ t12, linear_rgb=True)
    assert low.gp.kind.tolist() == [0] * 12 + [1] and low.gp.spread.tolist() == [0] * 12 + [2] and low.gp.path_stop_off.tolist() == [0] * 13 + [3]
    assert np.array_equal(low.gp.m6[12], gp.m6[0]) and np.array_equal(low.gp.geom[12], gp.geom[0]) and not low.gp.geom[:12].any()
    assert np.array_equal(low.gp.stop_pos, gp.stop_pos) and np.array_equal(low.gp.stop_rgba, gp.stop_rgba) and np.array_equal(rows[0], np.ones(4))
    roles = [r for r, _p in low.sources]
    assert roles == ["fill", "stroke", "fill", "fill", "fill", "fill", "clip", "fill", "fill", "clip", "clip", "fill", "fill"]
    for (_r, got), want in zip(low.sources, (A, B, C_, D, E, F, CL1, G_, H_, CL2, CL3, I_, CL4)):
        assert got is want
    # and the program is one compose_grouped accepts for these planes
    diff._group_topology(low.groups, 13, 3)


def test_the_render_transform_defaults_to_the_identity_and_a_clip_paths_paint_is_not_looked_at():
    low = diff.lower_scene(S.Scene.group([S.Scene.fill(A, RED), S.Scene.fill(D, BLUE)]))
    assert np.array_equal(low.m6, np.tile(S.Transform().m6(), (2, 1))) and low.groups.items.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0]]
    assert np.array_equal(low.paints[0], solid_paint(RED, False))
    none = S.Scene.fill(A, None)
    low = diff.lower_scene(S.Scene.group([S.Scene.fill(C_, GREY), S.Scene.fill(D, BLUE).clip(none.transform(T1))]))
    assert [r for r, _p in low.sources] == ["fill", "clip", "fill"]   # (a clip path's paint is not looked at)


def _deep(levels):
    node = S.Scene.fill(A, RED)
    for level in range(levels):
        node = S.Scene.group([S.Scene.fill(D, BLUE), node]).opacity(0.5 + 0.05 * level)
    return node


def test_every_refused_node_raises_and_names_itself():
    leaf = S.Scene.fill(A, RED)
    flt = object()
    pattern = Pattern(leaf, False, None, 0.0, 0.0, 4.0, 4.0, None, False)
    image = ImagePaint(np.zeros((2, 2, 4), dtype=np.uint8), S.Transform())
    bbox_lin = GradLinear((0.0, 0.0), (1.0, 1.0), STOPS, None, "pad", True, None)
    focal = GradRadial((5.0, 5.0), 4.0, (4.0, 4.0), None, STOPS, None, "pad", False, None)
    cases = [
        (leaf.clip(S.Scene.fill(CL1, None), bbox_units=True), "CLIP node"),
        (leaf.mask(S.Scene.fill(CL1, GREY)), "MASK node"),
        (S.Scene.group([leaf, leaf.filter(flt)]), "FILTER node"),
        (S.Scene.group([leaf, S.Scene.fill(D, BLUE).blend("multiply")]), "BLEND node"),
        (S.Scene.fill(A, pattern), "FILL node.*Pattern"),
        (S.Scene.stroke(B, image, 1.0), "STROKE node.*ImagePaint"),
        (S.Scene.fill(A, bbox_lin), "FILL node.*bbox_units"),
        (S.Scene.fill(A, focal), "FILL node.*focal"),
        (S.Scene.fill(A, GradLinear((0.0, 0.0), (1.0, 1.0), [], None, "pad", False, None)), "FILL node.*stops"),
        (S.Scene.fill(A, RED, "oddeven"), "FILL node.*fill rule"),
        (leaf.clip(S.Scene.fill(CL1, None).clip(S.Scene.fill(CL2, None))), "CLIP node.*inside a clip"),
        (leaf.clip(S.Scene.stroke(B, GREY, 1.0)), "STROKE node.*clip's scene"),
        (leaf.clip(S.Scene.fill(CL1, None).opacity(0.5)), "OPACITY node.*clip's scene"),
        (_deep(diff.group_depth() + 1), "OPACITY node.*deeper"),
        (S.Scene.fill(A, None), "draws nothing"),
    ]
    for scene, names in cases:
        with pytest.raises(ValueError, match=names):
            diff.lower_scene(scene)
    assert len(diff.lower_scene(_deep(diff.group_depth())).groups.opacity) == diff.group_depth()
    with pytest.raises(TypeError):
        diff.lower_scene([leaf])
