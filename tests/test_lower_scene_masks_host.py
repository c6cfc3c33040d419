"""diff.lower_scene(..., masks=True) on the host: a MASK node lowers to the HOLD / BEGIN / END_MASK triple of a mask_program, with
the mask's planes after its target's and in the role "mask"; what it drops and what it refuses.  No device."""
import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import diff
from svgrasterize_amd.paint import GradRadial

RED, GREEN, BLUE, GREY = (np.array(c, dtype=np.float64) for c in ((0.8, 0.1, 0.1, 0.9), (0.1, 0.7, 0.2, 1.0), (0.1, 0.2, 0.9, 0.5), (0.4, 0.4, 0.4, 0.7)))
STOPS = [(0.0, np.array([1.0, 1.0, 1.0, 1.0])), (0.6, np.array([0.6, 0.6, 0.6, 0.8])), (1.0, np.array([0.0, 0.0, 0.0, 0.0]))]
A, B, C_, D, CL1, M1, M2 = (S.Path.from_svg(d) for d in (
    "M1,1 L9,2 L5,9 Z", "M2,2 C6,1 9,5 7,9", "M3,1 L8,1 L8,6 L3,6 Z", "M1,4 L6,3 L4,8 Z", "M0,0 L6,0 L6,6 L0,6 Z", "M0,0 L10,0 L10,10 L0,10 Z",
    "M2,1 L9,5 L2,9 Z"))
T1 = S.Transform().translate(1.5, -0.5).scale(1.25)
FILL, BEGIN, END, HOLD, END_MASK = diff.OP_FILL, diff.OP_BEGIN, diff.OP_END, diff.OP_HOLD, diff.OP_END_MASK


def _radial():
    return GradRadial((5.0, 5.0), 4.5, None, None, STOPS, None, "pad", False, None)


def test_a_mask_node_lowers_to_the_triple():
    leaf = S.Scene.fill(A, RED)
    low = diff.lower_scene(leaf.mask(S.Scene.fill(M1, GREY)), masks=True)
    assert low.groups.items.tolist() == [[BEGIN, 2, 0, 0], [FILL, 0, 0, 0], [HOLD, 0, -1, -1], [BEGIN, 5, 0, 0], [FILL, 1, 0, 0], [END_MASK, 3, 0, 0]]
    assert [r for r, _p in low.sources] == ["fill", "mask"] and low.sources[0][1] is A and low.sources[1][1] is M1
    assert np.array_equal(low.paints[1], S.geometry.solid_paint(GREY, False))
    diff._mask_topology(low.groups, 2, 0)
    with pytest.raises(ValueError):
        diff._group_topology(low.groups, 2, 0)


def test_mask_clip_opacity_takes_one_level_and_the_masks_scene_is_an_ordinary_scene():
    target = S.Scene.group([S.Scene.fill(A, RED), S.Scene.stroke(B, GREEN, 1.5)]).opacity(0.6).clip(S.Scene.fill(CL1, None))
    mask = S.Scene.group([S.Scene.fill(M1, _radial()), S.Scene.stroke(B, GREY, 2.0).opacity(0.5), S.Scene.fill(M2, BLUE).transform(T1)])
    low = diff.lower_scene(S.Scene.group([S.Scene.fill(C_, BLUE), target.mask(mask), S.Scene.fill(D, GREY)]), masks=True)
    # planes: 0 C_; clip 1; target 2, 3; mask 4 (radial), 5 (stroke in an opacity group), 6; 7 D
    assert low.groups.items.tolist() == [
        [FILL, 0, 0, 0],
        [BEGIN, 4, 0, 0], [FILL, 2, 0, 0], [FILL, 3, 0, 0], [HOLD, 1, 0, 0],
        [BEGIN, 11, 0, 0], [FILL, 4, 0, 0], [BEGIN, 9, 0, 0], [FILL, 5, 0, 0], [END, 7, 1, -1], [FILL, 6, 0, 0], [END_MASK, 5, 0, 0],
        [FILL, 7, 0, 0]]
    assert low.groups.clip_off.tolist() == [0, 1] and low.groups.clip_planes.tolist() == [1] and low.groups.opacity.tolist() == [0.6, 0.5]
    assert [r for r, _p in low.sources] == ["fill", "clip", "fill", "stroke", "mask", "mask", "mask", "fill"]
    assert [p for _r, p in low.sources] == [C_, CL1, A, B, M1, B, M2, D]
    assert low.gp.kind.tolist() == [0, 0, 0, 0, 2, 0, 0, 0] and low.gp.path_stop_off.tolist() == [0, 0, 0, 0, 0, 3, 3, 3, 3]
    assert np.array_equal(low.segs[low.path_seg_off[6]:low.path_seg_off[7]], np.asarray(M2.transform(T1).packed()[0]).reshape(-1, 8))
    diff._mask_topology(low.groups, 8, 2)
    # any other order takes a level more: MASK(OPACITY(..)) without a CLIP between them is two groups
    low = diff.lower_scene(S.Scene.fill(A, RED).opacity(0.5).mask(S.Scene.fill(M1, GREY)), masks=True)
    assert low.groups.items[:, 0].tolist() == [BEGIN, BEGIN, FILL, END, HOLD, BEGIN, FILL, END_MASK] and low.groups.items[3].tolist() == [END, 1, 0, -1]
    low = diff.lower_scene(S.Scene.fill(A, RED).clip(S.Scene.fill(CL1, None)).opacity(0.5).mask(S.Scene.fill(M1, GREY)), masks=True)
    assert low.groups.items[:, 0].tolist() == [BEGIN, BEGIN, BEGIN, FILL, END, END, HOLD, BEGIN, FILL, END_MASK]


def test_a_mask_inside_a_mask_and_without_masks_nothing_changes():
    inner = S.Scene.fill(M2, GREEN).mask(S.Scene.fill(CL1, GREY))
    scene = S.Scene.fill(A, RED).mask(S.Scene.group([S.Scene.fill(M1, GREY), inner]))
    low = diff.lower_scene(scene, masks=True)
    assert low.groups.items[:, 0].tolist() == [BEGIN, FILL, HOLD, BEGIN, FILL, BEGIN, FILL, HOLD, BEGIN, FILL, END_MASK, END_MASK]
    assert [r for r, _p in low.sources] == ["fill", "mask", "mask", "mask"]
    with pytest.raises(ValueError, match="MASK node.*masks=True"):
        diff.lower_scene(scene)
    with pytest.raises(ValueError, match="MASK node"):
        diff.lower_scene(scene, masks=False)
    plain = S.Scene.group([S.Scene.fill(A, RED), S.Scene.fill(D, BLUE).opacity(0.5).clip(S.Scene.fill(CL1, None))])
    a, b = diff.lower_scene(plain), diff.lower_scene(plain, masks=True)
    for x, y in zip(a.groups, b.groups):
        assert np.array_equal(x, y)
    assert np.array_equal(a.segs, b.segs) and a.sources == b.sources


def test_what_draws_nothing_is_dropped():
    backdrop, top = S.Scene.fill(C_, BLUE), S.Scene.fill(D, GREY)
    nothing = S.Scene.fill(M1, None)
    # an empty mask scene hides its target: neither gets a plane, the clip's planes go too
    target = S.Scene.fill(A, RED).clip(S.Scene.fill(CL1, None))
    low = diff.lower_scene(S.Scene.group([backdrop, target.mask(nothing), top]), masks=True)
    assert low.groups.items.tolist() == [[FILL, 0, 0, 0], [FILL, 1, 0, 0]] and [p for _r, p in low.sources] == [C_, D]
    low = diff.lower_scene(S.Scene.group([backdrop, target.mask(S.Scene.group([nothing, nothing.opacity(0.5)])), top]), masks=True)
    assert low.groups.items.tolist() == [[FILL, 0, 0, 0], [FILL, 1, 0, 0]]
    # a target that draws nothing is dropped together with its mask
    low = diff.lower_scene(S.Scene.group([backdrop, S.Scene.fill(A, None).mask(S.Scene.fill(M1, GREY)), top]), masks=True)
    assert low.groups.items.tolist() == [[FILL, 0, 0, 0], [FILL, 1, 0, 0]] and [p for _r, p in low.sources] == [C_, D]
    with pytest.raises(ValueError, match="draws nothing"):
        diff.lower_scene(S.Scene.fill(A, RED).mask(nothing), masks=True)


def _deep(levels, mask_at_the_bottom):
    node = S.Scene.fill(A, RED)
    if mask_at_the_bottom:
        node, levels = node.mask(S.Scene.fill(M1, GREY)), levels - 1
    for level in range(levels):
        node = S.Scene.group([S.Scene.fill(D, BLUE), node]).opacity(0.5 + 0.05 * level)
    return node


def test_what_is_refused_names_itself():
    leaf = S.Scene.fill(A, RED)
    with pytest.raises(ValueError, match="MASK node.*bbox_units"):
        diff.lower_scene(leaf.mask(S.Scene.fill(M1, GREY), bbox_units=True), masks=True)
    with pytest.raises(ValueError, match="CLIP node.*bbox_units"):
        diff.lower_scene(leaf.clip(S.Scene.fill(CL1, None), bbox_units=True).mask(S.Scene.fill(M1, GREY)), masks=True)
    depth = diff.group_depth()
    assert len(diff.lower_scene(_deep(depth, True), masks=True).groups.opacity) == depth - 1
    with pytest.raises(ValueError, match="MASK node.*deeper"):
        diff.lower_scene(_deep(depth + 1, True), masks=True)
    # the mask's own group counts: a group inside the mask of a pair at the deepest level is one too many
    deep_mask = S.Scene.fill(M1, GREY).opacity(0.5)
    node = leaf.mask(deep_mask)
    for level in range(depth - 1):
        node = S.Scene.group([S.Scene.fill(D, BLUE), node]).opacity(0.5)
    with pytest.raises(ValueError, match="OPACITY node.*deeper"):
        diff.lower_scene(node, masks=True)
    with pytest.raises(ValueError, match="FILTER node"):
        diff.lower_scene(leaf.mask(S.Scene.fill(M1, GREY).filter(object())), masks=True)


DOCUMENT = """<svg xmlns="http://www.w3.org/2000/svg" width="20" height="20" viewBox="0 0 20 20">
<defs>
<radialGradient id="g" cx="10" cy="10" r="9" gradientUnits="userSpaceOnUse"><stop offset="0" stop-color="#fff"/><stop offset="1" stop-color="#000" stop-opacity="0"/></radialGradient>
<mask id="m" maskUnits="userSpaceOnUse" maskContentUnits="userSpaceOnUse" x="0" y="0" width="20" height="20"><rect x="0" y="0" width="20" height="20" fill="url(#g)"/></mask>
</defs>
<rect x="1" y="1" width="18" height="18" fill="#123456"/>
<g mask="url(#m)" opacity="0.5"><path d="M2,2 L18,4 L10,18 Z" fill="#c03020"/></g>
</svg>"""


def test_a_loaded_document_with_a_mask_lowers():
    scene = S.svg_scene_from_str(DOCUMENT)[0]
    with pytest.raises(ValueError, match="MASK node"):
        diff.lower_scene(scene)
    low = diff.lower_scene(scene, masks=True)
    # the loader's MASK(OPACITY(..)) has no CLIP between the two: the opacity's group sits inside the target
    assert low.groups.items.tolist() == [[FILL, 0, 0, 0], [BEGIN, 5, 0, 0], [BEGIN, 4, 0, 0], [FILL, 1, 0, 0], [END, 2, 0, -1], [HOLD, 1, -1, -1],
                                         [BEGIN, 8, 0, 0], [FILL, 2, 0, 0], [END_MASK, 6, 0, 0]]
    assert [r for r, _p in low.sources] == ["fill", "fill", "mask"] and low.gp.kind.tolist() == [0, 0, 2] and low.groups.opacity.tolist() == [0.5]
    assert low.gp.geom[2][:3].tolist() == [10.0, 10.0, 9.0] and np.abs(low.gp.stop_rgba - [[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]]).max() <= 1e-12
    diff._mask_topology(low.groups, 3, 1)
