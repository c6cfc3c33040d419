"""The canvas reference (tests/canvas_ref.py) and the directed cases (tests/canvas_cases.py) on the host: the reference against the
oracle's own solid render and against closed-form rectangle coverage, every case's distance from the `mask < 1e-6` cut, and the
layout every case names, from its geometry."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import canvas_cases as cc
from tests import canvas_ref as cr
from tests.canvas_ref import Entry, Group
from tests.util import assert_close64


def _solid_reduction(case):
    """The case's paths (clip sources too) as plain solid fills, in batch order."""
    out = []
    for n, (kind, idx, d, rule) in enumerate(cc.paths_of(case)):
        paint = case.entries[idx].paint if kind == "entry" else cc.PAINTS[n % 8]
        out.append(Entry(d, rule, cc.PAINTS[(n + 3) % 8] if isinstance(paint, cr.Grad) else paint))
    return out


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_solid_scenes_equal_the_oracles_render(case):
    entries = _solid_reduction(case)
    segs, kinds, offs = [], [], [0]
    for e in entries:
        lines, cubics = cr.segments(e.d)
        s = np.zeros((len(lines) + len(cubics), 8))
        s[:len(lines), :4] = lines.reshape(-1, 4)
        s[len(lines):] = cubics.reshape(-1, 8)
        segs.append(s)
        kinds.append(np.r_[np.zeros(len(lines), np.uint8), np.ones(len(cubics), np.uint8)])
        offs.append(offs[-1] + len(s))
    for clamp in (False, True):
        want, _P, _E = orc.render_solid(np.concatenate(segs), np.concatenate(kinds), offs, [1 if e.rule else 0 for e in entries],
                                        np.array([e.paint for e in entries]), case.viewport, clip01=clamp)
        assert_close64(cr.render(entries, (), case.viewport, clamp=clamp), want, atol=1e-12, what=case.name)


def _rect_area(rect, viewport):
    """Closed form: the area of pixel (r, c) inside the rectangle (x0, y0, x1, y1) (x: columns, y: rows), over the viewport."""
    x0, y0, x1, y1 = rect
    r = np.arange(viewport[0], viewport[0] + viewport[2], dtype=np.float64)
    c = np.arange(viewport[1], viewport[1] + viewport[3], dtype=np.float64)
    h = np.clip(np.minimum(r + 1, max(y0, y1)) - np.maximum(r, min(y0, y1)), 0, None)
    w = np.clip(np.minimum(c + 1, max(x0, x1)) - np.maximum(c, min(x0, x1)), 0, None)
    return h[:, None] * w[None, :]


def test_rectangle_coverage_is_the_closed_form_overlap():
    seen = 0
    for case in cc.CASES:
        for _kind, _idx, d, rule in cc.paths_of(case):
            rects = cc.rects_of(d)
            if rects is None:
                continue
            if len(rects) == 2:      # a ring: the inner rectangle lies inside the outer one
                area = _rect_area(rects[0], case.viewport)
                inner = _rect_area(rects[1], case.viewport)
                want = area - inner if rule == "evenodd" else area   # (nonzero: both wind the same way)
            else:
                want = _rect_area(rects[0], case.viewport)
            got, _bb = cr.mask_layer(d, rule, case.viewport)
            assert_close64(got, want, atol=1e-12, what=f"{case.name}: {d}")
            seen += 1
    assert seen > 500


def test_hand_sized_clip_and_group_canvases():
    """Whole canvases written out from the closed form: a clip pair, a clipped and faded group over a background, a group whose
    clip misses it."""
    vp = (2, 3, 6, 9)
    A = lambda *rect: _rect_area(rect, vp)[..., None]
    R = lambda x0, y0, x1, y1: f"M{x0},{y0} H{x1} V{y1} H{x0} Z"
    p, q, s = cc.PAINTS[0], cc.PAINTS[1], cc.PAINTS[2]
    over = lambda dst, src: src + dst * (1 - src[..., 3:])
    # a rectangle under an opacity, clipped by another one
    got = cr.render([Entry(R(4.25, 3.5, 9.5, 6.75), None, p, opacity=0.5, clip=(R(6.5, 2.25, 11.0, 5.5), None))], (), vp)
    want = ((A(4.25, 3.5, 9.5, 6.75) * p) * 0.5) * A(6.5, 2.25, 11.0, 5.5)
    assert_close64(got, want, atol=1e-12, what="clip pair")
    # pixel (4, 7) lies inside both, pixel (4, 6) has half its columns inside the clip, row 2 is above the rectangle
    assert want[2, 4, 3] == p[3] * 0.5 and want[2, 3, 3] == (p[3] * 0.5) * 0.5 and want[0].max() == 0.0
    # background, then a group of two members, clipped and faded as a whole
    entries = [Entry(R(3.0, 2.0, 12.0, 8.0), None, s),
               Entry(R(4.5, 3.25, 8.0, 7.0), None, p, group=0), Entry(R(6.25, 4.0, 11.5, 7.5), None, q, opacity=0.75, group=0)]
    clip = (R(5.0, 2.5, 10.25, 6.5), None)
    got = cr.render(entries, (Group(0.6, clip),), vp)
    layer = over(A(4.5, 3.25, 8.0, 7.0) * p, (A(6.25, 4.0, 11.5, 7.5) * q) * 0.75)
    want = over(A(3.0, 2.0, 12.0, 8.0) * s, (layer * A(5.0, 2.5, 10.25, 6.5)) * 0.6)
    assert_close64(got, want, atol=1e-12, what="clipped and faded group")
    inside = want[2, 4]   # pixel (4, 7): inside everything
    assert np.allclose(inside, over(s, over(p, q * 0.75) * 0.6), atol=1e-15)
    # (members OVER one another first, then the clip: not each member clipped on its own)
    each = over(over(A(3.0, 2.0, 12.0, 8.0) * s, A(4.5, 3.25, 8.0, 7.0) * p * A(5.0, 2.5, 10.25, 6.5) * 0.6),
                A(6.25, 4.0, 11.5, 7.5) * q * 0.75 * A(5.0, 2.5, 10.25, 6.5) * 0.6)
    assert np.abs(each - want).max() > 1e-3
    # the group's clip lies outside the viewport: the group is invisible, the background is untouched
    got = cr.render(entries, (Group(0.6, (R(20.0, 20.0, 25.0, 25.0), None)),), vp, clamp=True)
    assert_close64(got, A(3.0, 2.0, 12.0, 8.0) * s, atol=1e-12, what="group whose clip misses the viewport")


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_no_coverage_near_the_cut(case):
    """`mask < 1e-6 -> 0` (S:990) is the one place where the order of a sum may flip a pixel.  It is asked of Path.mask only -- of
    every path and every clip source; the products of the sequence (fill, IN, opacity, OVER) are not cut again -- so a case whose
    raw coverages all stay 1e-9 away from it needs no allowance on the device."""
    for _kind, _idx, d, rule in cc.paths_of(case):
        raw = cr.raw_coverage(d, rule, case.viewport)
        if raw is None:
            continue
        assert (np.abs(raw - cr.CUT) > 1e-9).all(), f"{case.name}: coverage within 1e-9 of the cut: {d}"
        cut = np.where(raw < cr.CUT, 0.0, raw)
        got, bb = cr.mask_layer(d, rule, case.viewport)
        r0, c0 = bb[0] - case.viewport[0], bb[1] - case.viewport[1]
        assert np.array_equal(got[r0:r0 + bb[2], c0:c0 + bb[3]], cut)


def _path(case, kind, idx):
    for k, i, d, rule in cc.paths_of(case):
        if (k, i) == (kind, idx):
            return d, rule
    raise KeyError((kind, idx))


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_named_layouts_hold(case):
    for kind, idx, band, ct, cls in case.layout:
        d, rule = _path(case, kind, idx)
        assert cc.cell_class(d, rule, case.viewport, band, ct) == cls, f"{case.name}: {kind} {idx} in tile ({band}, {ct})"
    for kind, idx, band, half in case.halves:
        d, rule = _path(case, kind, idx)
        _m, bb = cr.mask_layer(d, rule, case.viewport)
        # (the layer's margin row above / below the shape may fall into the neighbouring band: what counts is this band's rows)
        band0 = case.viewport[0] + band * cc.TR
        r_lo, r_hi = max(bb[0], band0), min(bb[0] + bb[2], band0 + cc.TR)
        assert r_lo < r_hi and band0 + half * cc.HALF <= r_lo and r_hi <= band0 + (half + 1) * cc.HALF, \
            f"{case.name}: {kind} {idx} leaves half {half} of band {band}"
    for (band, ct), count in case.items:
        n = sum(cc.cell_class(d, rule, case.viewport, band, ct) != 0 for _k, _i, d, rule in cc.paths_of(case))
        assert n == count, f"{case.name}: {n} items in tile ({band}, {ct})"
    # members of a group are consecutive entries, and every tile under test lies inside the viewport
    seen = []
    for e in case.entries:
        if e.group is not None and (not seen or seen[-1] != e.group):
            assert e.group not in seen
            seen.append(e.group)
    assert seen == list(range(len(case.groups)))
    for band, ct in case.tiles:
        assert band * cc.TR < case.viewport[2] and ct * cc.TC < case.viewport[3]
        assert cc.nontrivial(case, cr.render(case.entries, case.groups, case.viewport), band, ct), f"{case.name}: tile ({band}, {ct})"


def test_the_case_list_is_what_it_says():
    names = set(cc.IDS)
    assert len(names) == len(cc.IDS)
    for origin in cc.ORIGINS:
        assert origin == (0, 0) or (origin[0] % cc.TR and origin[1] % cc.TC)
        tag = "o%d_%d" % origin
        for form in ("plain", "clip", "groups", "gradient"):
            for n in cc.DEEP_COUNTS:
                assert f"deep_{form}_{n}-{tag}" in names
    for case in cc.CASES:
        assert case.viewport[2] <= 96 and case.viewport[3] <= 320 and len(cc.paths_of(case)) <= 130
    # the deep groups hold a group open across the round boundary: members 60 .. 70 of 130, 60 .. 64 of 65
    for case in cc.CASES:
        if case.name.startswith("deep_groups_130") or case.name.startswith("deep_groups_65"):
            at = [n for n, (k, i, _d, _r) in enumerate(cc.paths_of(case)) if k == "entry" and case.entries[i].group == 0]
            assert at[0] == 60 and at[-1] == (70 if "130" in case.name else 64) and at[0] < cc.ROUND <= at[-1]
        if case.name.startswith("deep_clip_130") or case.name.startswith("deep_clip_65"):
            kinds = [k for k, _i, _d, _r in cc.paths_of(case)]
            assert kinds[cc.ROUND - 1] == "clip" and kinds[cc.ROUND] == "entry"   # the pair sits astride the round boundary
    # the direct description is used only where the scene walk cannot express the case
    assert 0 < sum(cc.is_direct(c) for c in cc.CASES) < len(cc.CASES) // 4
    spreads = {e.paint.spread for c in cc.CASES for e in c.entries if isinstance(e.paint, cr.Grad)}
    assert spreads == {"pad", "repeat", "reflect"}
