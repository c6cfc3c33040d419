"""Directed cases for the tile kernel's CLIP, GROUPS and GRAD variants: where a clip source, a clipped path, a group or a gradient
lies relative to the 16 x 64 tile grid and to the 8-row halves the two waves of a workgroup own.

Positions are in TILE UNITS from the viewport's origin -- `rect(b0, t0, b1, t1)` spans bands b0 .. b1 (16 rows each) and column
tiles t0 .. t1 (64 columns each) -- because the tile grid starts at the viewport's first pixel: every case is built once at origin
(0, 0) and once at an origin that is a multiple of neither 16 nor 64, with the same layout in the grid.  Negative positions hang out
of the viewport to the left / top.  The viewports' sizes are no multiple of the tile either: the last band and the last column tile
are cut.

A case names its layout: `layout` rows (which path, band, column tile, cell class) and `halves` rows (which path, band, which wave's
rows its layer keeps to); tests/test_canvas_ref_host.py checks them from the geometry.  `items`: paths with a cell in a deep tile."""
from __future__ import annotations

import re
from typing import NamedTuple

import numpy as np

from tests.canvas_ref import Entry, Grad, Group, edges_of, mask_layer

TR, TC = 16, 64            # the tile: rows per band, columns per column tile (svgr_tile_rows / svgr_tile_cols)
HALF = TR // 2             # rows of a tile one wave owns
ORIGINS = ((0, 0), (-7, 83))
VIEW = (61, 250)           # directed cases: 4 bands x 4 column tiles, the last of each cut
DEEP_VIEW = (35, 180)      # deep tiles: 3 bands x 3 column tiles
DEEP_TILE = (1, 1)
DEEP_COUNTS = (1, 2, 3, 4, 23, 24, 25, 26, 63, 64, 65, 130)   # (23 .. 26: on either side of the 24 items a tile's page holds)
ROUND = 64                 # items per round of the tile kernel's list

_A = (0.55, 0.8, 0.4, 0.65, 0.9, 0.35, 0.7, 0.5)
_RGB = ((0.9, 0.2, 0.1), (0.1, 0.7, 0.3), (0.2, 0.3, 0.95), (0.8, 0.75, 0.1), (0.6, 0.1, 0.7), (0.1, 0.8, 0.8), (0.95, 0.5, 0.2), (0.4, 0.4, 0.45))
PAINTS = tuple(np.array([r * a, g * a, b * a, a]) for (r, g, b), a in zip(_RGB, _A))   # premultiplied
FAINT = np.array([0.03, 0.06, 0.09, 0.15])


class Case(NamedTuple):
    name: str
    entries: tuple
    groups: tuple
    viewport: tuple           # (r0, c0, rows, cols)
    tiles: tuple              # (band, column tile) under test: the reference must be non-trivial there
    layout: tuple = ()        # (kind, index, band, column tile, class): kind "entry" / "clip" (entry's leaf clip) / "gclip" (group's clip)
    halves: tuple = ()        # (kind, index, band, half): the path's layer has rows in that half of the band only (0: rows 0-7, 1: rows 8-15)
    items: tuple = ()         # ((band, column tile), count): paths with a cell in that tile


class Geo:
    """Path data at an origin, positions in tile units."""

    def __init__(self, origin):
        self.r, self.c = origin

    def y(self, b):
        return self.r + b * TR

    def x(self, t):
        return self.c + t * TC

    def rect(self, b0, t0, b1, t1):
        x0, y0, x1, y1 = self.x(t0), self.y(b0), self.x(t1), self.y(b1)
        return f"M{x0!r},{y0!r} H{x1!r} V{y1!r} H{x0!r} Z"

    def ring(self, b0, t0, b1, t1, hb0, ht0, hb1, ht1):
        """A rectangle and a rectangle inside it: a hole under the even-odd rule."""
        return self.rect(b0, t0, b1, t1) + " " + self.rect(hb0, ht0, hb1, ht1)

    def blob(self, b, t, rb, rt):
        """Four cubics around (b, t), radii rb bands / rt column tiles, lopsided so that no edge is axis-aligned."""
        cx, cy, rx, ry = self.x(t), self.y(b), rt * TC, rb * TR
        k = 0.61
        p = [(cx + rx, cy + 0.1 * ry), (cx + rx, cy + k * ry), (cx + k * rx, cy + ry), (cx - 0.1 * rx, cy + ry),
             (cx - 0.7 * rx, cy + ry), (cx - rx, cy + 0.5 * ry), (cx - rx, cy - 0.15 * ry),
             (cx - rx, cy - 0.8 * ry), (cx - 0.4 * rx, cy - ry), (cx + 0.2 * rx, cy - ry),
             (cx + 0.8 * rx, cy - ry), (cx + rx, cy - 0.5 * ry), (cx + rx, cy + 0.1 * ry)]
        f = lambda q: f"{q[0]!r},{q[1]!r}"
        return f"M{f(p[0])} " + " ".join(f"C{f(p[i])} {f(p[i + 1])} {f(p[i + 2])}" for i in range(1, 13, 3)) + " Z"

    def pt(self, b, t):
        return (self.x(t), self.y(b))


_RECT = re.compile(r"M(\S+),(\S+) H(\S+) V(\S+) H(\S+) Z")


def rects_of(d):
    """[(x0, y0, x1, y1)] when the path data is made of `Geo.rect` subpaths only, else None."""
    found = _RECT.findall(d)
    if not found or _RECT.sub("", d).strip():
        return None
    return [(float(x0), float(y0), float(x1), float(y1)) for x0, y0, x1, y1, _ in found]


def tile_box(viewport, band, ct):
    """(r0, c0, r1, c1) of a tile, absolute, not cut by the viewport."""
    return viewport[0] + band * TR, viewport[1] + ct * TC, viewport[0] + (band + 1) * TR, viewport[1] + (ct + 1) * TC


def cell_class(d, rule, viewport, band, ct):
    """The class of the path's cell in a tile, from the geometry (the CellHdr comment): 2 when an edge with a row extent lies in the
    tile's rows and columns, 1 when none does and some row's carry-in is visible there (the coverage, constant along each row, is
    not zero), else 0.  An edge that only touches the tile's first or last column is refused: the case has to say which it means."""
    r0, c0, r1, c1 = tile_box(viewport, band, ct)
    r1, c1 = min(r1, viewport[0] + viewport[2]), min(c1, viewport[1] + viewport[3])
    e = edges_of(d)
    rlo, rhi = e[:, :, 0].min(axis=1), e[:, :, 0].max(axis=1)
    clo, chi = e[:, :, 1].min(axis=1), e[:, :, 1].max(axis=1)
    rows = (rhi > rlo) & (rhi > r0) & (rlo < r1)
    assert not (rows & ((chi == c0) | (clo == c1))).any(), "an edge on the tile's border: ambiguous layout"
    if (rows & (chi > c0) & (clo < c1)).any():
        return 2
    m, _ = mask_layer(d, rule, viewport)
    return 1 if m[r0 - viewport[0]: r1 - viewport[0], c0 - viewport[1]: c1 - viewport[1]].any() else 0


def nontrivial(case, canvas, band, ct):
    """The reference canvas holds, in that tile, an alpha that is neither 0 nor the alpha of a paint of the case."""
    a = canvas[band * TR: (band + 1) * TR, ct * TC: (ct + 1) * TC, 3].ravel()
    plain = [0.0] + [float(e.paint[3]) for e in case.entries if not isinstance(e.paint, Grad)]
    return bool((np.abs(a[:, None] - np.array(plain)[None, :]).min(axis=1) > 1e-9).any())


def paths_of(case):
    """Every path of the case in batch order: [(kind, index, path data, rule)] -- a clip source sits right in front of the leaf /
    of the first member it clips."""
    out, seen = [], set()
    for i, e in enumerate(case.entries):
        if e.group is not None and e.group not in seen:
            seen.add(e.group)
            g = case.groups[e.group]
            if g.clip is not None:
                out.append(("gclip", e.group, g.clip[0], g.clip[1]))
        if e.clip is not None:
            out.append(("clip", i, e.clip[0], e.clip[1]))
        out.append(("entry", i, e.d, e.rule))
    return out


def _stops(*idx):
    n = len(idx)
    return tuple((k / (n - 1) if n > 1 else 0.0, PAINTS[i]) for k, i in enumerate(idx))


def _background(g, view):
    """A blob over most of the viewport with slanted stripes cut out of it (even-odd): partial coverage in every tile, so that a
    tile in which everything else must come out as nothing still holds values that are neither 0 nor a plain paint."""
    b, t = view[0] / TR, view[1] / TC
    d = g.blob(0.49 * b, 0.5 * t, 0.47 * b, 0.48 * t)
    y0, y1 = g.y(-0.2), g.y(b + 0.2)
    for k in range(int(view[1] / 37.9) + 2):
        x = g.x(0) - 20.7 + 37.9 * k
        d += f" M{x!r},{y0!r} L{x + 6.4!r},{y0!r} L{x + 31.7!r},{y1!r} L{x + 25.3!r},{y1!r} Z"
    return Entry(d, "evenodd", PAINTS[7])


# --------------------------------------------------------------------------------------------------------------------------------
# clip pairs (a leaf clip = SVGR_PATH_CLIP_SOURCE then SVGR_PATH_CLIPPED), no groups
# --------------------------------------------------------------------------------------------------------------------------------
def _clip_cases(g, view):
    bg = _background(g, view)
    prime = lambda b, t, i: Entry(g.rect(b + 0.1, t + 0.1, b + 0.9, t + 0.9), None, PAINTS[i], clip=(g.rect(b - 0.3, t - 0.3, b + 1.3, t + 1.3), None))
    yield ("clip_source_class1", (
        bg,
        Entry(g.rect(1.2, 2.15, 1.83, 2.77), None, PAINTS[0], clip=(g.rect(0.5, 1.6, 2.5, 3.4), None)),
        Entry(g.blob(1.5, 2.5, 0.4, 0.35), "evenodd", PAINTS[1], clip=(g.rect(0.45, 1.55, 2.45, 3.45), None)),
    ), (), dict(tiles=((1, 2),), layout=(("clip", 1, 1, 2, 1), ("entry", 1, 1, 2, 2), ("clip", 2, 1, 2, 1), ("entry", 2, 1, 2, 2))))
    yield ("clip_clipped_class1", (
        bg,
        Entry(g.rect(0.5, 1.6, 2.5, 3.4), None, PAINTS[2], clip=(g.blob(1.5, 2.5, 0.42, 0.4), None)),
        Entry(g.rect(0.55, 1.65, 2.45, 3.35), None, PAINTS[3], clip=(g.rect(1.2, 2.15, 1.83, 2.77), "evenodd")),
    ), (), dict(tiles=((1, 2),), layout=(("entry", 1, 1, 2, 1), ("clip", 1, 1, 2, 2), ("entry", 2, 1, 2, 1), ("clip", 2, 1, 2, 2))))
    # the second pair's source lives in tile (3, 0) only; in tile (1, 2) the clip tile still holds the first pair's source
    yield ("clip_source_absent_stale_tile", (
        bg,
        Entry(g.rect(1.1, 2.1, 1.9, 2.9), None, PAINTS[4], clip=(g.rect(0.6, 1.7, 2.4, 3.3), None)),
        Entry(g.rect(1.15, 0.2, 3.6, 2.85), None, PAINTS[0], clip=(g.rect(3.1, 0.3, 3.7, 0.9), None)),
    ), (), dict(tiles=((1, 2), (3, 0)), layout=(("clip", 1, 1, 2, 1), ("clip", 2, 1, 2, 0), ("entry", 2, 1, 2, 2), ("clip", 2, 3, 0, 2))))
    yield ("clip_second_source_smaller", (
        bg,
        Entry(g.rect(1.05, 2.05, 1.95, 2.95), None, PAINTS[1], clip=(g.rect(0.6, 1.7, 2.4, 3.3), None)),
        Entry(g.rect(1.08, 2.08, 1.92, 2.92), None, PAINTS[5], clip=(g.rect(1.3, 2.3, 1.7, 2.6), None)),
        Entry(g.blob(1.5, 2.5, 0.45, 0.45), None, PAINTS[6], clip=(g.blob(1.45, 2.4, 0.2, 0.18), None)),
    ), (), dict(tiles=((1, 2),), layout=(("clip", 1, 1, 2, 1), ("clip", 2, 1, 2, 2), ("entry", 2, 1, 2, 2))))
    # per tile: a pair whose source fills the clip tile, then the pair under test.  Layers reach one row past the shape on either
    # side (the bbox's margin): a shape within rows 0.8 .. 6.4 of a band keeps to rows 0 .. 7, one within 9.6 .. 15.2 to rows 8 .. 15
    lo, hi, full = (0.05, 0.4), (0.6, 0.95), (0.08, 0.93)
    ent, hv = [bg], []
    for (b, t), src, tgt, i in (((0, 0), lo, full, 0), ((0, 2), hi, full, 1), ((2, 0), full, lo, 2), ((2, 2), full, hi, 3)):
        ent.append(prime(b, t, i + 3))
        ent.append(Entry(g.rect(b + tgt[0], t + 0.15, b + tgt[1], t + 0.85), None, PAINTS[i],
                         clip=(g.rect(b + src[0], t + 0.2, b + src[1], t + 0.8), None)))
        for kind, span in (("clip", src), ("entry", tgt)):
            if span is not full:
                hv.append((kind, len(ent) - 1, b, 0 if span is lo else 1))
    yield ("clip_wave_halves", tuple(ent), (), dict(tiles=((0, 0), (0, 2), (2, 0), (2, 2)), halves=tuple(hv)))
    yield ("clip_straddles_tiles_evenodd_hole", (
        bg,
        Entry(g.blob(2.0, 2.0, 0.9, 0.45), None, PAINTS[2], clip=(g.ring(1.4, 1.5, 2.6, 2.5, 1.8, 1.8, 2.2, 2.2), "evenodd")),
    ), (), dict(tiles=((1, 1), (1, 2), (2, 1), (2, 2)), layout=tuple(("clip", 1, b, t, 2) for b in (1, 2) for t in (1, 2))))
    yield ("clip_source_outside_viewport", (
        Entry(g.blob(0.8, 0.8, 0.9, 0.7), None, PAINTS[7]),
        Entry(g.rect(-0.5, -0.5, 1.5, 1.5), None, PAINTS[0], clip=(g.rect(-2.0, -1.5, -0.6, -0.3), None)),
        Entry(g.blob(0.3, 0.3, 0.5, 0.4), None, PAINTS[1], clip=(g.rect(-0.6, -0.4, 0.7, 0.8), None)),
        Entry(g.rect(0.2, 0.1, 0.9, 0.6), None, PAINTS[2], clip=(g.blob(-0.1, 0.2, 0.6, 0.5), None)),
    ), (), dict(tiles=((0, 0),), layout=(("clip", 1, 0, 0, 0), ("entry", 1, 0, 0, 1), ("clip", 2, 0, 0, 2))))


# --------------------------------------------------------------------------------------------------------------------------------
# isolated groups
# --------------------------------------------------------------------------------------------------------------------------------
def _members(g, b, t, gid, n=2, first=0):
    """`n` overlapping members inside tile (b, t): rectangles with fractional edges, every third a blob."""
    out = []
    for k in range(n):
        s = 0.06 * k
        if k % 3 == 2:
            out.append(Entry(g.blob(b + 0.5, t + 0.45 + s, 0.3, 0.25), "evenodd", PAINTS[(first + k) % 8], group=gid))
        else:
            out.append(Entry(g.rect(b + 0.12 + s, t + 0.1 + 2 * s, b + 0.7 + s, t + 0.62 + 2 * s), None, PAINTS[(first + k) % 8],
                             opacity=0.8 if k % 2 else None, group=gid))
    return out


def _group_cases(g, view):
    bg = _background(g, view)
    prime = lambda b, t, i: Entry(g.rect(b + 0.1, t + 0.1, b + 0.9, t + 0.9), None, PAINTS[i], clip=(g.rect(b - 0.3, t - 0.3, b + 1.3, t + 1.3), None))
    # closing: (0, 2) a group, then a plain path; (2, 0) a group, then another group; (2, 2) a group, then a clip pair;
    # (0, 0) a group as the last items of the tile's list (and of the batch)
    yield ("group_closing", (
        bg,
        *_members(g, 0, 2, 0, 3), Entry(g.blob(0.55, 2.5, 0.35, 0.3), None, PAINTS[4]),
        *_members(g, 2, 0, 1, 2, 2), *_members(g, 2, 0, 2, 3, 5),
        *_members(g, 2, 2, 3, 2, 1), Entry(g.rect(2.2, 2.2, 2.8, 2.8), None, PAINTS[6], clip=(g.blob(2.5, 2.5, 0.25, 0.3), None)),
        *_members(g, 0, 0, 4, 3, 3),
    ), (Group(0.5), Group(0.7), Group(1.0, (g.blob(2.5, 0.5, 0.4, 0.35), None)), Group(0.8), Group(0.6)),
        dict(tiles=((0, 0), (0, 2), (2, 0), (2, 2))))
    yield ("group_opacity_or_clip", (
        bg,
        *_members(g, 0, 0, 0, 2), *_members(g, 0, 2, 1, 2, 3), *_members(g, 2, 0, 2, 3, 5),
    ), (Group(0.45), Group(1.0, (g.rect(0.3, 2.2, 0.8, 2.7), "evenodd")), Group(0.55)), dict(tiles=((0, 0), (0, 2), (2, 0))))
    # both together; a single member under both; a single member under an opacity alone
    # (a GROUP of one child is that child to the scene walk: single-member groups exist in the direct description only)
    yield ("group_opacity_and_clip", (
        bg,
        *_members(g, 0, 0, 0, 3), *_members(g, 0, 2, 1, 1, 3), *_members(g, 2, 2, 2, 1, 4),
    ), (Group(0.45, (g.blob(0.5, 0.5, 0.4, 0.4), None)), Group(0.7, (g.rect(0.3, 2.2, 0.8, 2.7), None)), Group(0.55)),
        dict(tiles=((0, 0), (0, 2), (2, 2))))
    # group 0: members in tiles (1..3, 1..3), its clip source in tile (3, 3) only, no clip tile written before in (1, 1);
    # group 1: members in band 0, its clip source in tile (0, 3) only, after a pair that filled the clip tile of (0, 0)
    yield ("group_clip_absent", (
        bg,
        Entry(g.rect(1.1, 1.1, 1.9, 1.9), None, PAINTS[0], group=0), Entry(g.blob(1.5, 1.5, 0.4, 0.4), None, PAINTS[1], group=0),
        Entry(g.rect(1.2, 1.2, 3.5, 3.5), None, PAINTS[2], group=0),
        prime(0, 0, 3),
        Entry(g.rect(0.2, 0.2, 0.8, 0.8), None, PAINTS[4], group=1), Entry(g.rect(0.3, 0.3, 0.7, 3.6), None, PAINTS[5], group=1),
    ), (Group(1.0, (g.rect(3.05, 3.05, 3.8, 3.8), None)), Group(1.0, (g.rect(0.1, 3.1, 0.9, 3.8), None))),
        dict(tiles=((1, 1), (3, 3), (0, 0), (0, 3)),
             layout=(("gclip", 0, 1, 1, 0), ("entry", 1, 1, 1, 2), ("gclip", 0, 3, 3, 2), ("gclip", 1, 0, 0, 0), ("entry", 5, 0, 0, 2),
                     ("clip", 4, 0, 0, 1), ("gclip", 1, 0, 3, 2))))
    # tile (0, 0): only the first member has a cell; tile (0, 3): only the last; tile (2, 1): the clip source and no member
    yield ("group_member_cells", (
        bg,
        Entry(g.rect(0.3, 0.3, 0.8, 0.8), None, PAINTS[0], group=0), Entry(g.blob(1.5, 2.0, 0.45, 0.6), None, PAINTS[1], group=0),
        Entry(g.rect(0.25, 3.1, 0.9, 3.7), None, PAINTS[2], group=0),
    ), (Group(1.0, (g.rect(0.2, 0.2, 2.8, 3.8), None)),),
        dict(tiles=((0, 0), (0, 3), (2, 1), (1, 2)),
             layout=(("entry", 1, 0, 0, 2), ("entry", 2, 0, 0, 0), ("entry", 3, 0, 0, 0), ("entry", 1, 0, 3, 0), ("entry", 2, 0, 3, 0),
                     ("entry", 3, 0, 3, 2), ("gclip", 0, 2, 1, 1), ("entry", 1, 2, 1, 0), ("entry", 2, 2, 1, 0), ("entry", 3, 2, 1, 0))))
    # after a pair that filled the clip tile: (1, 1) group clip in rows 8-15, members in rows 0-7; (3, 1) the other way round;
    # (1, 3) group clip in rows 8-15, members in all rows
    lo, hi = (0.05, 0.4), (0.6, 0.95)
    ent, hv = [bg], []
    clips = []
    for gid, ((b, t), src, tgt) in enumerate((((1, 1), hi, lo), ((3, 1), lo, hi), ((1, 3), hi, (0.08, 0.93)))):
        ent.append(prime(b, t, gid + 3))
        for k in range(2):
            ent.append(Entry(g.rect(b + tgt[0] + 0.02 * k, t + 0.2 + 0.1 * k, b + tgt[1] - 0.02 * k, t + 0.7 + 0.1 * k), None, PAINTS[gid + k], group=gid))
            if tgt in (lo, hi):
                hv.append(("entry", len(ent) - 1, b, 0 if tgt is lo else 1))
        clips.append(Group(1.0, (g.rect(b + src[0], t + 0.15, b + src[1], t + 0.85), None)))
        hv.append(("gclip", gid, b, 0 if src is lo else 1))
    yield ("group_wave_halves", tuple(ent), tuple(clips), dict(tiles=((1, 1), (3, 1), (1, 3)), halves=tuple(hv)))
    many = []
    for k in range(20):
        b0, t0 = 1.05 + 0.04 * k, 1.1 + 0.035 * k
        d = g.ring(b0, t0, b0 + 0.9, t0 + 0.8, b0 + 0.2, t0 + 0.15, b0 + 0.6, t0 + 0.5) if k % 5 != 4 else g.blob(b0 + 0.4, t0 + 0.4, 0.4, 0.4)
        many.append(Entry(d, "evenodd" if k % 2 else None, PAINTS[k % 8], opacity=(0.5 + 0.02 * k) if k % 3 == 0 else None, group=0))
    yield ("group_of_twenty", (bg, *many), (Group(1.0, (g.blob(1.8, 1.8, 0.8, 0.7), None)),), dict(tiles=((1, 1), (2, 2), (1, 2), (2, 1))))


# --------------------------------------------------------------------------------------------------------------------------------
# gradients
# --------------------------------------------------------------------------------------------------------------------------------
def _grads(g):
    lin_pad = Grad("linear", "pad", _stops(0, 1, 2, 3), p0=g.pt(0.41, 0.33), p1=g.pt(2.53, 2.21))
    rad_rep = Grad("radial", "repeat", _stops(4, 5, 6), center=g.pt(2.43, 2.71), radius=23.7)
    # the focal point outside the end circle: det < 0 outside the cone
    focal = Grad("radial", "reflect", _stops(1, 3, 5, 0), center=g.pt(1.07, 3.03), radius=19.3, fcenter=g.pt(1.93, 3.41), fradius=2.9)
    th = 0.37
    gt = ((1.3 * np.cos(th), -0.8 * np.sin(th), 3.1), (1.3 * np.sin(th), 0.8 * np.cos(th), -2.3), (0.0, 0.0, 1.0))
    lin_gt = Grad("linear", "reflect", _stops(2, 6, 0), p0=g.pt(2.9, 0.2), p1=g.pt(3.3, 0.9), gt=gt)
    return lin_pad, rad_rep, focal, lin_gt


def _grad_cases(g, view):
    bg = _background(g, view)
    lin_pad, rad_rep, focal, lin_gt = _grads(g)
    yield ("gradient_kinds", (
        bg,
        Entry(g.rect(0.3, 0.2, 2.7, 2.4), None, lin_pad),
        Entry(g.rect(1.2, 1.6, 3.6, 3.8), None, rad_rep),
        Entry(g.blob(1.0, 3.0, 0.9, 0.8), "evenodd", focal),
        Entry(g.rect(2.6, 0.1, 3.7, 1.4), None, lin_gt, opacity=0.85),
    ), (), dict(tiles=((1, 1), (2, 2), (0, 3), (3, 0)), layout=(("entry", 1, 1, 1, 1), ("entry", 2, 2, 2, 1))))
    yield ("gradient_in_clipped_faded_group", (
        bg,
        Entry(g.rect(0.6, 0.7, 2.6, 2.9), None, lin_pad, group=0), Entry(g.blob(1.6, 1.7, 0.7, 0.8), None, PAINTS[4], opacity=0.7, group=0),
        Entry(g.blob(1.9, 2.3, 0.8, 0.6), "evenodd", rad_rep, opacity=0.9, group=0),
    ), (Group(0.65, (g.blob(1.6, 1.8, 0.9, 0.95), None)),), dict(tiles=((1, 1), (1, 2), (2, 2)), layout=(("entry", 1, 1, 1, 1),)))
    yield ("gradient_leaf_clip_and_opacity", (
        bg,
        Entry(g.rect(0.4, 2.3, 1.9, 3.8), None, focal, opacity=0.6, clip=(g.blob(1.1, 3.0, 0.6, 0.6), None)),
        Entry(g.rect(1.7, 0.4, 3.4, 2.6), None, rad_rep, opacity=0.75, clip=(g.ring(1.9, 0.6, 3.2, 2.4, 2.3, 1.2, 2.8, 1.8), "evenodd")),
    ), (), dict(tiles=((0, 3), (1, 2), (2, 1))))


# --------------------------------------------------------------------------------------------------------------------------------
# deep tiles: one tile with N items, for the four variants
# --------------------------------------------------------------------------------------------------------------------------------
def _deep_shape(g, i):
    b, t = DEEP_TILE
    if i % 16 == 5:   # the whole tile, faintly: a class-1 cell among the class-2 ones
        return g.rect(b - 0.3, t - 0.4, b + 1.3, t + 1.4), None, FAINT
    if i % 10 == 3:
        return g.blob(b + 0.5, t + 0.3 + (i * 0.07) % 0.4, 0.3, 0.22), ("evenodd" if i % 4 == 3 else None), PAINTS[i % 8]
    b0, t0 = b + 0.05 + (i * 0.37) % 0.55, t + 0.03 + (i * 0.53) % 0.6
    return g.rect(b0, t0, b0 + 0.3 + (i % 3) * 0.04, t0 + 0.2 + (i % 5) * 0.03), None, PAINTS[i % 8]


def _deep(g, form, n):
    b, t = DEEP_TILE
    ent = [Entry(*_deep_shape(g, i)) for i in range(n)]
    groups, items, layout, tiles = (), n, (), (DEEP_TILE,)
    if form == "clip":
        if n == 1:   # the source never reaches the deep tile: the clipped path is its only item, and invisible there
            ent = [Entry(g.rect(0.3, 0.3, b + 0.9, t + 0.9), None, PAINTS[0], clip=(g.rect(0.1, 0.1, 0.8, 0.8), None))]
            layout, tiles = (("clip", 0, b, t, 0), ("entry", 0, b, t, 2)), ((0, 0),)
        else:        # the source is the last item of a round and the clipped path the first of the next when the list is that long
            at = ROUND - 1 if n > ROUND else n - 2
            ent = ent[:at] + [Entry(g.rect(b + 0.1, t + 0.1, b + 0.9, t + 0.9), None, PAINTS[3], clip=(g.blob(b + 0.5, t + 0.5, 0.42, 0.4), None))] + ent[at + 2:]
    elif form == "groups":
        if n > 70:    # a clip source as item 59, its group's members items 60 .. 70: open across the round boundary
            ent = ent[:59] + [e._replace(group=0) for e in ent[60:71]] + ent[71:]
            groups = (Group(1.0, (g.blob(b + 0.5, t + 0.5, 0.42, 0.42), None)),)
        elif n > ROUND:   # members 60 .. 64: open across the round boundary, closed by the end of the list
            ent = ent[:60] + [e._replace(group=0) for e in ent[60:]]
            groups = (Group(0.6),)
        else:
            k = min(3, n)
            ent = ent[:n - k] + [e._replace(group=0) for e in ent[n - k:]]
            groups = (Group(0.6),)
    elif form == "gradient":
        at = n // 2
        e = ent[at]
        ent[at] = e._replace(paint=Grad("linear", "reflect", _stops(1, 4, 6), p0=g.pt(b + 0.13, t + 0.21), p1=g.pt(b + 0.47, t + 0.52)),
                             opacity=0.9 if n % 2 else None)
    return tuple(ent), groups, dict(tiles=tiles, items=((DEEP_TILE, items),), layout=layout)


def _all():
    out = []
    for origin in ORIGINS:
        g = Geo(origin)
        tag = "o%d_%d" % origin
        for name, entries, groups, kw in (*_clip_cases(g, VIEW), *_group_cases(g, VIEW), *_grad_cases(g, VIEW)):
            out.append(Case(f"{name}-{tag}", tuple(entries), tuple(groups), (*origin, *VIEW), **kw))
        for form in ("plain", "clip", "groups", "gradient"):
            for n in DEEP_COUNTS:
                entries, groups, kw = _deep(g, form, n)
                out.append(Case(f"deep_{form}_{n}-{tag}", entries, groups, (*origin, *DEEP_VIEW), **kw))
    return out


CASES = _all()
IDS = [c.name for c in CASES]


# --------------------------------------------------------------------------------------------------------------------------------
# device batches
# --------------------------------------------------------------------------------------------------------------------------------
def _paint_object(S, paint):
    if not isinstance(paint, Grad):
        return np.asarray(paint, dtype=np.float64)
    stops = [(float(o), np.asarray(c, dtype=np.float64)) for o, c in paint.stops]
    tr = None if paint.gt is None else S.Transform(np.asarray(paint.gt, dtype=np.float64))
    if paint.kind == "linear":
        return S.GradLinear(np.asarray(paint.p0, float), np.asarray(paint.p1, float), stops, tr, paint.spread, False, None)
    return S.GradRadial(np.asarray(paint.center, float), float(paint.radius), None if paint.fcenter is None else np.asarray(paint.fcenter, float),
                        paint.fradius, stops, tr, paint.spread, False, None)


def is_direct(case):
    """The scene walk cannot express the case: a group under a clip AND an opacity (kept node by node), under neither, or with a
    single member (a GROUP of one child is that child).  Such a case is described to _abi.Batch directly."""
    for gi, grp in enumerate(case.groups):
        if (grp.clip is None) == (grp.opacity == 1.0) or sum(e.group == gi for e in case.entries) < 2:
            return True
    return False


def scene_of(S, case):
    """The case as a Scene: a FILL per entry under its OPACITY and CLIP, the members of a group as a GROUP under its CLIP or
    OPACITY (one of the two: the scene walk keeps a group with both node by node)."""
    source = lambda clip: S.Scene.fill(S.Path.from_svg(clip[0]), np.zeros(4), clip[1])

    def leaf(e):
        node = S.Scene.fill(S.Path.from_svg(e.d), _paint_object(S, e.paint), e.rule)
        if e.opacity is not None:
            node = node.opacity(e.opacity)
        return node if e.clip is None else node.clip(source(e.clip))

    nodes, i = [], 0
    while i < len(case.entries):
        e = case.entries[i]
        if e.group is None:
            nodes.append(leaf(e))
            i += 1
            continue
        j = i
        while j < len(case.entries) and case.entries[j].group == e.group:
            j += 1
        grp, node = case.groups[e.group], S.Scene.group([leaf(m) for m in case.entries[i:j]])
        nodes.append(node.opacity(grp.opacity) if grp.clip is None else node.clip(source(grp.clip)))
        i = j
    return S.Scene.group(nodes)


def expected_leaves(case):
    """(flags, group index or None) per batch entry: what the scene walk must make of the case."""
    flags = {"gclip": 1, "clip": 1}
    out = []
    for kind, idx, _d, _rule in paths_of(case):
        e = case.entries[idx] if kind == "entry" else None
        out.append((flags.get(kind, 2 if (e is not None and e.clip is not None) else 0), e.group if e is not None else None))
    return out


def build_batch(S, case, ctx):
    """The planned-to-be batch of a case: through Scene -> _batchable_leaves -> build_batch (the leaves are checked against the
    case: the Python plumbing is under test too), or, for what the scene walk cannot express, _abi.Batch + set_groups /
    set_gradients."""
    from svgrasterize_amd import _abi
    from svgrasterize_amd import scene as sm

    swap = S.Transform().matrix(0, 1, 0, 1, 0, 0)
    if not is_direct(case):
        leaves = sm._batchable_leaves(scene_of(S, case), swap, True)
        assert leaves is not None, case.name
        want = expected_leaves(case)
        assert [leaf[4] for leaf in leaves] == [f for f, _ in want], case.name
        tags = {}
        got_groups = [None if leaf[5] is None else tags.setdefault(leaf[5][0], len(tags)) for leaf in leaves]
        want_tags = {}
        assert got_groups == [None if gi is None else want_tags.setdefault(gi, len(want_tags)) for _, gi in want], case.name
        assert [leaf[6] is not None for leaf in leaves] == [k == "entry" and isinstance(case.entries[i].paint, Grad) for k, i, _d, _r in paths_of(case)]
        return sm.build_batch(leaves, list(case.viewport), ctx)
    paths = paths_of(case)
    packs = [S.Path.from_svg(d).packed() for _k, _i, d, _r in paths]
    offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in packs])]).astype(np.int64)
    rules, paints, path_group, path_grad, grads, keep = [], [], [], [], [], []
    group_src = [-1] * len(case.groups)
    for at, (kind, idx, _d, rule) in enumerate(paths):
        e = case.entries[idx] if kind == "entry" else None
        flag = 1 if e is None else (2 if e.clip is not None else 0)
        rules.append((1 if rule == "evenodd" else 0) | (flag << 1))
        path_group.append(-1 if e is None or e.group is None else e.group)
        if kind == "gclip":
            group_src[idx] = at
        mult = 1.0 if e is None or e.opacity is None else e.opacity
        if e is not None and isinstance(e.paint, Grad):
            gs, k = _paint_object(S, e.paint).abi(swap.invert, True)
            path_grad.append(len(grads))
            grads.append(gs)
            keep.append(k)
            paints.append(np.ones(4) * mult)
        else:
            path_grad.append(-1)
            paints.append(np.zeros(4) if e is None else np.asarray(e.paint, dtype=np.float64) * mult)
    batch = _abi.Batch(ctx, np.concatenate([p[0] for p in packs]), np.concatenate([p[1] for p in packs]), offs,
                       np.tile(swap.m6(), (len(paths), 1)), rules, np.array(paints), viewport=list(case.viewport))
    if case.groups:
        batch.set_groups(path_group, group_src, [g.opacity for g in case.groups])
    if grads:
        batch.set_gradients(path_grad, grads)
    del keep
    return batch
