"""Variable fonts: the ``fvar`` / ``avar`` / ``gvar`` tables of a ``truetype.TrueTypeFont`` and its instances.

Host code, pure Python + numpy, with the discipline of ``truetype.py``: every offset, length and count is checked against the
data, nothing is allocated by a size a field claims, a malformed table raises ``ValueError("truetype: ...")`` that says which
-- when the font is read (``fvar``, ``avar``, the ``gvar`` header) or, for a glyph's variation data, when that glyph is first
used.  The per-point work -- the stored or interpolated delta of every point in every tuple, summed -- is done on the device
(``_abi.gvar_deltas`` / ``_abi.glyf_outline_var``, svgr_gvar.h); DESIGN.md, "Variable fonts", has the definitions.

Read: ``fvar`` (the axes: tag, minimum, default, maximum; named instances are skipped over), ``avar`` version 1 (version 2 warns
once per font and its map is not applied), ``gvar`` version 1 (short and long offsets, shared tuples, embedded peaks,
intermediate regions, shared and private point numbers, "all points", every run form of packed points and deltas).  A font
with ``fvar`` and no ``gvar`` has axes, and its instances draw the default outline.

Not read: ``HVAR`` / ``VVAR`` / ``MVAR`` / ``STAT`` / ``cvar``, CFF2, named instances.  The advance of an instance comes from the
phantom points of ``gvar``.  Nothing is rounded to integers: neither the varied points nor the advances.
"""
from __future__ import annotations

import collections
import math
import warnings

import numpy as np

from . import _abi
from .truetype import TrueTypeFont, _need, _unpack

Axis = collections.namedtuple("Axis", "tag minimum default maximum")

_SHARED_POINTS, _COUNT_MASK = 0x8000, 0x0FFF
_EMBEDDED_PEAK, _INTERMEDIATE, _PRIVATE_POINTS, _TUPLE_INDEX_MASK = 0x8000, 0x4000, 0x2000, 0x0FFF
_POINTS_WORDS, _POINT_RUN_MASK = 0x80, 0x7F
_DELTAS_ZERO, _DELTAS_WORDS, _DELTA_RUN_MASK = 0x80, 0x40, 0x3F


class Tuple:
    """One tuple of a glyph's variation data: `peak`, `start`, `end` (per axis; `start` and `end` None without an intermediate
    region), `index` (int32, increasing point numbers, the four phantom points included) and `dxy` (n, 2) int16."""

    __slots__ = ("peak", "start", "end", "index", "dxy")

    def __init__(self, peak, start, end, index, dxy):
        self.peak, self.start, self.end, self.index, self.dxy = peak, start, end, index, dxy


class Variations:
    """What `read_variations` found: `axes`, `maps` (per axis the ``avar`` segment map as ``[(from, to)]``, or None), and of
    ``gvar`` the shared tuples and the glyphs' data offsets (`gvar` None: no outline variation)."""

    __slots__ = ("axes", "maps", "gvar", "shared", "offsets", "data_at", "glyphs")

    def __init__(self, axes, maps):
        self.axes, self.maps = axes, maps
        self.gvar = self.shared = self.offsets = self.data_at = None
        self.glyphs = {}   # glyph id -> [Tuple], decoded on first use


# ----------------------------------------------------------------------------------------------------------------------
# the definitions that run on the host: normalisation and the scalar of a tuple
# ----------------------------------------------------------------------------------------------------------------------
def normalise(axis: Axis, segment_map, value: float) -> float:
    """The normalised coordinate of the user value `value` on `axis`: clamped, scaled to [-1, 1] around the default, through the
    ``avar`` map, rounded to F2Dot14."""
    v = min(max(float(value), axis.minimum), axis.maximum)
    if v == axis.default:
        n = 0.0
    elif v < axis.default:
        n = (v - axis.default) / (axis.default - axis.minimum)
    else:
        n = (v - axis.default) / (axis.maximum - axis.default)
    if segment_map:
        for (ka, va), (kb, vb) in zip(segment_map, segment_map[1:]):
            if n == ka:
                n = va
                break
            if ka < n <= kb:
                n = va + (vb - va) * (n - ka) / (kb - ka)
                break
    return math.floor(n * 16384 + 0.5) / 16384


def scalar(tuple_, coords) -> float:
    """How much of a tuple's deltas the instance at the normalised `coords` takes: the product over the axes, in axis order."""
    s = 1.0
    for a, n in enumerate(coords):
        peak = tuple_.peak[a]
        if peak == 0:
            continue
        if n == peak:
            continue
        if tuple_.start is None:
            if n == 0 or n < min(0.0, peak) or n > max(0.0, peak):
                return 0.0
            s *= n / peak
        else:
            start, end = tuple_.start[a], tuple_.end[a]
            if start > peak or peak > end or (start < 0 < end):   # (OpenType: such a region is ignored, the axis does not count)
                continue
            if n <= start or n >= end:
                return 0.0
            s *= (n - start) / (peak - start) if n < peak else (end - n) / (end - peak)
    return s


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def read_variations(font: TrueTypeFont):
    """The `Variations` of a font with an ``fvar`` table, None for a static font."""
    tables, data = font.tables, font.data
    if "fvar" not in tables:
        return None
    off, length = tables["fvar"]
    fvar = data[off:off + length]
    _major, _minor, axes_at, _reserved, n_axes, axis_size = _unpack(">HHHHHH", fvar, 0, "fvar")
    if axis_size < 20:
        raise ValueError(f"truetype: fvar: an axis record of {axis_size} bytes")
    axes = []
    for a in range(n_axes):
        tag, lo, default, hi = _unpack(">4siii", fvar, axes_at + a * axis_size, "fvar: axis record")
        lo, default, hi = lo / 65536.0, default / 65536.0, hi / 65536.0
        if not lo <= default <= hi:
            raise ValueError(f"truetype: fvar: axis {tag!r} with minimum {lo}, default {default}, maximum {hi}")
        axes.append(Axis(tag.decode("latin-1"), lo, default, hi))
    if not axes:
        return None
    maps = [None] * n_axes
    if "avar" in tables:
        off, length = tables["avar"]
        avar = data[off:off + length]
        major, _minor, _reserved, count = _unpack(">HHHH", avar, 0, "avar")
        if major == 2:
            warnings.warn(f"truetype: {font.family}: avar version 2 is not read, its map is not applied")
        elif major != 1:
            raise ValueError(f"truetype: avar: version {major}")
        else:
            if count != n_axes:
                raise ValueError(f"truetype: avar: {count} axes where fvar has {n_axes}")
            at = 8
            for a in range(n_axes):
                n_pairs, = _unpack(">H", avar, at, "avar: segment map")
                at += 2
                _need(avar, at, 4 * n_pairs, "avar: segment map")
                pairs = [(k / 16384.0, v / 16384.0) for k, v in zip(*[iter(_unpack(f">{2 * n_pairs}h", avar, at, "avar: segment map"))] * 2)]
                at += 4 * n_pairs
                if any(b[0] <= a_[0] for a_, b in zip(pairs, pairs[1:])):
                    raise ValueError("truetype: avar: a segment map whose from-coordinates do not increase")
                maps[a] = pairs or None
    var = Variations(tuple(axes), maps)
    if "gvar" in tables:
        _read_gvar_header(font, var)
    return var


def _read_gvar_header(font, var) -> None:
    off, length = font.tables["gvar"]
    gvar = font.data[off:off + length]
    major, _minor, n_axes, n_shared, shared_at, n_glyphs, flags, data_at = _unpack(">HHHHIHHI", gvar, 0, "gvar")
    if major != 1:
        raise ValueError(f"truetype: gvar: version {major}")
    if n_axes != len(var.axes):
        raise ValueError(f"truetype: gvar: axisCount {n_axes} where fvar has {len(var.axes)}")
    if n_glyphs != font.n_glyphs:
        raise ValueError(f"truetype: gvar: glyphCount {n_glyphs} where maxp has {font.n_glyphs}")
    if flags & 1:
        _need(gvar, 20, 4 * (n_glyphs + 1), "gvar: offsets")
        offsets = np.frombuffer(gvar, dtype=">u4", count=n_glyphs + 1, offset=20).astype(np.int64)
    else:
        _need(gvar, 20, 2 * (n_glyphs + 1), "gvar: offsets")
        offsets = np.frombuffer(gvar, dtype=">u2", count=n_glyphs + 1, offset=20).astype(np.int64) * 2
    if (np.diff(offsets) < 0).any() or data_at + int(offsets[-1]) > len(gvar):
        raise ValueError("truetype: gvar: the offsets decrease or leave the table")
    _need(gvar, shared_at, 2 * n_axes * n_shared, "gvar: shared tuples")
    shared = [tuple(v / 16384.0 for v in _unpack(f">{n_axes}h", gvar, shared_at + 2 * n_axes * k, "gvar: shared tuples")) for k in range(n_shared)]
    var.gvar, var.shared, var.offsets, var.data_at = gvar, shared, offsets, data_at


def _packed_points(data, at: int):
    """(None for "all points" or the list of point numbers, the position behind them)."""
    _need(data, at, 1, "gvar: point count")
    count = data[at]
    at += 1
    if count == 0:
        return None, at
    if count & _POINTS_WORDS:
        _need(data, at, 1, "gvar: point count")
        count = ((count & _POINT_RUN_MASK) << 8) | data[at]
        at += 1
    out, value = [], 0
    while len(out) < count:
        _need(data, at, 1, "gvar: point run")
        control = data[at]
        at += 1
        run = (control & _POINT_RUN_MASK) + 1
        if len(out) + run > count:
            raise ValueError("truetype: gvar: a point run beyond the point count")
        if control & _POINTS_WORDS:
            diffs = _unpack(f">{run}H", data, at, "gvar: point run")
            at += 2 * run
        else:
            diffs = _unpack(f">{run}B", data, at, "gvar: point run")
            at += run
        for d in diffs:
            value += d
            out.append(value)
    return out, at


def _packed_deltas(data, at: int, count: int):
    """(`count` deltas, the position behind them)."""
    out = []
    while len(out) < count:
        _need(data, at, 1, "gvar: delta run")
        control = data[at]
        at += 1
        run = (control & _DELTA_RUN_MASK) + 1
        if len(out) + run > count:
            raise ValueError("truetype: gvar: a delta run beyond the point count")
        if control & _DELTAS_ZERO:
            out.extend([0] * run)
        elif control & _DELTAS_WORDS:
            out.extend(_unpack(f">{run}h", data, at, "gvar: delta run"))
            at += 2 * run
        else:
            out.extend(_unpack(f">{run}b", data, at, "gvar: delta run"))
            at += run
    return out, at


def glyph_tuples(font: TrueTypeFont, gid: int) -> list:
    """The tuples of glyph `gid`, decoded on first use: point numbers increasing, a repeated one keeping its later delta, one at
    or beyond the glyph's point count + 4 (the phantom points) dropped, "all points" spelled out."""
    var = font._var
    if var is None or var.gvar is None or not 0 <= gid < font.n_glyphs:
        return []
    got = var.glyphs.get(gid)
    if got is None:
        got = var.glyphs[gid] = _decode_glyph(font, var, gid)
    return got


def _decode_glyph(font, var, gid) -> list:
    begin, end = int(var.offsets[gid]), int(var.offsets[gid + 1])
    if begin == end:
        return []
    data = var.gvar[var.data_at + begin:var.data_at + end]   # (every read below is checked against the glyph's own data)
    n_axes, n_all = len(var.axes), font.point_count(gid) + 4
    count, data_at = _unpack(">HH", data, 0, "gvar: glyph variation data")
    shared_points = bool(count & _SHARED_POINTS)
    count &= _COUNT_MASK
    at = 4
    headers = []
    for _ in range(count):
        size, index = _unpack(">HH", data, at, "gvar: tuple header")
        at += 4
        if index & _EMBEDDED_PEAK:
            peak = tuple(v / 16384.0 for v in _unpack(f">{n_axes}h", data, at, "gvar: tuple header"))
            at += 2 * n_axes
        else:
            if (index & _TUPLE_INDEX_MASK) >= len(var.shared):
                raise ValueError(f"truetype: gvar: glyph {gid} names shared tuple {index & _TUPLE_INDEX_MASK} of {len(var.shared)}")
            peak = var.shared[index & _TUPLE_INDEX_MASK]
        start = stop = None
        if index & _INTERMEDIATE:
            both = [v / 16384.0 for v in _unpack(f">{2 * n_axes}h", data, at, "gvar: tuple header")]
            at += 4 * n_axes
            start, stop = tuple(both[:n_axes]), tuple(both[n_axes:])
        headers.append((size, bool(index & _PRIVATE_POINTS), peak, start, stop))
    if at > data_at:
        raise ValueError(f"truetype: gvar: the tuple headers of glyph {gid} run into its data")
    at = data_at
    shared = None
    if shared_points:
        shared, at = _packed_points(data, at)
    out = []
    for size, private, peak, start, stop in headers:
        _need(data, at, size, "gvar: tuple data")
        own = data[at:at + size]
        at += size
        points, p = _packed_points(own, 0) if private else (shared, 0)
        if points is None:
            points = range(n_all)
        dx, p = _packed_deltas(own, p, len(points))
        dy, p = _packed_deltas(own, p, len(points))
        kept: dict = {}
        for point, x, y in zip(points, dx, dy):   # (point numbers never decrease: the differences are unsigned)
            if point < n_all:
                kept[point] = (x, y)
        out.append(Tuple(peak, start, stop, np.fromiter(kept, dtype=np.int32, count=len(kept)),
                         np.array(list(kept.values()), dtype=np.int16).reshape(-1, 2)))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# instances
# ----------------------------------------------------------------------------------------------------------------------
def coordinates(font: TrueTypeFont, coords=None, axes=None):
    """(user values clamped, normalised coordinates), both per axis in ``fvar`` order, of ``{tag: value}`` given as `coords`
    and / or `axes`; an axis not named stays at its default.  A tag the font does not have raises ``ValueError``."""
    var = font._var
    wanted = dict(coords or {})
    wanted.update(axes or {})
    tags = [axis.tag for axis in font.axes]
    for tag in wanted:
        if tag not in tags:
            raise ValueError(f"truetype: {font.family} has no axis {tag!r}" + (f" (it has {', '.join(tags)})" if tags else " (it is not a variable font)"))
    user, normal = [], []
    for axis, segment_map in zip(font.axes, var.maps if var else ()):
        v = float(wanted.get(axis.tag, axis.default))
        if not math.isfinite(v):
            raise ValueError(f"truetype: axis {axis.tag!r}: {v} is not a position")
        v = min(max(v, axis.minimum), axis.maximum)
        user.append(v)
        normal.append(normalise(axis, segment_map, v))
    return tuple(user), tuple(normal)


def instance(font: TrueTypeFont, coords=None, axes=None):
    """``TrueTypeFont.instance``: the font itself with every axis at its default, else the `TrueTypeInstance` of the normalised
    coordinates, made once."""
    user, normal = coordinates(font, coords, axes)
    if all(v == axis.default for v, axis in zip(user, font.axes)):
        return font
    made = font._instances.get(normal)
    if made is None:
        made = font._instances[normal] = TrueTypeInstance(font, user, normal)
    return made


def live_tuples(font: TrueTypeFont, gid: int, normal) -> list:
    """``[(scalar, Tuple)]`` of glyph `gid` at the normalised coordinates: the tuples whose scalar is not 0, in the file's order."""
    out = []
    for t in glyph_tuples(font, gid):
        s = scalar(t, normal)
        if s != 0.0:
            out.append((s, t))
    return out


def tuple_arrays(font: TrueTypeFont, gids, normal) -> dict:
    """The tuple arguments of ``_abi.gvar_deltas`` / ``_abi.glyf_outline_var`` for an atlas of the simple glyphs `gids`: phantom
    entries stripped, tuples that touch no point of the outline left out."""
    glyph_tuple_off, scalars, tuple_pt_off, index, dxy = [0], [], [0], [], []
    for gid in gids:
        n = font.point_count(gid)
        for s, t in live_tuples(font, gid, normal):
            real = int(np.searchsorted(t.index, n))   # (the phantom points, n .. n + 3, come last)
            if real == 0:
                continue
            scalars.append(s)
            index.append(t.index[:real])
            dxy.append(t.dxy[:real])
            tuple_pt_off.append(tuple_pt_off[-1] + real)
        glyph_tuple_off.append(len(scalars))
    return dict(glyph_tuple_off=np.array(glyph_tuple_off, dtype=np.int32), tuple_scalar=np.array(scalars, dtype=np.float64),
                tuple_pt_off=np.array(tuple_pt_off, dtype=np.int32),
                tp_index=np.concatenate(index) if index else np.zeros(0, np.int32),
                tp_dxy=np.concatenate(dxy) if dxy else np.zeros((0, 2), np.int16))


def point_sums(font: TrueTypeFont, gid: int, normal, points) -> list:
    """``[(sum of scalar * dx, sum of scalar * dy)]`` of the point numbers `points` of glyph `gid`, an untouched one taking 0: the
    host's arithmetic for phantom points and for the components of a composite glyph (no interpolation)."""
    sums = [[0.0, 0.0] for _ in points]
    for s, t in live_tuples(font, gid, normal):
        for k, point in enumerate(points):
            at = int(np.searchsorted(t.index, point))
            if at < len(t.index) and int(t.index[at]) == point:
                sums[k][0] = sums[k][0] + s * float(t.dxy[at, 0])
                sums[k][1] = sums[k][1] + s * float(t.dxy[at, 1])
    return [tuple(v) for v in sums]


class TrueTypeInstance(TrueTypeFont):
    """One instance of a variable font (``TrueTypeFont.instance``): `parent`, `coords` ``{tag: user value}`` and `normalised`
    (per axis).  It shares the parsed tables and the decoded glyphs with its parent and keeps its own varied parts, advances
    and glyph objects."""

    __slots__ = ["parent", "coords", "normalised", "_advances"]

    def __init__(self, parent: TrueTypeFont, user, normal):   # (not TrueTypeFont's: nothing is parsed again)
        for name in ("data", "tables", "n_glyphs", "advances", "loca", "_cmap", "_simple", "_composite", "_var", "_instances",
                     "family", "style", "ascent", "descent", "units_per_em", "hkern"):
            setattr(self, name, getattr(parent, name))
        self.parent, self.normalised = parent, tuple(normal)
        self.coords = {axis.tag: v for axis, v in zip(parent.axes, user)}
        self.weight = int(math.floor(self.coords["wght"] + 0.5)) if "wght" in self.coords else parent.weight
        self.glyphs, self._parts, self._by_gid, self._advances = {}, {}, {}, {}
        self._warned_matching = True   # (the parent warns)
        self.missing_glyph = self.glyph(0, None)

    def instance(self, coords=None, **axes):
        return self.parent.instance(coords, **axes)

    def advance(self, gid: int) -> float:
        """The ``hmtx`` advance plus the difference of the deltas of the glyph's second and first phantom point, unrounded."""
        got = self._advances.get(gid)
        if got is None:
            got = self._advances[gid] = self.parent.advance(gid) + self._phantom(gid)
        return got

    def _phantom(self, gid: int) -> float:
        if not 0 <= gid < self.n_glyphs:
            return 0.0
        n, total = self.parent.point_count(gid), 0.0
        for s, t in live_tuples(self.parent, gid, self.normalised):
            d = [0.0, 0.0]
            for k, point in enumerate((n, n + 1)):
                at = int(np.searchsorted(t.index, point))
                if at < len(t.index) and int(t.index[at]) == point:
                    d[k] = float(t.dxy[at, 0])
            total = total + s * (d[1] - d[0])
        return total

    def _components(self, gid: int):
        return self.parent._components(gid)

    def _placed_components(self, gid: int):
        components = self.parent._components(gid)
        if components is None:
            return None
        sums = point_sums(self.parent, gid, self.normalised, range(len(components)))
        return [(child, (c00, c01, c10, c11, dx + sx, dy + sy)) for (child, (c00, c01, c10, c11, dx, dy)), (sx, sy) in zip(components, sums)]

    def _outline_call(self, atlas_gids, args):
        return _abi.glyf_outline_var(**args, **tuple_arrays(self.parent, atlas_gids, self.normalised))

    def __repr__(self) -> str:
        where = ", ".join(f"{tag}={value:g}" for tag, value in self.coords.items())
        return f'TrueTypeInstance(family="{self.family}", {where})'
