"""SVG markers (``marker-start`` / ``marker-mid`` / ``marker-end``, SVG 2 11.6; beyond the reference): the ``Marker`` a
``<marker>`` element describes, and the payload of a MARKERS scene node, which turns into one instance of a marker's content per
vertex of its path.  The vertices and their directions come from the device (``Path.vertices``, svgr_path_markers), so the node
stays as it is until something draws or walks it: building one -- loading a document -- needs no device."""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from .geometry import PATH_CLOSED, PATH_LINE, Path, Transform

ORIENT_AUTO = "auto"
ORIENT_AUTO_START_REVERSE = "auto-start-reverse"


@dataclass(frozen=True, eq=False)
class Marker:
    """What a ``<marker>`` element says.  `scene`: its content (None: empty); `ref` = (refX, refY) in content coordinates;
    `size` = (markerWidth, markerHeight); `viewbox` = (x, y, w, h) or None; `orient`: None (0), degrees, ``"auto"`` or
    ``"auto-start-reverse"``; `units_stroke_width`: the marker's coordinate system is scaled by the stroke width; `clip`: the
    content is clipped to the marker's viewport (``overflow`` hidden)."""

    scene: "tuple | None"
    ref: tuple = (0.0, 0.0)
    size: tuple = (3.0, 3.0)
    viewbox: "tuple | None" = None
    preserve_aspect_ratio: str = "xMidYMid meet"
    units_stroke_width: bool = True
    orient: "float | str | None" = None
    clip: bool = True

    def placed(self):
        """``(content, (sx, sy))``: the content, clipped to the viewport unless `clip` is off, and the scale of the viewBox
        mapping; None when the marker draws nothing (no content, a zero markerWidth or markerHeight, an empty viewBox).  The
        viewport is (0, 0, markerWidth, markerHeight) and the viewBox is fitted into it by `preserve_aspect_ratio`; since
        (refX, refY) is then moved onto the vertex, only the scale of that mapping reaches an instance's matrix, and its
        translation only the clip rectangle."""
        from .scene import Scene, image_placement  # noqa: PLC0415

        mw, mh = (float(v) for v in self.size)
        if self.scene is None or not (mw > 0 and mh > 0):
            return None
        if self.viewbox is None:
            sx = sy = 1.0
            tx = ty = 0.0
        else:
            vx, vy, vw, vh = (float(v) for v in self.viewbox)
            fit = image_placement((vh, vw), 0.0, 0.0, mw, mh, self.preserve_aspect_ratio)
            if fit is None:
                return None
            m = fit[0].m
            sx, sy = float(m[0, 0]), float(m[1, 1])
            tx, ty = float(m[0, 2]) - sx * vx, float(m[1, 2]) - sy * vy
        content = self.scene
        if self.clip:   # the viewport in content coordinates, as a nested <svg> clips
            x0, y0, x1, y1 = (0.0 - tx) / sx, (0.0 - ty) / sy, (mw - tx) / sx, (mh - ty) / sy
            frame = [(PATH_LINE, [[x0, y0], [x1, y0]]), (PATH_LINE, [[x1, y0], [x1, y1]]), (PATH_LINE, [[x1, y1], [x0, y1]]),
                     (PATH_CLOSED, [[x0, y1], [x0, y0]])]
            content = content.clip(Scene.fill(Path([frame]), np.ones(4)))
        return content, (sx, sy)

    def instance_transform(self, scale, x: float, y: float, ux: float, uy: float, stroke_width: float, at_start: bool) -> Transform:
        """From content coordinates to the path's user space for the vertex (x, y) with the unit direction (ux, uy): translate
        to the vertex, rotate (by the direction for ``auto``, by its opposite for ``auto-start-reverse`` at the start vertex,
        else by the fixed angle), scale by the stroke width (`units_stroke_width`) and by the viewBox mapping's `scale`, and
        move (refX, refY) onto the origin."""
        if self.orient in (ORIENT_AUTO, ORIENT_AUTO_START_REVERSE):
            c, s = (-ux, -uy) if at_start and self.orient == ORIENT_AUTO_START_REVERSE else (ux, uy)
        else:
            angle = math.radians(float(self.orient or 0.0))
            c, s = math.cos(angle), math.sin(angle)
        k = float(stroke_width) if self.units_stroke_width else 1.0
        return Transform().translate(x, y).matrix(c, -s, 0, s, c, 0).scale(k * scale[0], k * scale[1]).translate(-float(self.ref[0]), -float(self.ref[1]))


class Symbol(NamedTuple):
    """What a ``<symbol>`` element says (beyond the reference).  `scene`: its content in the symbol's own coordinates (None:
    empty); `viewbox` = (x, y, w, h) or None; `x`, `y`, `width`, `height`: the symbol's own (None: not given); `clip`: the
    content is clipped to the viewport (``overflow`` neither ``visible`` nor ``auto``)."""

    scene: "tuple | None"
    viewbox: "tuple | None" = None
    preserve_aspect_ratio: str = "xMidYMid meet"
    x: float = 0.0
    y: float = 0.0
    width: "float | None" = None
    height: "float | None" = None
    clip: bool = True

    def viewport(self, width=None, height=None):
        """``(width, height)`` of the viewport an instance gets: the <use>'s `width` / `height`, else the symbol's own, else
        the viewBox's size (a deviation: SVG says 100 %, which needs a viewport that is not known when a document loads);
        None for each that none of them gives."""
        box = (None, None) if self.viewbox is None else self.viewbox[2:]
        return tuple(next((float(v) for v in (given, own, fallback) if v is not None), None)
                     for given, own, fallback in ((width, self.width, box[0]), (height, self.height, box[1])))

    def instance(self, x: float = 0.0, y: float = 0.0, width=None, height=None):
        """What a ``<use>`` at (`x`, `y`) with `width` / `height` (None: not given) draws: the content under one transform --
        the translation by (`x`, `y`) and the symbol's own ``x`` / ``y``, times the fit of the viewBox into the viewport
        (``scene.image_placement``, the mapping a <marker> uses) -- and, unless `clip` is off, clipped to the viewport, a
        rectangle in content coordinates as a nested <svg>'s frame is.  Without a viewBox the content is not scaled; without
        any size it is not clipped.  None when nothing is drawn (no content, an empty viewport or viewBox)."""
        from .scene import Scene, image_placement  # noqa: PLC0415

        if self.scene is None:
            return None
        w, h = self.viewport(width, height)
        if (w is not None and not w > 0) or (h is not None and not h > 0):
            return None
        content, place = self.scene, Transform().translate(float(x) + float(self.x or 0.0), float(y) + float(self.y or 0.0))
        sx = sy = 1.0
        tx = ty = 0.0
        if self.viewbox is not None:
            vx, vy, vw, vh = (float(v) for v in self.viewbox)
            fit = image_placement((vh, vw), 0.0, 0.0, w, h, self.preserve_aspect_ratio)
            if fit is None:
                return None
            m = fit[0].m
            sx, sy = float(m[0, 0]), float(m[1, 1])
            tx, ty = float(m[0, 2]) - sx * vx, float(m[1, 2]) - sy * vy
            place = place.translate(float(m[0, 2]), float(m[1, 2])).scale(sx, sy).translate(-vx, -vy)
        if self.clip and w is not None and h is not None:
            x0, y0, x1, y1 = (0.0 - tx) / sx, (0.0 - ty) / sy, (w - tx) / sx, (h - ty) / sy
            frame = [(PATH_LINE, [[x0, y0], [x1, y0]]), (PATH_LINE, [[x1, y0], [x1, y1]]), (PATH_LINE, [[x1, y1], [x0, y1]]),
                     (PATH_CLOSED, [[x0, y1], [x0, y0]])]
            content = content.clip(Scene.fill(Path([frame]), np.ones(4)))
        return content.transform(place)


class MarkerInstances:
    """Payload of a MARKERS node: the path, its three markers (None: none) and the stroke width.  `expand()` makes the instances
    once -- ordinary TRANSFORM nodes over the markers' content, in vertex order, as one GROUP -- and keeps them in `scene`
    (None before, and when nothing is drawn)."""

    __slots__ = ("path", "start", "mid", "end", "stroke_width", "scene", "_expanded", "_lock")

    def __init__(self, path: Path, start=None, mid=None, end=None, stroke_width: float = 1.0):
        self.path, self.start, self.mid, self.end = path, start, mid, end
        self.stroke_width = float(stroke_width)
        self.scene = None
        self._expanded = False
        self._lock = threading.Lock()

    def expand(self):
        """The GROUP of instances (a single instance: that node); None when there is none."""
        if not self._expanded:
            with self._lock:
                if not self._expanded:
                    self.scene = self._instances()
                    self._expanded = True
        return self.scene

    def _instances(self):
        from .scene import Scene  # noqa: PLC0415

        by_kind = [m if m is None else (m, m.placed()) for m in (self.start, self.mid, self.end)]
        if all(m is None or m[1] is None for m in by_kind):
            return None
        xy, direction, kind = self.path.vertices()
        out = []
        for (x, y), (ux, uy), k in zip(xy.tolist(), direction.tolist(), kind.tolist()):
            entry = by_kind[k]
            if entry is None or entry[1] is None:
                continue
            marker, (content, scale) = entry
            out.append(content.transform(marker.instance_transform(scale, x, y, ux, uy, self.stroke_width, k == 0)))
        return Scene.group(out) if out else None
