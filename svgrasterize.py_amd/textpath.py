"""Text on a path (``<textPath>``, SVG 1.1 10.13; beyond the reference): the payload of a lazily expanded scene node that
holds the referenced path, the runs of text and the offsets, and turns into ordinary FILL / STROKE nodes -- one shape per
run -- when it is first drawn or walked.  The glyphs are placed on the device (``Font.str_on_path``,
svgr_path_place_glyphs) and a percentage ``startOffset`` needs the path's length (``Path.length``), so the node stays as it
is until then: building one -- loading a document -- needs no device.  It rides in the node kind of the markers
(``scene.RENDER_MARKERS``), whose payload only has to offer ``expand()``.  ``TextOutline`` is the same for a straight run set in a
face whose outlines are made on the device (a TrueType or OpenType / CFF font): the run's shapes, made at the first render."""
from __future__ import annotations

import threading
from typing import NamedTuple

import numpy as np

from .geometry import Path

ANCHORS = {None: 0.0, "start": 0.0, "middle": 0.5, "end": 1.0}


class TextRun(NamedTuple):
    """One run of characters: its text, ``Font``, size in user units per em, the attributes its shape is made from, and the
    run's ``dx`` (along the path) and ``dy`` (across it; both stay in force for the runs that follow)."""

    text: str
    font: object
    size: float
    attrs: dict
    dx: float = 0.0
    dy: float = 0.0


def _fill_shape(attrs, path) -> list:
    """The shape of a run without a loader: a fill with ``attrs["fill"]`` (an RGBA array; opaque black without one)."""
    from .scene import Scene  # noqa: PLC0415

    paint = attrs.get("fill")
    return [Scene.fill(path, np.array([0.0, 0.0, 0.0, 1.0]) if paint is None else paint)]


class TextOutline:
    """Payload of a straight run of text whose outline is made on the device (``Scene.text``; the ``str_to_path`` of a
    ``truetype.TrueTypeFont`` or an ``opentype_cff.CFFFont``, of any font for that matter): `font`, `size` in user units per em, `text`, the attributes `attrs` its shape is made from and `shape`:
    ``(attrs, Path) -> [Scene]`` (the loader's; without one a fill with ``attrs["fill"]``).  `expand()` makes the nodes once and
    keeps them in `scene` (None before, and for an empty outline)."""

    __slots__ = ("font", "size", "text", "attrs", "shape", "scene", "_expanded", "_lock")

    def __init__(self, font, size: float, text: str, attrs=None, shape=None):
        self.font, self.size, self.text = font, float(size), text
        self.attrs = {} if attrs is None else dict(attrs)
        self.shape = _fill_shape if shape is None else shape
        self.scene = None
        self._expanded = False
        self._lock = threading.Lock()

    def expand(self):
        """The GROUP of the run's shapes (a single node: that node); None for an empty outline."""
        if not self._expanded:
            with self._lock:
                if not self._expanded:
                    self.scene = self._shapes()
                    self._expanded = True
        return self.scene

    def _shapes(self):
        from .scene import Scene  # noqa: PLC0415

        outline, _advance = self.font.str_to_path(self.size, self.text)
        if not outline.subpaths:
            return None
        out = self.shape(dict(self.attrs), outline)
        return Scene.group(out) if out else None


class TextOnPath:
    """Payload of a text-on-a-path node.  `path`: the referenced path in the user space of the text; `runs`: ``TextRun``s;
    `start_offset`: a length along the path, or a percentage of the path's length with `percent`; `path_length`: the author's
    ``pathLength`` of the path (scales a `start_offset` that is a length); `anchor`: ``start`` / ``middle`` / ``end`` shifts
    the chunk back by 0, 1/2 or 1 of its total advance; `shape`: ``(attrs, Path) -> [Scene]`` (the loader's, so that fill,
    stroke, dashes, opacity and gradients are those of straight text).  `expand()` makes the nodes once and keeps them in
    `scene` (None before, and when nothing is drawn)."""

    __slots__ = ("path", "runs", "start_offset", "percent", "path_length", "anchor", "shape", "scene", "_expanded", "_lock")

    def __init__(self, path: Path, runs, start_offset: float = 0.0, percent: bool = False, path_length: "float | None" = None,
                 anchor: "str | None" = None, shape=None):
        if anchor not in ANCHORS:
            raise ValueError(f"unknown text anchor: `{anchor}`")
        self.path = path
        self.runs = tuple(TextRun(*run) for run in runs)
        self.start_offset, self.percent = float(start_offset), bool(percent)
        self.path_length = None if path_length is None else float(path_length)
        self.anchor = anchor
        self.shape = _fill_shape if shape is None else shape
        self.scene = None
        self._expanded = False
        self._lock = threading.Lock()

    def advance(self) -> float:
        """The chunk's total advance along the path: every run's ``dx`` and set width (host arithmetic)."""
        return sum(run.dx + run.font.str_to_glyphs(run.text)[1] * (run.size / run.font.units_per_em) for run in self.runs)

    def expand(self):
        """The GROUP of the runs' shapes (a single node: that node); None when there is none."""
        if not self._expanded:
            with self._lock:
                if not self._expanded:
                    self.scene = self._shapes()
                    self._expanded = True
        return self.scene

    def _shapes(self):
        from .scene import Scene  # noqa: PLC0415

        if not self.runs:
            return None
        if self.percent or self.path_length is not None:
            length = self.path.length()
            start = length * self.start_offset / 100.0 if self.percent else self.start_offset * (length / self.path_length)
        else:
            start = self.start_offset
        at = start - ANCHORS[self.anchor] * self.advance()
        across, out = 0.0, []
        for run in self.runs:
            at += run.dx
            across += run.dy
            outline, advance = run.font.str_on_path(self.path, run.size, run.text, at, across)
            at += advance
            if outline.subpaths:
                out.extend(self.shape(dict(run.attrs), outline))
        return Scene.group(out) if out else None
