"""A scene that is batch entries and nothing else, compiled ONCE to flat arrays ("Scene -> (once, Python) arrays").

`Scene.render` (S:649-752) walks the tree on every call; what the walk finds out about a document made of solid fills, strokes,
transforms, single-path clips and opacity / clip groups -- which leaves there are, in which order, with which rule, flags and
isolated group -- does not depend on the render transform at all.  Only the leaves' matrices do: `transform @ A @ B ...` down the
chain of TRANSFORM nodes above each leaf.  This module keeps the transform-independent part per scene object.  It has no analysis
of its own: `scene._batchable_leaves_` runs with the transform left symbolic (`_Symbolic`), and the walk's `_drop_empty`, packing
and window code work on the result as they do on the walk's leaves.  A render of such a scene is

    chain products (stacked 3x3 matmuls, level by level: the same BLAS call on the same operands in the same association as the
    walk's `Transform.__matmul__` -- bit-identical, checked in tests/test_displaylist.py) -> `_abi.Batch` -> plan -> window -> Layer

instead of ~2 000 Python frames of tree walk and ~10 000 small-array operations (material-design @4096: 4.7 -> ~1 ms per render).
Scenes with anything else in them (gradients, filters, masks, patterns, objectBoundingBox clips) are not display lists: `compile`
returns None and `Scene.render` takes its general route.

What is kept is keyed by the scene OBJECT (a `Scene` is an immutable tuple tree; the entry holds it, so its id cannot come back as
another scene's) and is transform-, viewport- and device-independent; nothing of a render's RESULT is kept.  Paint arrays are read
again at every render (a colour edited in place is drawn with its new value, as the reference would); path geometry is a value
type here as in the reference (`Path.packed` has kept its packed segments since round 1).
"""
from __future__ import annotations

import threading

import numpy as np

from . import _abi, scene as sc   # (scene.py imports this module inside `Scene._render_top` only)
from .geometry import FLATNESS, Transform, solid_paint

ENABLED = True   # (tests turn the display lists off to compare with the scene walk)
_MAX_ENTRIES = 32
_CACHE: "dict[int, tuple]" = {}     # id(scene) -> (scene, {linear_rgb: DisplayList or None})   (insertion-ordered: oldest first)
_LOCK = threading.Lock()


class DisplayList:
    __slots__ = ("n", "paths", "segs", "kinds", "offs", "rules", "flags", "clipped", "paint_refs", "paint_uniq", "opac", "raw", "paints",
                 "linear_rgb", "path_group", "group_src", "group_op", "leaf_node", "levels", "n_nodes")

    # -- per render ---------------------------------------------------------------------------------------------------------------
    def matrices(self, transform: Transform) -> np.ndarray:
        """(n, 6): every leaf's accumulated matrix `transform @ A @ B ...`, the products made level by level over all chains at once
        (np.matmul on stacked 3x3 matrices calls the BLAS routine `np.dot` calls, per pair: the walk's own bits)."""
        P = np.empty((self.n_nodes, 3, 3), dtype=np.float64)
        P[0] = np.asarray(transform.m, dtype=np.float64)
        for nodes, parents, mats in self.levels:
            P[nodes] = np.matmul(P[parents], mats)
        return np.ascontiguousarray(P[self.leaf_node, :2, :]).reshape(self.n, 6)

    def current_paints(self) -> np.ndarray:
        """(n, 4) paints in the compositing space; converted again only when some paint array changed since the last render."""
        # (the distinct paint OBJECTS are read -- a document's clip sources all share one --, not one array per leaf)
        raw = np.concatenate(self.paint_uniq) if self.paint_uniq else np.zeros(0)
        if self.paints is None or not np.array_equal(raw, self.raw):
            out = np.empty((self.n, 4), dtype=np.float64)
            lin = self.linear_rgb
            for i, (p, o) in enumerate(zip(self.paint_refs, self.opac)):
                if p is sc._ZERO4:   # (a clip source)
                    out[i] = 0.0
                else:
                    c = solid_paint(p, lin)
                    out[i] = c if o is None else c * o   # Layer.opacity over the leaf: image * opacity (S:174)
            self.raw, self.paints = raw, out
        return self.paints

    def render(self, transform: Transform, viewport, linear_rgb: bool):
        """What `Scene._render` returns for this scene: (Layer over the union of the leaves' effective bboxes, lazy hull) or None."""
        if self.n == 0:
            return None
        batch = _abi.Batch(_abi.Context.get(), self.segs, self.kinds, self.offs, self.matrices(transform), self.rules, self.current_paints(),
                           viewport=[int(v) for v in viewport], flatness=FLATNESS)
        try:
            if self.group_src is not None:
                batch.set_groups(self.path_group, self.group_src, self.group_op)
            batch.plan()
            win, in_hull = sc._window_and_hull(self.flags, self.clipped, batch.bboxes())
        except Exception:
            batch.destroy()
            raise
        if win is None:
            batch.destroy()
            return None
        return sc._window_layer(batch, win, in_hull, linear_rgb)


class _Symbolic:
    """The leaf analysis (`scene._batchable_leaves_`) with the render transform left open: a leaf's placement is the chain of
    TRANSFORM matrices above it, a solid leaf's paint (the document's own array, the opacity over it), read again at every
    render; a gradient is not display-list material."""

    step = staticmethod(lambda chain, m: chain + (m,))
    place = staticmethod(lambda chain: chain)
    solid = staticmethod(lambda path, chain, rule, paint, linear_rgb, opacity: (path, chain, rule, (paint, opacity), 0, None, None))
    gradient = staticmethod(lambda *_args: None)


def _compile(scene, linear_rgb: bool):
    """The display list of `scene`, or None when it is not one: the walk's own analysis, tidying and packing
    (`scene._batchable_leaves_`, `_drop_empty`, `_packed_paths`, `_rules_and_groups`) on symbolic leaves, then the chains as a trie."""
    leaves = sc._batchable_leaves_(scene, (), linear_rgb, None, _Symbolic)
    if leaves is None:
        return None
    leaves = sc._drop_empty(leaves)
    dl = DisplayList()
    n = dl.n = len(leaves)
    dl.linear_rgb = bool(linear_rgb)
    dl.paths = [lf[0] for lf in leaves]
    dl.segs, dl.kinds, dl.offs = sc._packed_paths(dl.paths)   # (read-only and shared with the walk's batches of the same paths)
    dl.flags, dl.clipped = sc._leaf_flags(leaves)
    dl.rules, dl.path_group, dl.group_src, dl.group_op = sc._rules_and_groups(leaves)
    pairs = [(lf[3], None) if lf[4] == 1 else lf[3] for lf in leaves]   # (a clip source: `scene._ZERO4`, as in the walk)
    dl.paint_refs = [p for p, _o in pairs]
    dl.paint_uniq = list({id(p): p for p in dl.paint_refs}.values())
    dl.opac = [o for _p, o in pairs]
    dl.raw = dl.paints = None
    # the chains as a trie of prefixes: node 0 = the render transform, a node per distinct (prefix, next matrix object)
    node_of = {(): 0}
    by_level: list = []
    leaf_node = np.zeros(n, dtype=np.int64)
    for i, lf in enumerate(leaves):
        chain = lf[1]
        key = ()
        at = 0
        for d, tr in enumerate(chain):
            key = key + (id(tr),)
            nxt = node_of.get(key)
            if nxt is None:
                nxt = node_of[key] = len(node_of)
                while len(by_level) <= d:
                    by_level.append(([], [], []))
                by_level[d][0].append(nxt)
                by_level[d][1].append(at)
                by_level[d][2].append(np.array(tr.m, dtype=np.float64).reshape(3, 3))
            at = nxt
        leaf_node[i] = at
    dl.leaf_node = leaf_node
    dl.n_nodes = len(node_of)
    dl.levels = [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.stack(c)) for a, b, c in by_level]
    return dl


def get(scene, linear_rgb: bool):
    """The display list of `scene` in this colour space, compiled on first use; None when the scene is not one."""
    if not ENABLED:
        return None
    lin = bool(linear_rgb)
    with _LOCK:
        hit = _CACHE.get(id(scene))
        if hit is not None and hit[0] is scene and lin in hit[1]:
            return hit[1][lin]
    dl = _compile(scene, lin)     # (raises what the walk would raise: an invalid fill rule)
    with _LOCK:
        hit = _CACHE.get(id(scene))
        if hit is None or hit[0] is not scene:
            hit = _CACHE[id(scene)] = (scene, {})
            while len(_CACHE) > _MAX_ENTRIES:
                _CACHE.pop(next(iter(_CACHE)))
        hit[1][lin] = dl
    return dl


def clear() -> None:
    with _LOCK:
        _CACHE.clear()
