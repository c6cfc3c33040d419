"""Which elements of a loaded document lie under a point (beyond the reference; the DOM's ``elementsFromPoint`` restricted to the
topmost hit region): ``Scene.pick`` finds the region, the loader's ``ids`` table names its owners.

An id OWNS a hit leaf when the leaf's ``source`` object -- the ``Path`` of the FILL or STROKE node the leaf comes from, or the
payload of a lazy marker / text node -- is reachable under ``ids[id]``.  Paths are compared by identity, not nodes: the loader
wraps a node again whenever it groups or transforms it (``Scene.group``, ``Scene.transform``), but the ``Path`` objects are
shared.  So the id of a ``<use>`` and the id of its target both own the shared leaves.
"""
from __future__ import annotations

from .scene import (RENDER_BLEND, RENDER_CLIP, RENDER_FILL, RENDER_FILTER, RENDER_GROUP, RENDER_MARKERS, RENDER_MASK, RENDER_OPACITY,
                    RENDER_STROKE, RENDER_TRANSFORM, Scene)


def reachable_sources(scene: Scene) -> set:
    """``id()`` of every source object under `scene`: the paths of its FILL and STROKE nodes and the payloads of its lazy nodes
    (which are not expanded), looking through every decoration to its target -- a clip's or a mask's own content draws nothing."""
    found, stack = set(), [scene]
    while stack:
        kind, args = stack.pop()
        if kind in (RENDER_FILL, RENDER_STROKE):
            found.add(id(args[0]))
        elif kind == RENDER_MARKERS:
            found.add(id(args))
        elif kind == RENDER_GROUP:
            stack.extend(args)
        elif kind in (RENDER_TRANSFORM, RENDER_OPACITY, RENDER_CLIP, RENDER_MASK, RENDER_FILTER, RENDER_BLEND):
            stack.append(args[0])
        else:
            raise ValueError(f"unhandled scene type: {kind}")
    return found


def owners(ids: dict) -> list:
    """``[(id, sources)]`` of the ids that are scenes, ordered by the number of sources they reach, smallest first (an inner
    element before the groups around it); ties keep the order of `ids`.  Values that are not scenes -- gradients, filters, fonts,
    symbols, the tuples of clipPath and mask -- own nothing and are left out."""
    table = [(name, reachable_sources(value)) for name, value in ids.items() if isinstance(value, Scene)]
    table.sort(key=lambda item: len(item[1]))   # (stable)
    return table


def leaf_owners(leaves, ids: dict) -> list:
    """Per hit leaf of ``Scene.hit_leaves`` the tuple of the ids that own it, innermost first."""
    table = owners(ids)
    return [tuple(name for name, sources in table if id(leaf.source) in sources) for leaf in leaves]


def elements_at(scene: Scene, ids: dict, transform, points) -> list:
    """Per point -- ``(n, 2)`` or a single pair, ``(row, col)`` in the coordinates `transform` maps into -- the tuple of the ids
    that own the topmost hit leaf there, innermost first; ``()`` where nothing is hit.  `scene` and `ids` are what ``svg_scene``
    returned."""
    index, leaves = scene.pick(transform, points)
    names = leaf_owners(leaves, ids)
    return [names[i] if i >= 0 else () for i in index.tolist()]
