"""Small synthetic scenes, one per branch of the leaf analysis (`scene._batchable_leaves_`, `_single_mask_leaf`, `_drop_empty`) that
the scene walk and the display list share: every path three or four segments, every case in a cell of its own so that the cases can
also be drawn side by side (tests/test_displaylist.py).

`cases()` gives (name, verdict, scene).  Verdicts:
  flat      a display list; its arrays are the walk's
  group     the same, with an isolated group in it: not batch entries at all when `scene._BATCH_GROUPS` is off
  refused   no batch entries on either route (`Scene.render` draws it node by node)
  gradient  batch entries for the walk, not a display list
  node      not a display list, and node by node for the walk too
"""
import numpy as np

CELL_X, CELL_Y, COLS = 24.0, 20.0, 6
ORIGIN_X, ORIGIN_Y = 36.0, 4.0   # (the first cells stick out of the viewport the GPU test draws: [8, 40, 80, 144])

RED, BLUE, GREEN, GREY = (np.array(c) for c in ([0.5, 0.0, 0.0, 0.5], [0.0, 0.0, 1.0, 1.0], [0.0, 0.25, 0.0, 0.25], [0.3, 0.3, 0.3, 0.6]))


def cases(host_dashes: bool = False):
    """`host_dashes`: the dashed path is handed its dashes (the dasher runs on the device; the analysis only needs the outline)."""
    import svgrasterize_amd as S
    from svgrasterize_amd import scene as sc

    fill, group, T = S.Scene.fill, S.Scene.group, S.Transform
    tri = lambda x, y, s: S.Path.from_svg(f"M{x},{y} h{s} l{-s},{s} Z")            # noqa: E731  (3 segments)
    sq = lambda x, y, s: S.Path.from_svg(f"M{x},{y} h{s} v{s} h{-s} Z")            # noqa: E731  (4 segments)
    about = lambda x, y, t: T().translate(x, y) @ t @ T().translate(-x, -y)         # noqa: E731
    under = lambda node, t: sc.Scene(sc.RENDER_TRANSFORM, (node, t))                # noqa: E731  (a TRANSFORM node of its own, never merged)
    empty = lambda: S.Path([])                                                      # noqa: E731
    out = []

    def case(name, verdict, make):
        k = len(out)
        out.append((name, verdict, make(ORIGIN_X + (k % COLS) * CELL_X + 2, ORIGIN_Y + (k // COLS) * CELL_Y + 2)))

    def chain(x, y):
        # leaves under (t1, t2, t3), (t1, t2), (t1, t2b), (t1, t2, t3) again as three TRANSFORM nodes right over one leaf, and none
        t1, t2, t2b, t3 = about(x, y, T().scale(0.9)), T().translate(1.5, 0.5), about(x, y, T().rotate(0.1)), about(x, y, T().scale(1.1, 0.8))
        inner = under(group([under(fill(tri(x, y, 6), RED), t3), fill(sq(x + 8, y, 5), BLUE)]), t2)
        stacked = under(under(under(fill(tri(x, y + 9, 5), GREEN), t3), t2), t1)
        return group([under(group([inner, under(fill(sq(x + 8, y + 8, 4), GREY), t2b)]), t1), stacked, fill(tri(x + 15, y + 10, 4), RED)])

    case("chain", "flat", chain)
    case("paint_none", "flat", lambda x, y: group([fill(sq(x, y, 8), None), fill(tri(x + 4, y + 4, 8), BLUE)]))
    case("stroke", "flat", lambda x, y: S.Scene.stroke(tri(x + 1, y + 1, 10), RED, 1.5))

    def dashed(x, y):
        node = S.Scene.stroke(sq(x + 1, y + 1, 10), GREEN, 1.5, dasharray=[4.0, 2.0], dashoffset=1.0)
        if host_dashes:
            node[1][0]._dashed = S.Path.from_svg(f"M{x + 1},{y + 1} h3 M{x + 6},{y + 1} h4 M{x + 11},{y + 2} v4")
        return node

    case("dashed_stroke", "flat", dashed)
    case("opacity_leaf", "flat", lambda x, y: fill(sq(x, y, 9), RED).opacity(0.5))
    case("opacity_leaf_under_transform", "flat", lambda x, y: under(fill(tri(x, y, 9), BLUE), T().translate(2.0, 1.0)).opacity(0.25))
    case("opacity_group", "group", lambda x, y: group([fill(sq(x, y, 8), RED), fill(tri(x + 3, y + 3, 9), BLUE)]).opacity(0.5))
    case("clip_fill_fill", "flat", lambda x, y: fill(sq(x, y, 12), GREY).clip(fill(tri(x + 2, y + 2, 12), RED, "evenodd")))
    case("clip_source_under_transform", "flat",
         lambda x, y: fill(sq(x, y, 12), BLUE).clip(under(under(fill(tri(x, y, 10), RED), about(x, y, T().rotate(0.2))), T().translate(1.0, 2.0))))
    case("clip_stroke", "flat", lambda x, y: S.Scene.stroke(sq(x + 1, y + 1, 9), RED, 2.0).clip(fill(tri(x, y, 14), BLUE)))
    case("clip_faded_leaf", "flat", lambda x, y: fill(sq(x, y, 10), GREEN).opacity(0.5).clip(fill(tri(x + 1, y + 1, 11), BLUE)))
    case("clip_group", "group", lambda x, y: under(group([fill(sq(x, y, 8), RED), fill(tri(x + 4, y + 2, 9), BLUE)]), T().translate(1.0, 0.0)).clip(fill(sq(x + 2, y + 2, 8), GREY)))
    case("clip_of_clipped_leaf", "refused", lambda x, y: fill(sq(x, y, 10), RED).clip(fill(tri(x, y, 10), BLUE)).clip(fill(sq(x + 2, y + 2, 6), BLUE)))
    case("clip_of_unpainted_leaf", "refused", lambda x, y: fill(sq(x, y, 10), None).clip(fill(tri(x, y, 10), BLUE)))
    case("opacity_over_group_with_clip", "refused",
         lambda x, y: group([fill(sq(x, y, 10), RED).clip(fill(tri(x, y, 10), BLUE)), fill(tri(x + 4, y + 4, 6), GREEN)]).opacity(0.5))
    case("two_groups_interleaved", "group", lambda x, y: group([
        fill(tri(x, y, 5), GREY),
        group([fill(sq(x + 2, y, 6), RED), fill(sq(x + 5, y + 2, 6), BLUE)]).opacity(0.5),
        fill(tri(x + 12, y, 5), GREEN),
        group([fill(sq(x, y + 8, 6), BLUE), fill(tri(x + 3, y + 9, 6), RED)]).clip(fill(sq(x + 2, y + 9, 5), GREY)),
        fill(tri(x + 10, y + 8, 5), GREY),
        group([fill(sq(x + 12, y + 6, 5), GREEN), fill(tri(x + 14, y + 8, 5), RED)]).opacity(0.3)]))
    grad = S.GradLinear(np.array([0.0, 0.0]), np.array([10.0, 0.0]), [(0.0, RED), (1.0, BLUE)], None, "pad", False, None)
    case("gradient", "gradient", lambda x, y: group([fill(sq(x, y, 10), grad), fill(tri(x + 6, y + 6, 8), GREEN)]))
    case("clip_bbox_units", "node", lambda x, y: fill(sq(x, y, 12), RED).clip(fill(tri(0.1, 0.1, 0.8), BLUE), bbox_units=True))
    # `_drop_empty`: an empty path as a plain leaf, a clip source, the single clipped leaf, one member and all members of a clipped group
    case("empty_plain", "flat", lambda x, y: group([fill(empty(), RED), fill(tri(x, y, 9), BLUE)]))
    case("empty_clip_source", "flat", lambda x, y: group([fill(tri(x, y, 9), RED).clip(fill(empty(), BLUE)), fill(sq(x + 8, y + 6, 6), GREEN)]))
    case("empty_clipped_leaf", "flat", lambda x, y: group([fill(empty(), RED).clip(fill(tri(x, y, 9), BLUE)), fill(sq(x + 8, y + 6, 6), GREY)]))
    case("empty_group_member", "group",
         lambda x, y: group([group([fill(empty(), RED), fill(tri(x, y, 10), BLUE)]).clip(fill(sq(x + 1, y + 1, 6), GREY)), fill(sq(x + 10, y + 8, 5), RED)]))
    case("empty_group_members_all", "group",
         lambda x, y: group([group([fill(empty(), RED), fill(empty(), BLUE)]).clip(fill(sq(x + 1, y + 1, 6), GREY)), fill(tri(x + 8, y + 6, 7), GREEN)]))
    return out
