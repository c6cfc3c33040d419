"""The renderer as a witness for ``Scene.pick`` / ``Scene.id_map``: the hit walk (scene.py: _hit_walk, _hit_hull) must place every
region where the render walk draws it -- accumulated transforms, the frame of a clip in bounding-box units, clips nested in clip
scenes, stroke outlines with their dashes, expanded markers and text.

Every paintable of a scene gets an opaque flat colour of its own, the scene is rendered into a viewport through the default route,
and ``id_map`` is taken for the same transform and viewport.  A pixel is *decided* when the render alone says so: alpha >= 1 - 1e-9
and the colour within 1e-9 of exactly one paintable's -- the pixel is fully covered by that paintable and touched by nothing above
it, so its centre lies in it and in nothing above, and the id map must give a leaf of it -- or alpha <= 1e-9, and the id map must
give -1.  Every other pixel is an edge pixel, where the centre may fall either way: skipped, at most 0.30 of a viewport.  Every
paintable, and the undrawn ground, needs 25 decided pixels at least.  Opacity, masks, filters and blends stay out of these scenes:
``hit_leaves`` looks through them by design."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the corners of the colour cube: any two differ by 1 in some channel, and every value is exact in any number format
PALETTE = np.array([[r, g, b, 1.0] for r in (0.0, 1.0) for g in (0.0, 1.0) for b in (0.0, 1.0)])
NAMES = ["black", "blue", "green", "cyan", "red", "magenta", "yellow", "white"]
MAX_SKIPPED, MIN_DECIDED = 0.30, 25


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


def view(S, dx=14.0, dy=6.0):
    """From a scene's user space (x to the right, y down, about 0 .. 90 each) into the viewport's (row, col): a rotation and a
    scale that is not uniform behind the swap of the axes."""
    return S.Transform().matrix(0, 1, 0, 1, 0, 0) @ S.Transform().translate(dx, dy).rotate(0.2).scale(1.1, 0.9)


class Painted:
    """Builds FILL / STROKE / lazy nodes in palette colours and keeps which source object, as which kind, has which colour."""

    def __init__(self, S):
        self.S = S
        self.colour_of = {}       # (id(source), kind) -> palette index; kind None: a lazy node's payload
        self.keep = []            # (the sources stay alive: their ids stay theirs)
        self.lazy = set()

    def note(self, source, kind, k):
        assert self.colour_of.setdefault((id(source), kind), k) == k
        self.keep.append(source)

    def fill(self, path, k, rule=None):
        self.note(path, "fill", k)
        return self.S.Scene.fill(path, PALETTE[k].copy(), rule)

    def stroke(self, path, k, width, **kw):
        node = self.S.Scene.stroke(path, PALETTE[k].copy(), width, **kw)
        self.note(node[1][0], "stroke", k)     # (a dashed stroke carries its pattern in a path of its own)
        return node

    def lazy_node(self, node, k):
        from svgrasterize_amd import scene as SC

        assert node[0] == SC.RENDER_MARKERS
        self.note(node[1], None, k)
        self.lazy.add(k)
        return node

    def adopt(self, scene):
        """The paints of a loaded document: every FILL and STROKE node's flat colour must be one of the palette's."""
        from svgrasterize_amd import scene as SC

        stack = [scene]
        while stack:
            kind, args = stack.pop()
            if kind in (SC.RENDER_FILL, SC.RENDER_STROKE):
                paint = np.asarray(args[1], dtype=np.float64)
                match = np.flatnonzero((np.abs(PALETTE - paint) <= 1e-12).all(axis=1))
                assert paint.shape == (4,) and len(match) == 1, f"a paint that is no palette colour: {args[1]!r}"
                self.note(args[0], "fill" if kind == SC.RENDER_FILL else "stroke", int(match[0]))
            elif kind == SC.RENDER_GROUP:
                stack.extend(args)
            elif kind == SC.RENDER_CLIP:
                stack.append(args[0])      # (a clip path's own content draws nothing)
            else:
                assert kind == SC.RENDER_TRANSFORM, f"a node the witness does not take: {kind}"
                stack.append(args[0])

    def leaf_colours(self, leaves):
        """Per leaf the palette index (-1: a clip source, which cannot be picked).  A pickable leaf without a colour is an error."""
        out = []
        for i, leaf in enumerate(leaves):
            if not leaf.pickable:
                assert leaf.kind == "clip"
                out.append(-1)
                continue
            k = self.colour_of.get((id(leaf.source), leaf.kind), self.colour_of.get((id(leaf.source), None)))
            assert k is not None, f"leaf {i} ({leaf!r}) matches no painted node"
            out.append(k)
        return np.array(out, dtype=np.int64)


def rendered(S, scene, transform, viewport):
    """The render of `scene` on a canvas of the viewport's size, (rows, cols, 4), transparent where nothing was drawn."""
    row0, col0, rows, cols = viewport
    canvas = np.zeros((rows, cols, 4))
    res = scene.render(transform, viewport=list(viewport))
    if res is not None:
        layer = res[0].convert(pre_alpha=False, linear_rgb=False)
        image = np.asarray(layer.image, dtype=np.float64)
        r, c = int(layer.offset[0]) - row0, int(layer.offset[1]) - col0
        assert image.shape[2] == 4 and r >= 0 and c >= 0 and r + image.shape[0] <= rows and c + image.shape[1] <= cols
        canvas[r:r + image.shape[0], c:c + image.shape[1]] = image
    return canvas


def decided_pixels(canvas, colours):
    """(colour index per pixel: -1 undrawn, -2 skipped) from the render alone."""
    alpha = canvas[..., 3]
    out = np.full(alpha.shape, -2, dtype=np.int64)
    out[alpha <= 1e-9] = -1
    opaque = alpha >= 1 - 1e-9
    near = np.stack([(np.abs(canvas[..., :3] - PALETTE[k, :3]) <= 1e-9).all(axis=2) for k in colours], axis=0)
    one = near.sum(axis=0) == 1
    for j, k in enumerate(colours):
        out[opaque & one & near[j]] = k
    return out


def witness(S, name, painted, scene, transform, viewport, shows):
    """The pixel rule on one scene.  `shows`: the palette indices the scene is meant to show.  Returns (decided, id map)."""
    canvas = rendered(S, scene, transform, viewport)
    id_map, leaves = scene.id_map(transform, viewport)
    assert id_map.shape == canvas.shape[:2] and len(leaves) == len(scene.hit_leaves(transform))
    colour = painted.leaf_colours(leaves)
    used = sorted(set(colour[colour >= 0].tolist()))
    assert set(shows) <= set(used), (shows, used)
    for k in used:
        if k not in painted.lazy:      # one paintable, one leaf: only a lazy node has several
            assert (colour == k).sum() == 1, f"{NAMES[k]}: {int((colour == k).sum())} leaves"
    decided = decided_pixels(canvas, used)
    skipped = float((decided == -2).mean())
    counts = {NAMES[k]: int((decided == k).sum()) for k in used}
    print(f"{name}: skipped share {skipped:.4f}, undrawn {int((decided == -1).sum())}, decided per leaf {counts}")
    got = np.where(id_map >= 0, colour[np.maximum(id_map, 0)], -1)     # the colour of the leaf the id map names (-1: none)
    assert (id_map < len(leaves)).all() and (id_map >= -1).all() and ((id_map < 0) | (got >= 0)).all()   # (never a clip source)
    for k in used:
        here = decided == k
        assert (got[here] == k).all(), f"{name}: {int((got[here] != k).sum())} of {int(here.sum())} pixels drawn in {NAMES[k]} are picked as something else"
    assert (id_map[decided == -1] == -1).all(), f"{name}: {int((id_map[decided == -1] != -1).sum())} undrawn pixels are picked"
    assert skipped <= MAX_SKIPPED
    assert (decided == -1).sum() >= MIN_DECIDED
    for k in shows:
        assert (decided == k).sum() >= MIN_DECIDED, f"{name}: {NAMES[k]} has {int((decided == k).sum())} decided pixels"
    return decided, id_map


def polygon(S, pts):
    from svgrasterize_amd.geometry import PATH_CLOSED, PATH_LINE

    pts = [[float(x), float(y)] for x, y in pts]
    return S.Path([[(PATH_LINE, [a, b]) for a, b in zip(pts, pts[1:])] + [(PATH_CLOSED, [pts[-1], pts[0]])]])


def rect(S, x0, y0, x1, y1):
    return polygon(S, [(x0, y0), (x1, y0), (x1, y1), (x0, y1)])


def circle(S, cx, cy, r):
    d = f"M{cx + r},{cy} A{r},{r} 0 0 1 {cx - r},{cy} A{r},{r} 0 0 1 {cx + r},{cy} Z"
    return S.Path.from_svg(d)


def star(S, cx, cy, r):
    t = -math.pi / 2 + 2.0 * math.pi * (2 * np.arange(5) % 5) / 5
    return polygon(S, np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1))


# ---- fills and rules --------------------------------------------------------------------------------------------------------------
def test_fills_rules_and_a_mirrored_group(S):
    p = Painted(S)
    mirror = S.Transform().translate(90.0, 0.0).scale(-1.0, 1.0)      # x -> 90 - x
    scene = S.Scene.group([
        p.fill(polygon(S, [(2, 2), (40, 6), (30, 34), (6, 28)]), 1),
        p.fill(polygon(S, [(18, 14), (52, 10), (46, 40), (22, 44)]), 2),                      # over the first
        p.fill(star(S, 68, 24, 22), 3, S.PATH_FILL_NONZERO),
        p.fill(star(S, 24, 68, 22), 4, S.PATH_FILL_EVENODD),                                  # its pentagon shows what is beneath
        p.fill(circle(S, 62, 66, 14), 5),
        S.Scene.group([p.fill(rect(S, 2, 46, 14, 58), 6), p.fill(polygon(S, [(4, 78), (20, 88), (2, 88)]), 7)]).transform(mirror),
    ])
    viewport = (-2, 3, 112, 125)      # the origin of a viewport is not the origin of the plane
    decided, id_map = witness(S, "fills", p, scene, view(S), viewport, shows=[1, 2, 3, 4, 5, 6, 7])
    # the even-odd star's pentagon is a hole, the nonzero star's is not: from the render, and so in the id map
    tr = view(S)
    for centre, k in (((24.0, 68.0), -1), ((68.0, 24.0), 3)):
        r, c = np.floor(tr(np.array([centre]))[0]).astype(int) - np.array(viewport[:2])
        assert decided[r, c] == k and (id_map[r, c] < 0) == (k < 0)


# ---- clips ------------------------------------------------------------------------------------------------------------------------
def clip_scene(S, p, which):
    """(scene, its target without the clip, the colours it shows)."""
    if which == "union":          # a clip scene of two shapes lets pass what lies in either
        target = p.fill(rect(S, 4, 4, 86, 86), 1)
        clip = S.Scene.group([p.fill(rect(S, 8, 10, 40, 44), 7), p.fill(circle(S, 60, 60, 20), 7)])
        return target.clip(clip), target, [1]
    if which == "nested":         # two clips on one target let pass what lies in both
        target = p.fill(rect(S, 4, 4, 86, 86), 2)
        a, b = p.fill(rect(S, 10, 10, 60, 80), 7), p.fill(circle(S, 50, 45, 30), 7)
        return target.clip(a).clip(b), target, [2]
    if which == "clipped-source":   # one of the clip scene's shapes is itself clipped
        target = p.fill(rect(S, 4, 4, 86, 86), 4)
        inner = p.fill(rect(S, 40, 0, 90, 50), 7)
        clip = S.Scene.group([p.fill(rect(S, 8, 50, 36, 84), 7), p.fill(circle(S, 58, 40, 26), 7).clip(inner)])
        return target.clip(clip), target, [4]
    assert which == "bbox-units"  # the clip's shapes are given in the unit square of the target's bounding box: of both shapes' hull
    target = S.Scene.group([p.fill(rect(S, 6, 8, 44, 50), 1), p.fill(polygon(S, [(40, 40), (86, 46), (80, 84), (46, 80)]), 2)])
    clip = S.Scene.group([p.fill(circle(S, 0.5, 0.5, 0.42), 7), p.fill(rect(S, 0.0, 0.0, 0.3, 0.25), 7)])
    return target.clip(clip, bbox_units=True), target, [1, 2]


@pytest.mark.parametrize("moved", [False, True], ids=["plain", "transformed"])
@pytest.mark.parametrize("which", ["union", "nested", "clipped-source", "bbox-units"])
def test_clips(S, which, moved):
    p = Painted(S)
    scene, target, shows = clip_scene(S, p, which)
    if moved:
        inner = S.Transform().translate(88.0, 4.0).scale(-0.95, 0.9)      # a mirror inside the scene, around the whole clip
        scene, target = scene.transform(inner), target.transform(inner)
    viewport = (0, 0, 112, 128)
    decided, _id_map = witness(S, f"clip {which}{' transformed' if moved else ''}", p, scene, view(S), viewport, shows=shows)
    # the clip bites: pixels the target alone covers in full are undrawn
    alone = rendered(S, target, view(S), viewport)
    bitten = (alone[..., 3] >= 1 - 1e-9) & (decided == -1)
    assert bitten.sum() >= MIN_DECIDED, f"{which}: the clip removes {int(bitten.sum())} whole pixels of its target"


# ---- strokes ----------------------------------------------------------------------------------------------------------------------
def test_strokes(S):
    p = Painted(S)
    zigzag = S.Path.from_svg("M6,30 L30,8 L50,34 L84,10")
    scene = S.Scene.group([
        p.stroke(zigzag, 1, 10.0, linejoin="round"),
        p.stroke(zigzag.transform(S.Transform().translate(0.0, 26.0)), 2, 10.0, linejoin="miter"),
        p.fill(rect(S, 8, 62, 40, 88), 3),
        p.stroke(circle(S, 24, 75, 13), 4, 8.0),                                  # a closed ring: its interior shows the fill beneath
        p.stroke(S.Path.from_svg("M48,66 L86,66 L86,88 L48,88"), 5, 8.0, dasharray=[14.0, 12.0]),
    ])
    decided, _id_map = witness(S, "strokes", p, scene, view(S), (0, 0, 112, 128), shows=[1, 2, 3, 4, 5])
    tr = view(S)
    r, c = np.floor(tr(np.array([[24.0, 75.0]]))[0]).astype(int)
    assert decided[r, c] == 3                     # inside the ring
    # the dashes have gaps: along the dashed line there are pixels of its colour and undrawn ones
    along = np.floor(tr(np.stack([np.linspace(50.0, 84.0, 69), np.full(69, 66.0)], axis=1))).astype(int)
    on_line = decided[along[:, 0], along[:, 1]]
    assert (on_line == 5).any() and (on_line == -1).any()


# ---- markers and text -------------------------------------------------------------------------------------------------------------
def font(S):
    with open(os.path.join(GOLDEN, "fonts", "varsynth.ttf"), "rb") as f:
        return S.read_ttf(f.read())


def test_markers(S):
    p = Painted(S)
    content = S.Scene.fill(polygon(S, [(0, 0), (12, 6), (0, 12)]), PALETTE[5].copy())
    marker = S.Marker(content, ref=(6.0, 6.0), size=(12.0, 12.0), units_stroke_width=False, orient="auto")
    path = S.Path.from_svg("M16,22 L50,64 L80,26")
    scene = S.Scene.group([p.fill(polygon(S, [(6, 10), (88, 14), (50, 84)]), 2), p.lazy_node(S.Scene.markers(path, marker, marker, marker), 5)])
    leaves = scene.hit_leaves(view(S))
    assert sum(1 for leaf in leaves if leaf.pickable and leaf.source is scene[1][1][1]) == 3      # an instance per vertex
    witness(S, "markers", p, scene, view(S), (0, 0, 112, 128), shows=[2, 5])


def test_text(S):
    p = Painted(S)
    text = p.lazy_node(S.Scene.text(font(S), 64.0, "Ao", {"fill": PALETTE[6].copy()}), 6).transform(S.Transform().translate(4.0, 70.0))
    scene = S.Scene.group([p.fill(rect(S, 10, 40, 80, 60), 1), text])
    witness(S, "text", p, scene, view(S), (0, 0, 112, 128), shows=[1, 6])


def test_text_on_a_path(S):
    p = Painted(S)
    arc = S.Path.from_svg("M8,70 Q45,10 84,70")
    node = p.lazy_node(S.Scene.text_on_path(arc, [("Ao", font(S), 48.0, {"fill": PALETTE[3].copy()}, 0.0, 0.0)], start_offset=12.0), 3)
    scene = S.Scene.group([p.fill(rect(S, 30, 20, 60, 50), 4), node])
    witness(S, "text on a path", p, scene, view(S), (0, 0, 112, 128), shows=[3, 4])


# ---- a document -------------------------------------------------------------------------------------------------------------------
DOC = """<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="90" height="90">
<defs>
<clipPath id="cp" clipPathUnits="objectBoundingBox"><circle cx="0.5" cy="0.5" r="0.45"/></clipPath>
<symbol id="sym"><rect id="sq" x="0" y="0" width="24" height="20" fill="#0000ff"/></symbol>
</defs>
<rect id="back" x="4" y="4" width="40" height="36" fill="#ff0000"/>
<rect id="round" x="50" y="4" width="36" height="40" fill="#00ff00" clip-path="url(#cp)"/>
<use id="u" xlink:href="#sym" x="10" y="14"/>
<g id="outer" transform="translate(8,48)"><g id="inner" transform="scale(1.5,1.25)">
<rect id="deep" x="0" y="0" width="20" height="28" fill="#ff00ff"/></g></g>
<path id="line" d="M48,56 L84,56 L66,84" fill="none" stroke="#00ffff" stroke-width="9"/>
</svg>"""
DOC_COLOURS = {"back": 4, "round": 2, "sq": 1, "deep": 5, "line": 3}


def test_a_document(S):
    scene, ids, size = S.svg_scene_from_str(DOC)
    assert tuple(size) == (90, 90)
    p = Painted(S)
    p.adopt(scene)
    viewport = (0, 0, 112, 128)
    decided, _id_map = witness(S, "document", p, scene, view(S), viewport, shows=sorted(DOC_COLOURS.values()))
    # the objectBoundingBox clip bites: the corner of the clipped rectangle is undrawn
    tr = view(S)
    r, c = np.floor(tr(np.array([[51.5, 5.5]]))[0]).astype(int)
    assert decided[r, c] == -1
    # elements_at names the element whose colour the render shows: at the middle decided pixel of three colours
    for name in ("back", "sq", "deep"):
        rows, cols = np.nonzero(decided == DOC_COLOURS[name])
        j = len(rows) // 2
        names = S.elements_at(scene, ids, tr, [(rows[j] + 0.5, cols[j] + 0.5)])[0]
        assert names and names[0] == name, (name, names)
    assert "u" in S.elements_at(scene, ids, tr, tr(np.array([[20.0, 24.0]])))[0]
