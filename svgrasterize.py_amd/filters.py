"""Filter effects (reference S:1716-1944): feGaussianBlur (the one on the hot path) and the other
primitives the reference implements -- feOffset, feMerge, feBlend, feComposite, feColorMatrix, feMorphology (8f-4) --,
plus primitives the reference does not have: feFlood, feTurbulence, feComponentTransfer, feConvolveMatrix,
feDisplacementMap, feDropShadow (expanded into the others by ``Filter.drop_shadow``), feDiffuseLighting and feSpecularLighting
(with a ``DistantLight``, ``PointLight`` or ``SpotLight``).

``Filter`` keeps the reference's (names, filters) structure so scene dumps replay unchanged.  The blur weights are
built on the host exactly like ``blur_kernel`` does (a few thousand numbers); every per-pixel operation runs on the
GPU (``svgr_layer_convolve``, ``svgr_layer_blend``, ``svgr_layer_color_matrix``, ``svgr_layer_morphology``,
``svgr_layer_turbulence``, ``svgr_layer_component_transfer``, ``svgr_layer_convolve_matrix``, ``svgr_layer_displacement_map``,
``svgr_layer_lighting``).

The chain runs in linearRGB (``color-interpolation-filters`` is ignored, as in the reference).  The generators (feFlood,
feTurbulence) and the lighting primitives cover the filter region: the ``<filter>``'s x / y / width / height in ``filterUnits`` (default
objectBoundingBox, -10% / -10% / 120% / 120%), resolved at call time against the hull's bounding box in user space (or the
source layer's extent when there is no hull) and rounded out to whole device pixels.  The other primitives keep the extent
of their input; in particular feComponentTransfer leaves the pixels outside its input transparent even where feFuncA maps
0 to something else.  Light sources stay in user space in the chain and are mapped to device space at call time
(``Layer.lighting``).

Primitive subregions (``Filter.subregion``; x / y / width / height on a primitive) and ``primitiveUnits`` (``Filter.empty``'s
`primitive_bbox`) follow Filter Effects 1 on the device-pixel grid.  A primitive with at least one of the four has a subregion;
the missing ones come from its default subregion: the union of the subregions of the results it references when each has one,
else the filter region (always the filter region for feTile, whose purpose is to cover more than its input).  A primitive without any has the union of its inputs' subregions when each has one and otherwise NONE:
it runs as described above, which keeps filters without these attributes bit for bit what they were.  A subregion is a
rectangle in user space (fractions of the bounding box under objectBoundingBox) and becomes the integer box around its
transformed corners, cut to the filter region's box -- under a rotation the axis-aligned box around the rotated rectangle,
as for the filter region.  The result of a primitive with box B is a layer of exactly B (``Layer.window``); generators,
lighting, feTile and feImage fill B instead of the filter region; an empty B is a transparent result.  Under
objectBoundingBox the lengths of feGaussianBlur / feOffset / feMorphology (and feDropShadow) are fractions of the box too;
light positions, ``surfaceScale`` and feDisplacementMap's ``scale`` are not rescaled.

feTile (``Layer.tile``, ``svgr_layer_tile``) repeats the subregion of its input (the filter region when the input has none) over
its own box.  feImage draws a raster (placed into its subregion by ``preserveAspectRatio`` and sampled by the image fill) or an
element of the document (looked up when the filter runs; rendered in the filtered element's user space, like ``<use>``)."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from .geometry import Transform
from .layer import COMPOSE_IN, Layer

import warnings

FE_BLEND, FE_COLOR_MATRIX, FE_COMPONENT_TRANSFER, FE_COMPOSITE, FE_CONVOLVE_MATRIX = 0, 1, 2, 3, 4  # S:1716-1730
FE_DIFFUSE_LIGHTING, FE_DISPLACEMENT_MAP, FE_FLOOD, FE_GAUSSIAN_BLUR, FE_MERGE = 5, 6, 7, 8, 9
FE_MORPHOLOGY, FE_OFFSET, FE_SPECULAR_LIGHTING, FE_TILE, FE_TURBULENCE = 10, 11, 12, 13, 14
FE_IMAGE = 15   # (not in the reference's list)
COLOR_MATRIX_LUM = np.array([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0.2125, 0.7154, 0.0721, 0, 0]], dtype=np.float64)
# feColorMatrix type="saturate" / "hueRotate" (the SVG 1.1 filter chapter's constants; S:1740-1747): the colour block is
# _HUE_BASE + cos(a) * _HUE_COS + sin(a) * _HUE_SIN; saturate(s) is the same with (cos, sin) := (s, 0)
_HUE_BASE = np.array([[0.213, 0.715, 0.072]] * 3, dtype=np.float64)
_HUE_COS = np.array([[0.787, -0.715, -0.072], [-0.213, 0.285, -0.072], [-0.213, -0.715, 0.928]], dtype=np.float64)
_HUE_SIN = np.array([[-0.213, -0.715, 0.928], [0.143, 0.140, -0.283], [-0.787, 0.715, 0.072]], dtype=np.float64)


def _hue_matrix(c: float, s: float) -> np.ndarray:
    matrix = np.eye(4, 5)
    matrix[:3, :3] = np.dot(np.stack([_HUE_BASE, _HUE_COS, _HUE_SIN]).T, [1, c, s]).T
    return matrix


def color_matrix_hue_rotate(angle: float) -> np.ndarray:
    """4x5 colour matrix of a hue rotation by ``angle`` radians (S:1947-1951)."""
    return _hue_matrix(math.cos(angle), math.sin(angle))


def color_matrix_saturate(value: float) -> np.ndarray:
    """4x5 colour matrix of feColorMatrix ``saturate`` (S:1954-1957)."""
    return _hue_matrix(value, 0)


# feDropShadow's first step: the input's alpha, colour zero (a colour matrix on straight alpha)
COLOR_MATRIX_ALPHA = np.array([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 0]], dtype=np.float64)
# limits of the C ABI (include/svgr.h): SVGR_TURBULENCE_MAX_OCTAVES, SVGR_TRANSFER_MAX_VALUES, SVGR_CONVOLVE_MATRIX_MAX_ORDER
TURBULENCE_MAX_OCTAVES, TRANSFER_MAX_VALUES, CONVOLVE_MATRIX_MAX_ORDER = 32, 4096, 32
# the filter region of a generator: (objectBoundingBox units?, x, y, width, height); None entries take the defaults below
FILTER_REGION_DEFAULT = (True, -0.1, -0.1, 1.2, 1.2)


def _user_bbox(transform: Transform, source: Layer, hull=None):
    """[x, y, width, height] in user space of the hull (ConvexHull.bbox), or of the source layer's extent without one."""
    if hull is not None and len(hull.points) > 0:
        return hull.bbox(transform)
    r0, c0 = source.offset
    r1, c1 = r0 + source.height, c0 + source.width
    pts = transform.invert(np.array([[r0, c0], [r0, c1], [r1, c0], [r1, c1]], dtype=np.float64))
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return [lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]]


def filter_region(region, transform: Transform, source: Layer, hull=None):
    """(offset, shape, (x, y, width, height)): the device pixels of the filter region `region` (see FILTER_REGION_DEFAULT)
    -- the integer box (floor / ceil) around its four transformed corners, at least one pixel -- and the region in user
    space.  objectBoundingBox values are fractions of the hull's bounding box (`_user_bbox`)."""
    bbox_units, *vals = FILTER_REGION_DEFAULT if region is None else region
    if bbox_units or any(v is None for v in vals):
        bx, by, bw, bh = _user_bbox(transform, source, hull)
        fx, fy, fw, fh = (d if v is None else v for v, d in zip(vals, FILTER_REGION_DEFAULT[1:]))
        rel = (bx + fx * bw, by + fy * bh, fw * bw, fh * bh)
        # (userSpaceOnUse without a value: the objectBoundingBox default for it; the viewport is not known here)
        vals = rel if bbox_units else [r if v is None else v for v, r in zip(vals, rel)]
    x, y, w, h = (float(v) for v in vals)
    corners = transform(np.array([[x, y], [x + w, y], [x, y + h], [x + w, y + h]], dtype=np.float64))
    lo, hi = np.floor(corners.min(axis=0)), np.ceil(corners.max(axis=0))
    shape = (max(int(hi[0] - lo[0]), 1), max(int(hi[1] - lo[1]), 1))
    return (int(lo[0]), int(lo[1])), shape, (x, y, w, h)


class DistantLight(NamedTuple):
    """feDistantLight: direction angles in degrees, user space."""
    azimuth: float = 0.0
    elevation: float = 0.0


class PointLight(NamedTuple):
    """fePointLight: position in user space (z in user units)."""
    x: float = 0.0
    y: float = 0.0
    z: float = 0.0


class SpotLight(NamedTuple):
    """feSpotLight: position and pointsAt in user space; `limiting_cone_angle` in degrees, None = no cone."""
    x: float = 0.0
    y: float = 0.0
    z: float = 0.0
    points_at_x: float = 0.0
    points_at_y: float = 0.0
    points_at_z: float = 0.0
    specular_exponent: float = 1.0
    limiting_cone_angle: float | None = None


FE_SOURCE_ALPHA = "SourceAlpha"
FE_SOURCE_GRAPHIC = "SourceGraphic"


_KERNEL_MEMO: dict = {}   # (matrix bytes, sigma) -> weights: a document's blurs repeat from render to render (and among its nodes)


def blur_kernel(transform: Transform, sigma):
    """Gaussian weights on the pixel grid for a blur given in user space (S:1903-1944); None = no-op.

    The values are the reference's own numpy expressions (its fixtures pin them bit for bit: numpy's vectorised ``exp``
    and its pairwise ``sum`` have no counterpart in libm), evaluated once per (matrix, sigma): the 37 blurs of icons.svg
    cost a dictionary look-up each on every render after the first."""
    memo_key = (transform.key(), float(sigma[0]), float(sigma[1]))
    hit = _KERNEL_MEMO.get(memo_key, _KERNEL_MEMO)
    if hit is not _KERNEL_MEMO:
        return hit
    if len(_KERNEL_MEMO) > 1024:
        _KERNEL_MEMO.clear()
    weights = _KERNEL_MEMO[memo_key] = _blur_weights(transform, float(sigma[0]), float(sigma[1]))
    if weights is not None:
        weights.setflags(write=False)   # (shared between the renders that look it up)
    return weights


def _blur_weights(transform: Transform, sigma_x: float, sigma_y: float):
    origin = transform([0, 0])
    # device pixels per user unit along the two axes; a deviation below half a pixel is raised to half a pixel unless BOTH are
    # (then the blur is the identity)
    per_x, per_y = np.linalg.norm(transform(np.eye(2)) - origin, axis=1)
    small_x, small_y = per_x * sigma_x < 0.5, per_y * sigma_y < 0.5
    if small_x and small_y:
        return None
    if small_x:
        sigma_x = 0.5 / per_x
    elif small_y:
        sigma_y = 0.5 / per_y
    # the kernel's footprint: 2.5 deviations to either side, mapped to the pixel grid, made odd in both directions
    reach_x, reach_y = 2.5 * sigma_x, 2.5 * sigma_y
    frame = transform([[-reach_x, -reach_y], [-reach_x, reach_y], [reach_x, reach_y], [reach_x, -reach_y]]) - origin
    low, high = frame.min(axis=0).astype(int), frame.max(axis=0).astype(int)
    kw, kh = (int(n) + (~int(n) & 1) for n in high - low)
    # pixel centres of the footprint, taken back to user space without the translation
    back = transform.invert
    ix, iy = np.indices((kw, kh)).astype(np.float64)
    centres = np.concatenate([ix[..., None], iy[..., None]], axis=2) + [-kw / 2 + 0.5, -kh / 2 + 0.5]
    user = back(centres)
    user -= back([0, 0])
    weights = np.exp(-np.square(user) / (2 * np.square(np.array([sigma_x, sigma_y])))).prod(axis=-1)
    return weights / weights.sum()


def _device_box(transform: Transform, rect):
    """(row0, col0, row1, col1): the integer box (floor / ceil) around the four transformed corners of the user-space
    rectangle `rect` = (x, y, width, height) -- ``filter_region``'s rounding, without its one-pixel minimum."""
    x, y, w, h = rect
    corners = transform(np.array([[x, y], [x + w, y], [x, y + h], [x + w, y + h]], dtype=np.float64))
    lo, hi = np.floor(corners.min(axis=0)), np.ceil(corners.max(axis=0))
    return int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])


def _union(regions):
    """The union of resolved subregions [(rect, box)]: the bounding rectangle in user space and the bounding device box."""
    rects, boxes = [r for r, _ in regions], [b for _, b in regions]
    x0, y0 = min(r[0] for r in rects), min(r[1] for r in rects)
    x1, y1 = max(r[0] + r[2] for r in rects), max(r[1] + r[3] for r in rects)
    r0, c0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    r1, c1 = max(b[0] + b[2] for b in boxes), max(b[1] + b[3] for b in boxes)
    return (x0, y0, x1 - x0, y1 - y0), (r0, c0, r1 - r0, c1 - c0)


_IMAGE_ACTIVE: set = set()   # the feImage element references being rendered (a reference that leads back to itself stops there)


class Filter(NamedTuple):
    names: dict
    filters: list  # [(type, attrs, inputs)]
    # entry index -> the primitive's subregion (x, y, width, height), None = not given; for the two entries of a drop shadow
    # that share one see ``drop_shadow``.  Entries without one are not in the table.
    subregions: dict = {}
    primitive_bbox: bool = False   # primitiveUnits="objectBoundingBox"
    # the <filter>'s region in the form of FILTER_REGION_DEFAULT: the frame of the subregions and what feTile / feImage cover
    # without one (the older generators carry the region in their own attrs)
    region: tuple | None = None

    @classmethod
    def empty(cls, primitive_bbox: bool = False, region=None) -> "Filter":
        return cls({FE_SOURCE_ALPHA: 0, FE_SOURCE_GRAPHIC: 1}, [], {}, bool(primitive_bbox), region)

    def add_filter(self, type, attrs, inputs, result=None) -> "Filter":
        names, filters = dict(self.names), list(self.filters)
        args = []
        for name in inputs:
            idx = None if name is None else self.names.get(name)
            args.append(len(filters) + 1 if idx is None else idx)  # default: previous result
        if result is not None:
            names[result] = len(filters) + 2
        filters.append((type, attrs, args))
        return self._replace(names=names, filters=filters)

    def subregion(self, x=None, y=None, width=None, height=None) -> "Filter":
        """The primitive subregion of the entry added last, in primitiveUnits (user space, or fractions of the bounding box);
        None = not given (it comes from the default subregion).  A negative `width` or `height` is an error here; 0 makes the
        result transparent."""
        if not self.filters:
            raise ValueError("subregion: the filter has no primitive yet")
        vals = tuple(None if v is None else float(v) for v in (x, y, width, height))
        if any(v is not None and v < 0 for v in vals[2:]):
            raise ValueError(f"negative subregion size: {vals[2]}, {vals[3]}")
        table = dict(self.subregions)
        table[len(self.filters) - 1] = vals
        return self._replace(subregions=table)

    def tile(self, input=None, result=None) -> "Filter":
        """feTile: the subregion of `input` (the filter region when it has none) repeated over this primitive's subregion
        (``subregion``; the filter region without one)."""
        return self.add_filter(FE_TILE, tuple(), [input], result)

    def image(self, pixels=None, preserve_aspect_ratio="xMidYMid meet", smooth=True, element=None, ids=None, result=None) -> "Filter":
        """feImage: the (h, w, 4) uint8 straight-alpha sRGB raster `pixels` placed into the primitive's subregion like an
        <image> into its viewport; or the scene ``ids[element]``, looked up when the filter runs and rendered in the filtered
        element's user space.  With neither (a source that could not be read) the result is transparent."""
        if pixels is not None:
            attrs = ("raster", np.asarray(pixels), preserve_aspect_ratio, bool(smooth))
        elif element is not None:
            attrs = ("element", element, None if ids is None else ids.get)   # (the look-up, not the table: a short repr)
        else:
            attrs = ("none",)
        return self.add_filter(FE_IMAGE, attrs, [], result)

    def offset(self, dx, dy, input=None, result=None) -> "Filter":
        return self.add_filter(FE_OFFSET, (dx, dy), [input], result)

    def merge(self, inputs, result=None) -> "Filter":
        return self.add_filter(FE_MERGE, tuple(), inputs, result)

    def blur(self, std_x, std_y=None, input=None, result=None) -> "Filter":
        return self.add_filter(FE_GAUSSIAN_BLUR, (std_x, std_y), [input], result)

    def blend(self, in1, in2, mode=None, result=None) -> "Filter":
        return self.add_filter(FE_BLEND, (mode,), [in1, in2], result)

    def composite(self, in1, in2, mode=None, result=None) -> "Filter":
        return self.add_filter(FE_COMPOSITE, (mode,), [in1, in2], result)

    def color_matrix(self, input, matrix, result=None) -> "Filter":
        return self.add_filter(FE_COLOR_MATRIX, (matrix,), [input], result)

    def morphology(self, rx, ry, method, input, result=None) -> "Filter":
        return self.add_filter(FE_MORPHOLOGY, (rx, ry, method), [input], result)

    def flood(self, color, region=None, result=None) -> "Filter":
        """feFlood: `color` = straight-alpha linear RGBA (flood-opacity already in the alpha) over the filter region."""
        return self.add_filter(FE_FLOOD, (tuple(float(c) for c in color), region), [], result)

    def turbulence(self, base_frequency, num_octaves=1, seed=0, stitch=False, fractal_noise=False, region=None,
                   result=None) -> "Filter":
        fx, fy = base_frequency
        return self.add_filter(FE_TURBULENCE, ((fx, fy), num_octaves, seed, stitch, fractal_noise, region), [], result)

    def component_transfer(self, input, funcs, result=None) -> "Filter":
        """`funcs`: (R, G, B, A) transfer functions in ``Layer.component_transfer``'s form."""
        return self.add_filter(FE_COMPONENT_TRANSFER, (tuple(funcs),), [input], result)

    def convolve_matrix(self, input, kernel, divisor=None, bias=0.0, target=None, edge_mode="duplicate", preserve_alpha=False,
                        result=None) -> "Filter":
        return self.add_filter(FE_CONVOLVE_MATRIX, (kernel, divisor, bias, target, edge_mode, preserve_alpha), [input], result)

    def displacement_map(self, in1, in2, scale=0.0, x_channel="A", y_channel="A", result=None) -> "Filter":
        return self.add_filter(FE_DISPLACEMENT_MAP, (scale, x_channel, y_channel), [in1, in2], result)

    def diffuse_lighting(self, input, light, color=(1.0, 1.0, 1.0), surface_scale=1.0, diffuse_constant=1.0, region=None,
                         result=None) -> "Filter":
        """feDiffuseLighting: `light` a DistantLight / PointLight / SpotLight, `color` linear RGB; covers the filter region."""
        return self.add_filter(FE_DIFFUSE_LIGHTING, (light, tuple(float(c) for c in color), float(surface_scale),
                                                     float(diffuse_constant), region), [input], result)

    def specular_lighting(self, input, light, color=(1.0, 1.0, 1.0), surface_scale=1.0, specular_constant=1.0,
                          specular_exponent=1.0, region=None, result=None) -> "Filter":
        """feSpecularLighting (premultiplied result), otherwise as ``diffuse_lighting``."""
        return self.add_filter(FE_SPECULAR_LIGHTING, (light, tuple(float(c) for c in color), float(surface_scale),
                                                      float(specular_constant), float(specular_exponent), region), [input], result)

    def drop_shadow(self, dx=2.0, dy=2.0, std_x=2.0, std_y=None, color=(0.0, 0.0, 0.0, 1.0), region=None, input=None,
                    result=None, subregion=None) -> "Filter":
        """feDropShadow as the six entries it stands for: the alpha of `input`, blurred, offset, a flood of `color` IN that
        shadow, and the merge of [shadow, `input`].  Only the merge can be named (`result`).  `subregion` = (x, y, width,
        height) as in ``subregion``: it applies to the merge -- its default is the subregion of `input`, feDropShadow's one
        input -- and the flood fills the same box."""
        names, filters = dict(self.names), list(self.filters)
        src = names.get(input) if input is not None else None
        src = len(filters) + 1 if src is None else src   # (the default input: add_filter's rule)
        at = len(filters) + 2                            # (stack index of the first new entry)
        filters.append((FE_COLOR_MATRIX, (COLOR_MATRIX_ALPHA,), [src]))
        filters.append((FE_GAUSSIAN_BLUR, (std_x, std_y), [at]))
        filters.append((FE_OFFSET, (dx, dy), [at + 1]))
        filters.append((FE_FLOOD, (tuple(float(c) for c in color), region), []))
        filters.append((FE_COMPOSITE, (COMPOSE_IN,), [at + 3, at + 2]))
        filters.append((FE_MERGE, tuple(), [at + 4, src]))
        if result is not None:
            names[result] = at + 5
        table = self.subregions
        if subregion is not None:
            merged = self._replace(names=names, filters=filters).subregion(*subregion)
            table = dict(merged.subregions)
            table[len(filters) - 1] = (*table[len(filters) - 1], [src])   # (the default subregion: from `input` alone)
            table[len(filters) - 3] = len(filters) - 1                     # (the flood: the box of the merge)
        return self._replace(names=names, filters=filters, subregions=table)

    def _regions(self, transform: Transform, source: Layer, hull, frame):
        """stack index -> the result's subregion ((x, y, width, height) in user space, (row0, col0, rows, cols) in device
        pixels) or None; `frame` = the filter region in the same form.  See the module docstring."""
        memo: dict = {}
        bbox = _user_bbox(transform, source, hull) if self.primitive_bbox else None
        f0, f1, frows, fcols = frame[1]

        def region(s):
            if s < 2:
                return None   # (SourceAlpha, SourceGraphic)
            if s in memo:
                return memo[s]
            _ftype, _attrs, inputs = self.filters[s - 2]
            spec = self.subregions.get(s - 2)
            if isinstance(spec, int):   # (a drop shadow's flood: the box of its merge)
                res = region(spec + 2)
            else:
                refs = [region(j) for j in (inputs if spec is None or len(spec) == 4 else spec[4])]
                res = _union(refs) if refs and all(r is not None for r in refs) else None
                if _ftype == FE_TILE:   # (the specification's exception: feTile is there to cover more than its input)
                    res = frame
                if spec is not None:
                    vals = spec[:4]
                    if bbox is not None:
                        bx, by, bw, bh = bbox
                        vals = tuple(None if v is None else o + v * n for v, o, n in zip(vals, (bx, by, 0.0, 0.0), (bw, bh, bw, bh)))
                    rect = tuple(d if v is None else v for v, d in zip(vals, (frame if res is None else res)[0]))
                    r0, c0, r1, c1 = _device_box(transform, rect)
                    if not (rect[2] > 0 and rect[3] > 0):
                        r1, c1 = r0, c0
                    r0, c0, r1, c1 = max(r0, f0), max(c0, f1), min(r1, f0 + frows), min(c1, f1 + fcols)
                    rows, cols = max(r1 - r0, 0), max(c1 - c0, 0)
                    res = (rect, (r0, c0, rows, cols) if rows and cols else (r0, c0, 0, 0))
            memo[s] = res
            return res

        return region

    def _image(self, attrs, transform: Transform, source: Layer, rect):
        """feImage's picture as a layer (any extent), or None: see ``image``.  `rect`: the subregion in user space."""
        from .scene import Scene   # noqa: PLC0415 (scene imports this module)

        kind = attrs[0]
        if kind == "raster":
            _, pixels, par, smooth = attrs
            scene = Scene.image(pixels, *rect, par, smooth)
            if scene is None:
                return None
            key = None
        elif kind == "element":
            _, name, lookup = attrs
            scene = None if lookup is None else lookup(name)
            if not isinstance(scene, Scene):
                warnings.warn(f"feImage: no drawable element with id: {name}")
                return None
            key = id(attrs)
            if key in _IMAGE_ACTIVE:
                warnings.warn(f"feImage: element {name} is drawn through this very feImage: transparent")
                return None
            _IMAGE_ACTIVE.add(key)
        else:
            return None
        try:
            # (inside the filtered element's render: Scene.render's lock is re-entrant, and without a viewport the walk shares the
            #  outer render's state, like a pattern's tile)
            res = scene.render(transform, linear_rgb=source.linear_rgb)
        finally:
            _IMAGE_ACTIVE.discard(key)
        return None if res is None else res[0]

    def __call__(self, transform: Transform, source: Layer, hull=None) -> Layer:
        """Execute the filter chain on `source` (S:1801-1831).  `hull`: the filtered node's ConvexHull, the frame of an
        objectBoundingBox filter region and of objectBoundingBox primitive units."""
        stack: list = [None, source.convert(pre_alpha=False, linear_rgb=True)]

        def get(i):
            if i == 0 and stack[0] is None:  # SourceAlpha, built only when referenced
                alpha = source.image[..., -1:] * np.array([0, 0, 0, 1])
                stack[0] = Layer(alpha, source.offset, pre_alpha=True, linear_rgb=True)
            return stack[i]

        frame = regions = None
        if self.subregions or any(f[0] in (FE_TILE, FE_IMAGE) for f in self.filters):
            f_off, f_shape, f_rect = filter_region(self.region, transform, source, hull)
            frame = (f_rect, (*f_off, *f_shape))
            if self.subregions:
                regions = self._regions(transform, source, hull, frame)
        unit_x = unit_y = 1.0   # a primitive's lengths in user units: fractions of the bounding box under objectBoundingBox
        if self.primitive_bbox:
            _, _, unit_x, unit_y = _user_bbox(transform, source, hull)

        for index, (ftype, attrs, inputs) in enumerate(self.filters):
            sub = None if regions is None else regions(index + 2)
            box = None if sub is None else sub[1]
            if box is not None and box[2] * box[3] == 0:   # (an empty subregion: nothing to compute)
                stack.append(Layer.transparent(box[:2]))
                continue

            def area(region):
                """(offset, shape, user rectangle) a generator fills: its subregion, or without one the filter region"""
                if box is not None:
                    return box[:2], box[2:], sub[0]
                return filter_region(region, transform, source, hull)

            args = [get(i) for i in inputs]
            if ftype == FE_GAUSSIAN_BLUR:
                std_x, std_y = attrs
                std_y = std_x if std_y is None else std_y
                if self.primitive_bbox:
                    std_x, std_y = std_x * unit_x, std_y * unit_y
                kernel = blur_kernel(transform, (std_x, std_y))
                res = args[0] if kernel is None else args[0].convolve(kernel)
            elif ftype == FE_OFFSET:  # S:1844-1850
                dx, dy = attrs
                if self.primitive_bbox:
                    dx, dy = dx * unit_x, dy * unit_y
                x, y = args[0].offset
                tx, ty = transform(transform.invert([x, y]) + [dx, dy])
                res = args[0].translate(int(tx) - x, int(ty) - y)
            elif ftype == FE_MERGE:  # S:1867-1871
                res = Layer.compose(args, linear_rgb=True)
            elif ftype == FE_BLEND:  # S:1874-1879 (the reference composes OVER whatever the mode)
                warnings.warn("feBlend is not properly supported")
                res = Layer.compose([args[1], args[0]], linear_rgb=True)
            elif ftype == FE_COMPOSITE:  # S:1882-1886
                res = Layer.compose([args[1], args[0]], attrs[0], linear_rgb=True)
            elif ftype == FE_COLOR_MATRIX:  # S:1834-1841
                matrix = attrs[0]
                if not isinstance(matrix, np.ndarray) or matrix.shape != (4, 5):
                    warnings.warn(f"invalid color matrix: {matrix}")
                    res = args[0]
                else:
                    res = args[0].color_matrix(matrix)
            elif ftype == FE_MORPHOLOGY:  # S:1853-1864
                rx, ry, method = attrs
                if self.primitive_bbox:
                    rx, ry = rx * unit_x, ry * unit_y
                ux, uy = transform([[rx, 0], [0, ry]]) - transform([[0, 0], [0, 0]])
                x, y = int(np.linalg.norm(ux) * 2), int(np.linalg.norm(uy) * 2)
                res = args[0] if x < 1 or y < 1 else args[0].morphology(x, y, method)
            elif ftype == FE_FLOOD:
                color, region = attrs
                offset, shape, _ = area(region)
                res = Layer.flood(color, offset, shape)
            elif ftype == FE_TURBULENCE:
                freq, octaves, seed, stitch, fractal, region = attrs
                offset, shape, rect = area(region)
                if not rect[2] > 0 or not rect[3] > 0:
                    stitch = False   # (a region without area has no pixel to stitch, and a tile must have one)
                res = Layer.turbulence(transform, offset, shape, freq, octaves, seed, rect if stitch else None, fractal)
            elif ftype == FE_COMPONENT_TRANSFER:
                res = args[0].component_transfer(attrs[0])
            elif ftype == FE_CONVOLVE_MATRIX:
                kernel, divisor, bias, target, edge_mode, preserve_alpha = attrs
                res = args[0].convolve_matrix(kernel, divisor, bias, target, edge_mode, preserve_alpha)
            elif ftype == FE_DISPLACEMENT_MAP:
                scale, x_channel, y_channel = attrs
                res = args[0].displacement_map(args[1], transform, scale, x_channel, y_channel)
            elif ftype == FE_DIFFUSE_LIGHTING:
                light, color, surface_scale, constant, region = attrs
                offset, shape, _ = area(region)
                res = args[0].lighting(transform, offset, shape, light, color, surface_scale, constant)
            elif ftype == FE_SPECULAR_LIGHTING:
                light, color, surface_scale, constant, exponent, region = attrs
                offset, shape, _ = area(region)
                res = args[0].lighting(transform, offset, shape, light, color, surface_scale, constant, exponent)
            elif ftype == FE_TILE:
                # the tile: the input's subregion, or without one the filter region; the output: this primitive's, likewise
                of = None if regions is None else regions(inputs[0])
                tile = frame[1] if of is None else of[1]
                out = frame[1] if box is None else box
                if tile[2] * tile[3] == 0:
                    res = Layer.transparent(out[:2])
                else:
                    res = args[0].tile(out[:2], out[2:], tile[:2], tile[2:])
            elif ftype == FE_IMAGE:
                out, rect = (frame[1], frame[0]) if box is None else (box, sub[0])
                res = self._image(attrs, transform, source, rect)
                res = Layer.transparent(out[:2]) if res is None else res.window(out[:2], out[2:])
            else:
                raise ValueError(f"unsupported filter type: {ftype}")
            if box is not None:   # the result is a layer of exactly the subregion's box
                if res is None:
                    res = Layer.transparent(box[:2])
                elif (int(res.x), int(res.y), res.height, res.width) != box:
                    res = res.window(box[:2], box[2:])
            stack.append(res)
        return get(len(stack) - 1)
