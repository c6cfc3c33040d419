"""SVG front-end: an SVG document -> ``Scene`` (reference ``svg_scene``, S:2803-3625).

Host code: XML in, scene tree out -- the part of the reference that sits in front of the hot path.  It produces
the same tree the reference's loader produces (same node nesting, same paints, same shape-to-path conversions,
the same quirks: gradients do not follow ``href``, shapes go through ``%g``-formatted path data, ``opacity`` makes an
isolated group, the order filter -> opacity -> clip-path -> mask -> transform), so that a scene loaded here renders
exactly like the scene dumps extracted from the reference (``tests/test_svg_loader.py`` compares the trees).

Supported: svg (nested, viewBox), g, defs, path, rect, circle, ellipse, line, polyline, polygon, use,
linearGradient / radialGradient / stop, pattern, clipPath, mask, filter (feOffset, feGaussianBlur, feMerge, feBlend, feComposite,
feColorMatrix matrix / saturate / hueRotate / luminanceToAlpha, feMorphology, and beyond the reference feFlood, feTurbulence,
feComponentTransfer, feConvolveMatrix, feDisplacementMap, feDropShadow, feDiffuseLighting, feSpecularLighting with feDistantLight /
fePointLight / feSpotLight, feTile, feImage (a raster from <image>'s sources, or ``#id``: an element, looked up when the filter runs);
the <filter>'s region for the generators and the lighting primitives; x / y / width / height on a primitive -- its subregion --
and ``primitiveUnits``, see ``filters.py``), text / tspan set in
SVG fonts (font, font-face, glyph, missing-glyph, hkern; ``fonts.py``) or, beyond the reference, in TrueType or OpenType / CFF fonts registered with
the ``FontsDB`` (``truetype.py``, ``opentype_cff.py``: such a run becomes one lazy node whose outline is made on the device at the first render, its
advance is host arithmetic from ``hmtx`` / ``kern``; loading needs no device), presentation attributes and ``style``, and beyond the
reference image (PNG or JPEG, from a base64 ``data:image/png`` / ``data:image/jpeg`` URI or a local file next to the document, the
decoder picked by the data's first bytes; ``png.py``, ``jpeg.py``) and CSS
``mix-blend-mode`` (all 16 modes of Compositing and Blending Level 1, not inherited; applied outermost, after the transform, as a
BLEND node that blends with the earlier siblings in its group node) and ``isolation: isolate`` (the element's content becomes
one group node).  ``plus-lighter``, ``plus-darker`` and unknown modes warn and draw as ``normal``.
Also beyond the reference: dashed strokes -- ``stroke-dasharray`` (comma / white space separated lengths, ``none``),
``stroke-dashoffset`` (both inherited) and ``pathLength`` on path, rect, circle, ellipse, line, polyline and polygon (not
inherited); text strokes take them like any shape.  The pattern rides in the STROKE node's path (``geometry.DashedPath``) and is
applied on the device at the first stroke; loading needs no device.  A percentage or a negative length warns and draws solid;
dashes of length 0 are not drawn (one warning per document).  ``stroke-miterlimit`` stays the reference's 4.
Also beyond the reference: markers -- ``<marker>`` (markerWidth / markerHeight, refX / refY, viewBox, preserveAspectRatio,
markerUnits, orient, overflow) and ``marker-start`` / ``marker-mid`` / ``marker-end`` / ``marker`` (inherited) on path, line,
polyline and polygon.  They become one MARKERS node behind the shape's fill and stroke nodes, which turns into the marker
instances on the device at the first render (``markers.py``); loading needs no device.  A marker is defined before its use.
Also beyond the reference: text on a path -- ``<textPath>`` inside ``<text>`` with ``href`` / ``xlink:href`` to a path, rect,
circle, ellipse, line, polyline or polygon defined before it (its own ``transform`` applied), ``startOffset`` (a length, scaled
by the path's ``pathLength``, or a percentage of the path's length), ``text-anchor``, nested ``<tspan>``s with ``dx`` (along the
path) and ``dy`` (across it); ``x`` / ``y`` inside it are ignored.  It becomes one lazy node (``textpath.py``) that turns into the
runs' fill and stroke nodes, the glyphs placed on the device, at the first render; loading needs no device.  A glyph whose
midpoint is off the path is not drawn, there is no wrap on closed paths, text after the ``<textPath>`` goes on from the pen
where it began; ``method="stretch"``, ``spacing`` and ``side="right"`` warn and the defaults are used.
Also beyond the reference: variable TrueType fonts -- ``font-weight`` picks the ``wght`` of a variable face, ``font-stretch`` (the
nine keywords or a percentage) its ``wdth``, ``font-variation-settings`` (``normal``, or ``"tag" number`` separated by commas) any
axis the face has, and wins over both; all inherited; a malformed value warns and counts as ``normal`` (``truetype_var.py``).
Also beyond the reference: stylesheets and document structure -- ``<style>`` elements and the ``css=`` argument (``css.py``: the
cascade of presentation attributes, rules, the inline ``style`` and ``!important``, see ``_Loader.props``), ``display`` and
``visibility``, ``<symbol>`` (``markers.Symbol``; ``<use>`` with ``width`` / ``height``), ``<switch>`` (``requiredExtensions``,
``systemLanguage`` against ``languages=``), ``<a>`` (a ``<g>``, inside text a ``<tspan>``); ``foreignObject`` draws nothing.
Not supported (a warning, the element is skipped): animation elements, script, ...; <image> of other formats
(GIF, WebP, SVG) or remote URLs.
"""
from __future__ import annotations

import base64
import binascii
import gzip
import io
import math
import os
import re
import warnings
import xml.etree.ElementTree as etree

import numpy as np

from .filters import (
    COLOR_MATRIX_LUM, CONVOLVE_MATRIX_MAX_ORDER, FE_IMAGE, FE_TILE, TRANSFER_MAX_VALUES, TURBULENCE_MAX_OCTAVES, DistantLight, Filter,
    PointLight,
    SpotLight, color_matrix_hue_rotate, color_matrix_saturate,
)
from .fonts import FONT_STYLE_NORMAL, Font, FontsDB, Glyph
from .truetype import SfntFont
from .geometry import (
    PATH_CLOSED, PATH_FILL_NONZERO, PATH_LINE, STROKE_CAP_BUTT, STROKE_JOIN_MITER, Path, Transform,
)
from .layer import BLEND_MODES, COMPOSE_ATOP, COMPOSE_IN, COMPOSE_OUT, COMPOSE_OVER, COMPOSE_XOR
from .css import Matcher, Stylesheet, parse_css, parse_declarations
from .markers import ORIENT_AUTO, ORIENT_AUTO_START_REVERSE, Marker, Symbol
from .textpath import ANCHORS, TextRun
from .paint import GradLinear, GradRadial, Pattern
from .jpeg import read_jpeg
from .jpeg import SIGNATURE as _JPEG_SIGNATURE
from .png import SIGNATURE as _PNG_SIGNATURE
from .png import read_png
from .scene import RENDER_BLEND, RENDER_GROUP, Scene, parse_preserve_aspect_ratio

UNITS_USER = "userSpaceOnUse"
UNITS_BBOX = "objectBoundingBox"
FONT_SIZE = 12  # S:2658

# presentation attributes that children inherit (S:2729-2744)
_INHERITED = {
    "color", "fill", "fill-rule", "fill-opacity", "stroke", "stroke-opacity", "stroke-width", "stroke-linecap",
    "stroke-linejoin", "stroke-miterlimit", "font-family", "font-size", "font-weight", "text-anchor",
    "image-rendering",   # (beyond the reference: <image>)
    "stroke-dasharray", "stroke-dashoffset",   # (beyond the reference: dashed strokes)
    "marker-start", "marker-mid", "marker-end",   # (beyond the reference: markers; the shorthand ``marker`` is spelled out into them)
    "font-variation-settings", "font-stretch",   # (beyond the reference: variable TrueType fonts)
    "visibility",   # (beyond the reference)
}
# the elements whose own ``display`` is read; on the resource elements (clipPath, mask, pattern, marker, symbol, the gradients,
# filter, font, defs) it is ignored, as SVG says, while their children's is honoured
_DISPLAYED = {"svg", "g", "a", "switch", "use", "image", "text", "foreignObject", "path", "rect", "circle", "ellipse", "line", "polyline",
              "polygon"}
_CSS_WIDE = ("initial", "unset")   # keywords (and ``var()``) that warn and drop their declaration
_NOTHING = Scene(RENDER_GROUP, ())   # what the id of an element with ``display: none`` stands for: a <use> of it draws nothing
_MARKER_PROPERTIES = ("marker-start", "marker-mid", "marker-end")
_PATH_SHAPES = {"path", "rect", "circle", "ellipse", "line", "polyline", "polygon"}   # what a <textPath> may reference
_NEAREST = {"pixelated", "optimizespeed", "crisp-edges"}   # image-rendering values that ask for the nearest texel
_NUMBER = re.compile(r"[-+]?(?:(?:\d*\.\d+)|(?:\d+\.?))(?:[Ee][+-]?\d+)?")
_HEX = re.compile("#?([0-9A-Fa-f]+)$")
_FUNC = re.compile(r"\s*(rgba?|hsl)\(([^\)]+)\)\s*")
_TRANSFORM_OP = re.compile(r"\s*(translate|scale|rotate|skewX|skewY|matrix)\s*\(([^\)]+)\)\s*")
_URL = re.compile(r"url\(\#([^)]+)\)")

# CSS named colours (the SVG 1.1 / CSS3 keyword table)
_NAMED = dict(zip(
    """aliceblue antiquewhite aqua aquamarine azure beige bisque black blanchedalmond blue blueviolet brown burlywood
    cadetblue chartreuse chocolate coral cornflowerblue cornsilk crimson cyan darkblue darkcyan darkgoldenrod darkgray
    darkgrey darkgreen darkkhaki darkmagenta darkolivegreen darkorange darkorchid darkred darksalmon darkseagreen
    darkslateblue darkslategray darkslategrey darkturquoise darkviolet deeppink deepskyblue dimgray dimgrey dodgerblue
    firebrick floralwhite forestgreen fuchsia gainsboro ghostwhite gold goldenrod gray grey green greenyellow honeydew
    hotpink indianred indigo ivory khaki lavender lavenderblush lawngreen lemonchiffon lightblue lightcoral lightcyan
    lightgoldenrodyellow lightgray lightgrey lightgreen lightpink lightsalmon lightseagreen lightskyblue lightslategray
    lightslategrey lightsteelblue lightyellow lime limegreen linen magenta maroon mediumaquamarine mediumblue
    mediumorchid mediumpurple mediumseagreen mediumslateblue mediumspringgreen mediumturquoise mediumvioletred
    midnightblue mintcream mistyrose moccasin navajowhite navy oldlace olive olivedrab orange orangered orchid
    palegoldenrod palegreen paleturquoise palevioletred papayawhip peachpuff peru pink plum powderblue purple
    rebeccapurple red rosybrown royalblue saddlebrown salmon sandybrown seagreen seashell sienna silver skyblue
    slateblue slategray slategrey snow springgreen steelblue tan teal thistle tomato turquoise violet wheat white
    whitesmoke yellow yellowgreen""".split(),
    """f0f8ff faebd7 00ffff 7fffd4 f0ffff f5f5dc ffe4c4 000000 ffebcd 0000ff 8a2be2 a52a2a deb887
    5f9ea0 7fff00 d2691e ff7f50 6495ed fff8dc dc143c 00ffff 00008b 008b8b b8860b a9a9a9
    a9a9a9 006400 bdb76b 8b008b 556b2f ff8c00 9932cc 8b0000 e9967a 8fbc8f
    483d8b 2f4f4f 2f4f4f 00ced1 9400d3 ff1493 00bfff 696969 696969 1e90ff
    b22222 fffaf0 228b22 ff00ff dcdcdc f8f8ff ffd700 daa520 808080 808080 008000 adff2f f0fff0
    ff69b4 cd5c5c 4b0082 fffff0 f0e68c e6e6fa fff0f5 7cfc00 fffacd add8e6 f08080 e0ffff
    fafad2 d3d3d3 d3d3d3 90ee90 ffb6c1 ffa07a 20b2aa 87cefa 778899
    778899 b0c4de ffffe0 00ff00 32cd32 faf0e6 ff00ff 800000 66cdaa 0000cd
    ba55d3 9370db 3cb371 7b68ee 00fa9a 48d1cc c71585
    191970 f5fffa ffe4e1 ffe4b5 ffdead 000080 fdf5e6 808000 6b8e23 ffa500 ff4500 da70d6
    eee8aa 98fb98 afeeee db7093 ffefd5 ffdab9 cd853f ffc0cb dda0dd b0e0e6 800080
    663399 ff0000 bc8f8f 4169e1 8b4513 fa8072 f4a460 2e8b57 fff5ee a0522d c0c0c0 87ceeb
    6a5acd 708090 708090 fffafa 00ff7f 4682b4 d2b48c 008080 d8bfd8 ff6347 40e0d0 ee82ee f5deb3 ffffff
    f5f5f5 ffff00 9acd32""".split(),
))
assert len(_NAMED) == 148


# ---------------------------------------------------------------------------------------------------------------------
# scalars
# ---------------------------------------------------------------------------------------------------------------------
def parse_float(text):
    """Number with an optional ``%`` (-> fraction) or ``px`` / ``pt`` suffix (S:3484-3495); None stays None."""
    if text is None or isinstance(text, float):
        return text
    text = text.strip()
    if text.endswith("%"):
        return float(text[:-1]) / 100.0
    if text.endswith("px") or text.endswith("pt"):
        return float(text[:-2])
    return float(text)


def parse_floats(text, at_least=None, at_most=None):
    if text is None:
        return None
    values = [float(v) for v in text.replace(",", " ").split(" ") if v]
    if at_least is not None and len(values) < at_least:
        raise ValueError(f"expected at least {at_least} arguments")
    if at_most is not None and len(values) > at_most:
        raise ValueError(f"expected at most {at_most} arguments")
    return values


def parse_angle(text) -> float:
    """Radians from ``<n>``, ``<n>deg`` (degrees) or ``<n>rad`` (S:3509-3516)."""
    text = text.strip()
    if text.endswith("deg"):
        return float(text[:-3]) * math.pi / 180
    if text.endswith("rad"):
        return float(text[:-3])
    return float(text) * math.pi / 180


def parse_size(text, default=None, dpi=96):
    """A length in user units (S:3519-3549): px, in, cm, mm, pt, pc, em, ex; ``%`` is not resolved."""
    if text is None:
        return default
    if isinstance(text, (int, float)):
        return float(text)
    text = text.strip().lower()
    m = _NUMBER.match(text)
    if m is None:
        warnings.warn(f"invalid size: {text}")
        return default
    value, unit = float(m.group(0)), text[m.end():].strip()
    if unit in ("", "px"):
        return value
    per_inch = {"in": 1, "cm": 2.54, "mm": 25.4, "pt": 72.0, "pc": 6.0}  # multiply by dpi first, then divide
    if unit in per_inch:
        return value * dpi if unit == "in" else value * dpi / per_inch[unit]
    if unit == "em":
        return value * FONT_SIZE
    if unit == "ex":
        return value * FONT_SIZE / 2.0
    if unit == "%":
        warnings.warn("size in % is not supported")
        return value
    return None


def parse_transform(text):
    """``transform`` attribute -> Transform, operations applied left to right (S:3416-3481); None stays None."""
    if text is None:
        return None
    tr = Transform()
    rest = text.strip().replace(",", " ")
    while rest:
        m = _TRANSFORM_OP.match(rest)
        if m is None:
            raise ValueError(f"failed to parse transform: {rest}")
        rest = rest[len(m.group(0)):]
        op, raw = m.groups()
        args = [a for a in raw.split(" ") if a]

        def need(*counts):
            if len(args) not in counts:
                raise ValueError(f"`{op}` transform requires {set(counts)} arguments {len(args)} where given")

        if op == "matrix":
            need(6)
            a, b, c, d, e, f = map(float, args)
            tr = tr.matrix(a, c, e, b, d, f)
        elif op == "translate":
            need(1, 2)
            v = list(map(float, args))
            tr = tr.translate(v[0], v[1] if len(v) == 2 else 0)
        elif op == "scale":
            need(1, 2)
            v = list(map(float, args))
            tr = tr.scale(v[0], v[1] if len(v) == 2 else v[0])
        elif op == "rotate":
            need(1, 3)
            angle = parse_angle(args[0])
            if len(args) == 1:
                tr = tr.rotate(angle)
            else:
                x, y = float(args[1]), float(args[2])
                tr = tr.translate(x, y).rotate(angle).translate(-x, -y)
        elif op == "skewX":
            need(1)
            tr = tr.skew(parse_angle(args[0]), 0)
        else:  # skewY
            need(1)
            tr = tr.skew(0, parse_angle(args[0]))
    return tr


def viewbox_transform(bbox, viewbox) -> Transform:
    """Fit `viewbox` into the viewport `bbox` = (x, y, w, h), uniform scale, centred (S:3116-3133)."""
    vx, vy, vw, vh = viewbox
    x, y, w, h = bbox
    if h is None and w is None:
        h, w = vh, vw
    elif h is None:
        h = vh * w / vw
    elif w is None:
        w = vw * h / vh
    scale = min(w / vw, h / vh)
    tx = -vx + (w / scale - vw) / 2 + x / scale
    ty = -vy + (h / scale - vh) / 2 + y / scale
    return Transform().scale(scale).translate(tx, ty)


# ---------------------------------------------------------------------------------------------------------------------
# colours and paints
# ---------------------------------------------------------------------------------------------------------------------
def _srgb_to_linear(rgba: np.ndarray) -> np.ndarray:
    rgb = rgba[:-1]
    small = rgb <= 0.04045
    rgb[small] = rgb[small] / 12.92
    large = ~small
    rgb[large] = np.power((rgb[large] + 0.055) / 1.055, 2.4)
    return rgba


def parse_color(text):
    """CSS colour -> premultiplied linear RGBA (S:3581-3624): #rgb[a], #rrggbb[aa], rgb()/rgba() with numbers or
    percentages, or a keyword; None (+ warning) when it is none of these."""
    color = None
    m = _HEX.match(text)
    if m is not None:
        digits = m.group(1)
        if len(digits) in (3, 4):
            color = np.array([int(c, 16) for c in digits], dtype=np.float64) / 15.0
        elif len(digits) in (6, 8):
            color = np.array([int(digits[i: i + 2], 16) for i in range(0, len(digits), 2)], dtype=np.float64) / 255.0
        else:
            raise ValueError(f"invalid hex color: {text}")
    m = _FUNC.match(text)
    if m is not None:
        kind, raw = m.groups()
        if kind.strip() not in ("rgb", "rgba"):
            raise ValueError(f"invalid rgb color: {text}")
        channels = []
        for ch in filter(None, raw.replace(",", " ").split(" ")):
            channels.append(float(ch[:-1]) / 100 if ch.endswith("%") else float(ch) / 255.0)
        color = np.array(channels)
    if color is not None:
        if color.shape == (3,):
            color = np.array([*color, 1.0], dtype=np.float64)
        color = _srgb_to_linear(color)
        color[:3] *= color[3:]
        return color
    named = _NAMED.get(text.lower().strip())
    if named is None:
        warnings.warn(f"invalid svg color: {text}")
        return None
    return parse_color("#" + named)


def _resolve_url(text, ids):
    m = _URL.match(text.strip())
    if m is None:
        return None
    target = ids.get(m.group(1))
    if target is None:
        warnings.warn(f"failed to resolve url: {text}")
    return target


def parse_paint(text, ids):
    """``fill`` / ``stroke`` value: none -> None, url(#id) -> the referenced paint, else a colour (S:3564-3578)."""
    if text is None:
        return None
    text = text.strip()
    if text == "none":
        return None
    target = _resolve_url(text, ids)
    if target is not None:
        return target
    color = parse_color(text)
    if color is None:
        warnings.warn(f"invalid paint: {text}")
    return color


def _expand_style(attrib, inherit=None) -> dict:
    """Element attributes with the ``style`` declarations folded in, on top of what the parent hands down (S:3103-3113)."""
    attrs = dict(attrib)
    style = attrs.pop("style", None)
    if style is not None:
        for decl in style.split(";"):
            if decl.strip():
                key, value = decl.split(":", 1)
                attrs[key.strip()] = value.strip()
    return attrs if inherit is None else {**inherit, **attrs}


def _keyword(text) -> str:
    """A CSS keyword compared ASCII case-insensitively (no Unicode case folding)."""
    return text.strip().encode("utf-8").lower().decode("utf-8")


def _props(loader, element, inherit=None) -> dict:
    """An element's properties: the loader's cascade, or without a loader its attributes and inline ``style``."""
    return _expand_style(element.attrib, inherit) if loader is None else loader.props(element, inherit)


def _display_none(attrs) -> bool:
    display = attrs.get("display")
    return display is not None and _keyword(display) == "none"


def _invisible(attrs) -> bool:
    visibility = attrs.get("visibility")
    return visibility is not None and _keyword(visibility) in ("hidden", "collapse")


def _href(attrs):
    href = attrs.get("href")
    if href is None:
        href = next((v for k, v in attrs.items() if k.endswith("}href")), None)
    return href


def _collapse(text, after_blank):
    """The characters of a text node as they are set (S:3737-3745) and whether they end in a blank: white space collapses to
    single blanks; one leading blank is kept unless the previous run ended in one, and one trailing blank.  ``(None,
    after_blank)`` when nothing is set."""
    if not text:
        return None, after_blank
    text = text.replace("\n", " ")
    lead = " " if text[0] in " \t" and len(text) > 1 and not after_blank else ""
    trail = " " if text[-1] in " \t" else ""
    words = " ".join(text.split())
    if not words:
        return None, after_blank
    return lead + words + trail, bool(trail)


def _isolated(group: list) -> list:
    """The nodes of an element with ``isolation: isolate``: one GROUP node, so that a blend inside sees only this content.  A
    single BLEND node has nothing of the element's before it: it draws as its target."""
    if len(group) == 1:
        return [group[0][1][0]] if group[0][0] == RENDER_BLEND else group
    return [Scene.group(group)]


def _gradient_stops(element, loader=None):
    stops = []
    for child in element:
        if not child.tag.endswith("stop"):
            continue
        attrs = _props(loader, child)
        offset = parse_float(attrs.get("offset")) or 0
        offset = min(max(offset, 0), 1)
        color = parse_color(attrs["stop-color"])
        if color is None:
            continue
        opacity = attrs.get("stop-opacity")
        if opacity:
            color *= float(opacity)
        stops.append((offset, color))
    stops.sort(key=lambda s: s[0])
    return stops


def _gradient(element, linear: bool, loader=None):
    """<linearGradient> / <radialGradient> -> GradLinear / GradRadial, a plain colour (one stop) or None (no stops).
    Like the reference (S:2873-2878, S:3181-3249) a gradient is built from its own element only: ``href`` is not followed."""
    attr = element.attrib
    text = attr.get("gradientTransform") or attr.get("transform")
    transform = parse_transform(text) if text is not None else None
    spread = attr.get("spreadMethod", "pad")
    units = attr.get("gradientUnits", UNITS_BBOX)
    if units not in (UNITS_BBOX, UNITS_USER):
        raise ValueError(f"invalid gradient unites: {units}")
    bbox_units = units == UNITS_BBOX
    stops = _gradient_stops(element, loader)
    if not stops:
        return None
    if len(stops) == 1:
        return stops[0][1]
    interp = attr.get("color-interpolation")
    linear_rgb = True if interp == "linearRGB" else (False if interp == "sRGB" else None)
    if linear:
        p0 = np.array([parse_float(attr.get("x1", "0")), parse_float(attr.get("y1", "0"))])
        p1 = np.array([parse_float(attr.get("x2", "1")), parse_float(attr.get("y2", "0"))])
        return GradLinear(p0, p1, stops, transform, spread, bbox_units, linear_rgb)
    cx, cy = parse_float(attr.get("cx", "0.5")), parse_float(attr.get("cy", "0.5"))
    fx, fy = parse_float(attr.get("fx")), parse_float(attr.get("fy"))
    fcenter = None
    if fx is not None or fy is not None:
        fcenter = np.array([cx if fx is None else fx, cy if fy is None else fy])
    radius = parse_float(attr.get("r")) or 0.5
    return GradRadial(np.array([cx, cy]), radius, fcenter, parse_float(attr.get("fr")), stops, transform, spread,
                      bbox_units, linear_rgb)


_COMPOSITE_OPERATORS = {"over": COMPOSE_OVER, "in": COMPOSE_IN, "out": COMPOSE_OUT, "atop": COMPOSE_ATOP, "xor": COMPOSE_XOR}


def _filter_region(attrs):
    """The <filter>'s region (x, y, width, height in filterUnits) in the form of ``filters.FILTER_REGION_DEFAULT``."""
    units = attrs.get("filterUnits", UNITS_BBOX)
    if units not in (UNITS_BBOX, UNITS_USER):
        warnings.warn(f"invalid filter units: {units}")
        units = UNITS_BBOX
    return (units == UNITS_BBOX, *(parse_float(attrs.get(k)) for k in ("x", "y", "width", "height")))


def _flood_color(attrs):
    """flood-color x flood-opacity (attributes or style) as straight-alpha linear RGBA; None (+ warning) if invalid."""
    color = parse_color(attrs.get("flood-color", "black").strip())
    if color is None:
        return None
    opacity = min(max(parse_float(attrs.get("flood-opacity", "1")), 0.0), 1.0)
    alpha = color[3]
    rgb = color[:3] / alpha if alpha > 0 else np.zeros(3)   # (parse_color's colour is premultiplied)
    return (*rgb, alpha * opacity)


_TRANSFER_FUNCS = {"feFuncR": 0, "feFuncG": 1, "feFuncB": 2, "feFuncA": 3}


def _transfer_funcs(element):
    """feFuncR/G/B/A children -> the four transfer functions of ``Layer.component_transfer`` (None = identity)."""
    funcs = [None] * 4
    for child in element:
        k = _TRANSFER_FUNCS.get(child.tag.split("}")[-1])
        if k is None:
            continue
        attrs = child.attrib
        kind = attrs.get("type", "identity")
        if kind in ("table", "discrete"):
            values = parse_floats(attrs.get("tableValues", "")) or []
            funcs[k] = (kind, tuple(values)) if values else None
        elif kind == "linear":
            funcs[k] = ("linear", parse_float(attrs.get("slope", "1")), parse_float(attrs.get("intercept", "0")))
        elif kind == "gamma":
            funcs[k] = ("gamma", parse_float(attrs.get("amplitude", "1")), parse_float(attrs.get("exponent", "1")),
                        parse_float(attrs.get("offset", "0")))
        elif kind != "identity":
            warnings.warn(f"invalid transfer function type: {kind}")
    return funcs


def _convolve_matrix_args(attrs):
    """feConvolveMatrix attributes -> (kernel (orderY, orderX), divisor, bias, (targetX, targetY), edge mode, preserve alpha);
    None (+ warning) when they do not describe a kernel."""
    order = parse_floats(attrs.get("order", "3"), 1, 2)
    ox, oy = (order[0], order[0]) if len(order) == 1 else order
    if ox != int(ox) or oy != int(oy) or ox < 1 or oy < 1:
        warnings.warn(f"invalid convolve matrix order: {attrs.get('order')}")
        return None
    ox, oy = int(ox), int(oy)
    if ox > CONVOLVE_MATRIX_MAX_ORDER or oy > CONVOLVE_MATRIX_MAX_ORDER:
        warnings.warn(f"convolve matrix order above {CONVOLVE_MATRIX_MAX_ORDER}: {attrs.get('order')}")
        return None
    values = parse_floats(attrs.get("kernelMatrix"))
    if values is None or len(values) != ox * oy:
        warnings.warn(f"kernelMatrix needs orderX * orderY = {ox * oy} values: {attrs.get('kernelMatrix')}")
        return None
    kernel = np.array(values, dtype=np.float64).reshape(oy, ox)
    divisor = parse_float(attrs.get("divisor"))
    if divisor == 0:
        warnings.warn("convolve matrix divisor 0: the default divisor is used")
        divisor = None
    tx, ty = (int(parse_float(attrs.get(k, str(o // 2)))) for k, o in (("targetX", ox), ("targetY", oy)))
    if not (0 <= tx < ox and 0 <= ty < oy):
        warnings.warn(f"convolve matrix target outside the kernel: {tx}, {ty}")
        return None
    edge_mode = attrs.get("edgeMode", "duplicate")
    if edge_mode not in ("duplicate", "wrap", "none"):
        warnings.warn(f"invalid edge mode: {edge_mode}")
        return None
    if attrs.get("kernelUnitLength") is not None:
        warnings.warn("kernelUnitLength is not supported: one kernel cell is one device pixel")
    return kernel, divisor, parse_float(attrs.get("bias", "0")), (tx, ty), edge_mode, attrs.get("preserveAlpha") == "true"


def _light_source(element):
    """The first feDistantLight / fePointLight / feSpotLight child as a filters light tuple (user space); None without one."""
    for child in element:
        tag, attrs = child.tag.split("}")[-1], child.attrib

        def num(key, default="0"):
            return parse_float(attrs.get(key, default))

        if tag == "feDistantLight":
            return DistantLight(num("azimuth"), num("elevation"))
        if tag == "fePointLight":
            return PointLight(num("x"), num("y"), num("z"))
        if tag == "feSpotLight":
            cone = attrs.get("limitingConeAngle")
            return SpotLight(num("x"), num("y"), num("z"), num("pointsAtX"), num("pointsAtY"), num("pointsAtZ"),
                             num("specularExponent", "1"), None if cone is None else parse_float(cone))
    return None


def _lighting_args(element, tag, loader=None):
    """feDiffuseLighting / feSpecularLighting -> (light, linear RGB colour, surfaceScale, constant, specularExponent or None);
    None (+ warning) without a light source, with a negative constant or an invalid lighting-color."""
    attrs = _props(loader, element)
    light = _light_source(element)
    if light is None:
        warnings.warn(f"{tag} without a light source")
        return None
    specular = tag == "feSpecularLighting"
    name = "specularConstant" if specular else "diffuseConstant"
    constant = parse_float(attrs.get(name, "1"))
    if constant < 0:
        warnings.warn(f"{tag}: negative {name}: {constant}")
        return None
    color = parse_color(attrs.get("lighting-color", "white").strip())
    if color is None:
        return None
    rgb = color[:3] / color[3] if color[3] > 0 else np.zeros(3)   # (as _flood_color; the alpha is ignored)
    exponent = None
    if specular:
        exponent = parse_float(attrs.get("specularExponent", "1"))
        if not 1.0 <= exponent <= 128.0:
            warnings.warn(f"specularExponent outside [1, 128] clamped: {exponent}")
            exponent = min(max(exponent, 1.0), 128.0)
    if attrs.get("kernelUnitLength") is not None:
        warnings.warn("kernelUnitLength is not supported: one Sobel cell is one device pixel")
    return light, tuple(rgb), parse_float(attrs.get("surfaceScale", "1")), constant, exponent


def _primitive_subregion(attrs, tag, bbox_units):
    """x / y / width / height of a filter primitive in the form of ``Filter.subregion``; None without any.  Under
    userSpaceOnUse a percentage warns and counts as absent (the viewport is not known here); a negative width or height warns
    and leaves the primitive its default subregion (four None)."""
    vals = []
    for key in ("x", "y", "width", "height"):
        text = attrs.get(key)
        if text is not None and text.strip().endswith("%") and not bbox_units:
            warnings.warn(f"{tag}: {key}=\"{text.strip()}\" needs the viewport, which is not known here: ignored")
            text = None
        vals.append(parse_float(text) if bbox_units else parse_size(text))
    if all(v is None for v in vals):
        return None
    if any(v is not None and v < 0 for v in vals[2:]):
        warnings.warn(f"{tag}: negative subregion size: {vals[2]}, {vals[3]}: the default subregion is used")
        return (None, None, None, None)
    return tuple(vals)


# every attribute of a filter primitive, of its feFunc*, light source and feMergeNode children, that holds numbers
_FILTER_NUMBERS = frozenset((
    "x", "y", "width", "height", "baseFrequency", "numOctaves", "seed", "slope", "intercept", "amplitude", "exponent", "offset",
    "tableValues", "order", "kernelMatrix", "divisor", "bias", "targetX", "targetY", "kernelUnitLength", "surfaceScale",
    "diffuseConstant", "specularConstant", "specularExponent", "azimuth", "elevation", "z", "pointsAtX", "pointsAtY", "pointsAtZ",
    "limitingConeAngle", "k1", "k2", "k3", "k4", "scale", "radius", "stdDeviation", "dx", "dy", "values", "flood-opacity"))
_NUMBER_SUFFIXES = ("", "%", "px", "pt", "deg", "rad")


def _non_finite_attribute(element):
    """The name of the first numeric attribute of a filter primitive (or of one of its children) that holds a number which is
    not finite -- ``nan``, ``inf`` or one that overflows, such as ``1e400`` -- or None.  The kernels behind the primitives take
    finite parameters only, so such a primitive is dropped; what is not a number at all is left to the primitive's own parsing."""
    for node in (element, *element):
        for key, text in node.attrib.items():
            if key not in _FILTER_NUMBERS:
                continue
            for token in text.replace(",", " ").split():
                for suffix in _NUMBER_SUFFIXES:
                    if suffix and not token.endswith(suffix):
                        continue
                    try:
                        value = float(token[:len(token) - len(suffix)])
                    except ValueError:
                        continue
                    if not math.isfinite(value):
                        return key if node is element else f"{node.tag.split('}')[-1]} {key}"
                    break
    return None


def _filter(element, loader=None) -> Filter:
    """A primitive with a numeric attribute that is not finite is dropped with a warning naming the attribute (no number makes
    this function raise).  <filter> -> Filter chain (S:3271-3362; feFlood, feTurbulence, feComponentTransfer, feConvolveMatrix, feDisplacementMap,
    feDropShadow, feDiffuseLighting, feSpecularLighting, feTile, feImage, primitive subregions and primitiveUnits beyond the
    reference).  `loader`: the document's loader, which reads feImage's rasters and holds the ids its element references are
    looked up in when the filter runs."""
    region = _filter_region(element.attrib)
    units = element.attrib.get("primitiveUnits")
    if units is not None and units not in (UNITS_BBOX, UNITS_USER):
        warnings.warn(f"invalid primitive units: {units}")
        units = UNITS_USER
    flt = Filter.empty(units == UNITS_BBOX)
    bbox_units = flt.primitive_bbox
    unscaled = set()   # what objectBoundingBox primitive units do not rescale, for one warning
    for child in element:
        tag = child.tag.split("}")[-1]
        attrs = child.attrib
        result, src = attrs.get("result"), attrs.get("in")
        before = len(flt.filters)
        bad = _non_finite_attribute(child) if tag.startswith("fe") else None
        if bad is not None:
            warnings.warn(f"{tag}: {bad} is not finite: the primitive is dropped")
            continue
        sub = _primitive_subregion(attrs, tag, bbox_units) if tag.startswith("fe") else None
        if bbox_units and tag in ("feDiffuseLighting", "feSpecularLighting", "feDisplacementMap"):
            unscaled.add(tag)
        if tag == "feTile":
            flt = flt.tile(src, result)
        elif tag == "feImage":
            flt = _fe_image(flt, child, loader, result)
        elif tag == "feFlood":
            color = _flood_color(_props(loader, child))
            if color is not None:
                flt = flt.flood(color, region, result)
        elif tag == "feTurbulence":
            freq = parse_floats(attrs.get("baseFrequency", "0"), 1, 2)
            fx, fy = (freq[0], freq[0]) if len(freq) == 1 else freq
            kind = attrs.get("type", "turbulence")
            octaves = int(parse_float(attrs.get("numOctaves", "1")))
            if fx < 0 or fy < 0:
                warnings.warn(f"negative baseFrequency: {attrs.get('baseFrequency')}")
            elif kind not in ("turbulence", "fractalNoise"):
                warnings.warn(f"invalid turbulence type: {kind}")
            else:
                flt = flt.turbulence((fx, fy), min(max(octaves, 0), TURBULENCE_MAX_OCTAVES), parse_float(attrs.get("seed", "0")),
                                     attrs.get("stitchTiles") == "stitch", kind == "fractalNoise", region, result)
        elif tag == "feComponentTransfer":
            funcs = _transfer_funcs(child)
            n_values = sum(len(f[1]) for f in funcs if f is not None and f[0] in ("table", "discrete"))
            if n_values > TRANSFER_MAX_VALUES:
                warnings.warn(f"feComponentTransfer: {n_values} table values (at most {TRANSFER_MAX_VALUES})")
            else:
                flt = flt.component_transfer(src, funcs, result)
        elif tag == "feConvolveMatrix":
            args = _convolve_matrix_args(attrs)
            if args is not None:
                flt = flt.convolve_matrix(src, *args, result=result)
        elif tag == "feDisplacementMap":
            xc, yc = attrs.get("xChannelSelector", "A"), attrs.get("yChannelSelector", "A")
            if xc not in ("R", "G", "B", "A") or yc not in ("R", "G", "B", "A"):
                warnings.warn(f"invalid channel selector: {xc}, {yc}")
            else:
                flt = flt.displacement_map(src, attrs.get("in2"), parse_float(attrs.get("scale", "0")), xc, yc, result)
        elif tag == "feDropShadow":
            style = _props(loader, child)
            color = _flood_color(style)
            stds = parse_floats(attrs.get("stdDeviation", "2"), 1, 2)
            std_x, std_y = stds * 2 if len(stds) == 1 else stds
            if color is not None:
                flt = flt.drop_shadow(parse_float(attrs.get("dx", "2")), parse_float(attrs.get("dy", "2")), std_x, std_y, color,
                                      region, src, result, sub)
                sub = None
        elif tag in ("feDiffuseLighting", "feSpecularLighting"):
            args = _lighting_args(child, tag, loader)
            if args is not None:
                light, color, surface_scale, constant, exponent = args
                if exponent is None:
                    flt = flt.diffuse_lighting(src, light, color, surface_scale, constant, region, result)
                else:
                    flt = flt.specular_lighting(src, light, color, surface_scale, constant, exponent, region, result)
        elif tag == "feOffset":
            flt = flt.offset(parse_float(attrs.get("dx", "0")), parse_float(attrs.get("dy", "0")), src, result)
        elif tag == "feGaussianBlur":
            stds = parse_floats(attrs.get("stdDeviation"), 1, 2)
            if stds is not None:
                std_x, std_y = stds * 2 if len(stds) == 1 else stds
                flt = flt.blur(std_x, std_y, src, result)
        elif tag == "feMerge":
            flt = flt.merge([n.get("in") for n in child if n.tag.split("}")[-1] == "feMergeNode"], result)
        elif tag == "feBlend":
            flt = flt.blend(src, attrs.get("in2"), attrs.get("mode"), result)
        elif tag == "feComposite":
            op = attrs.get("operator", "over")
            if op == "arithmetic":
                mode = tuple(parse_float(attrs.get(k, "0")) for k in ("k1", "k2", "k3", "k4"))
            elif op in _COMPOSITE_OPERATORS:
                mode = _COMPOSITE_OPERATORS[op]
            else:
                warnings.warn(f"unsupported composite mode: {op}")
                mode = COMPOSE_OVER
            flt = flt.composite(src, attrs.get("in2"), mode, result)
        elif tag == "feColorMatrix":
            kind, values = attrs.get("type", "matrix"), attrs.get("values")
            if kind == "matrix":
                matrix = np.eye(4, 5) if values is None else np.array(parse_floats(values, 20, 20)).reshape(4, 5)
            elif kind == "saturate":
                matrix = color_matrix_saturate(1 if values is None else parse_float(values))
            elif kind == "hueRotate":
                matrix = color_matrix_hue_rotate(0 if values is None else parse_angle(values))
            elif kind == "luminanceToAlpha":
                matrix = COLOR_MATRIX_LUM
            else:
                warnings.warn(f"unsupported color matrix type: {kind}")
                matrix = None
            if matrix is not None:
                flt = flt.color_matrix(src, matrix, result)
        elif tag == "feMorphology":
            method = {"erode": "min", "dilate": "max"}.get(attrs.get("operator", "erode"))
            if method is None:
                warnings.warn(f"invalid morphology operator: {attrs.get('operator')}")
            radius = parse_floats(attrs.get("radius", "0"), 1, 2)
            rx, ry = (radius[0], radius[0]) if len(radius) == 1 else radius
            if method is not None and rx > 0 and ry > 0:
                flt = flt.morphology(rx, ry, method, src, result)
        else:
            warnings.warn(f"unsupported filter type: {tag}")
        if sub is not None and len(flt.filters) > before:
            flt = flt.subregion(*sub)
    if flt.subregions or flt.primitive_bbox or any(f[0] in (FE_TILE, FE_IMAGE) for f in flt.filters):
        flt = flt._replace(region=region)   # (a chain without any of them stays what it has always been)
    if unscaled:
        warnings.warn(f"primitiveUnits=\"objectBoundingBox\": light positions, surfaceScale and the displacement scale stay in user "
                      f"units ({', '.join(sorted(unscaled))})")
    return flt


def _fe_image(flt: Filter, element, loader, result) -> Filter:
    """<feImage>: a raster (the sources and warnings of <image>) or ``#id``, an element of the document.  Whatever cannot be
    read still takes its place in the chain, with a transparent result."""
    attrs = element.attrib
    href = _href(attrs)
    if href is not None and href.strip().startswith("#"):
        return flt.image(element=href.strip()[1:], ids=None if loader is None else loader.ids, result=result)
    pixels = (loader if loader is not None else _Loader(None, None)).image_pixels(href)
    if pixels is None:
        return flt.image(result=result)
    par = attrs.get("preserveAspectRatio", "xMidYMid meet")
    try:
        parse_preserve_aspect_ratio(par)
    except ValueError:
        warnings.warn(f"invalid preserveAspectRatio: {par!r}, using xMidYMid meet")
        par = "xMidYMid meet"
    smooth = _props(loader, element).get("image-rendering", "auto").strip().lower() not in _NEAREST
    return flt.image(pixels, par, smooth, result=result)


def _font_weight(text) -> int:
    if text is None:
        return 400
    text = text.lower()
    return {"normal": 400, "bold": 700}.get(text) or int(float(text))


_FONT_STRETCH = {"ultra-condensed": 50.0, "extra-condensed": 62.5, "condensed": 75.0, "semi-condensed": 87.5, "normal": 100.0,
                 "semi-expanded": 112.5, "expanded": 125.0, "extra-expanded": 150.0, "ultra-expanded": 200.0}
_VARIATION = re.compile(r"""\s*(?:"([ -~]{4})"|'([ -~]{4})')\s+([-+]?(?:\d*\.\d+|\d+\.?)(?:[Ee][-+]?\d+)?)\s*$""")


def _font_variations(attrs):
    """``{axis tag: value}`` a run asks of a variable font beyond its weight, or None: ``font-stretch`` (a keyword or a
    percentage) sets ``wdth``; ``font-variation-settings`` (``normal``, or a comma-separated list of ``"tag" number``) sets what it
    names and wins.  A malformed value warns and counts as ``normal``."""
    out = {}
    stretch = attrs.get("font-stretch")
    if stretch is not None:
        word = _keyword(stretch)
        value = _FONT_STRETCH.get(word)
        if value is None and word.endswith("%"):
            try:
                value = float(word[:-1])
            except ValueError:
                value = None
            if value is not None and not (value >= 0 and math.isfinite(value)):
                value = None
        if value is None:
            warnings.warn(f"invalid font-stretch: {stretch}")
        else:
            out["wdth"] = value
    settings = attrs.get("font-variation-settings")
    if settings is not None and _keyword(settings) != "normal":
        named = {}
        for item in settings.split(","):
            match = _VARIATION.match(item)
            if match is None or not math.isfinite(float(match.group(3))):
                warnings.warn(f"invalid font-variation-settings: {settings}")
                named = {}
                break
            named[match.group(1) or match.group(2)] = float(match.group(3))
        out.update(named)
    return out or None


def _names_to_unicode(names, by_name) -> list:
    """Glyph names of an hkern ``g1`` / ``g2`` list -> their unicode strings (unknown or unicode-less names drop out)."""
    out = []
    for name in filter(None, (names or "").split(",")):
        glyph = by_name.get(name)
        if glyph is not None and glyph.unicode:
            out.append(glyph.unicode)
    return out


def _font(element, loader=None):
    """<font> -> Font, or None without a <font-face> (S:3627-3702).  Children inherit the <font>'s own attributes, so a
    ``horiz-adv-x`` on the <font> is the default advance; a glyph lacking ``unicode`` or any advance is dropped; kerning
    pairs are the cross product of (u1 + g1) x (u2 + g2), later <hkern> elements overriding earlier ones."""
    glyphs, by_name, kerning = {}, {}, {}
    missing, font = None, None
    for child in element:
        tag = child.tag.split("}")[-1]
        attrs = _props(loader, child, element.attrib)
        if tag == "glyph":
            code, advance = attrs.get("unicode"), attrs.get("horiz-adv-x")
            if code is None or advance is None:
                continue
            glyph = Glyph(code, float(advance), attrs.get("d", ""), attrs.get("glyph-name"))
            glyphs[code] = glyph
            if glyph.name is not None:
                by_name[glyph.name] = glyph
        elif tag == "missing-glyph":
            missing = Glyph(None, float(attrs.get("horiz-adv-x")), attrs.get("d", ""), "missing-glyph")
        elif tag == "font-face":
            upm = float(attrs.get("units-per-em", "2048"))
            font = Font(attrs.get("font-family", f"{id(element)}"), _font_weight(attrs.get("font-weight")),
                        attrs.get("font-style", FONT_STYLE_NORMAL), float(attrs.get("ascent", str(upm))),
                        float(attrs.get("descent", "0")), upm)
        elif tag == "hkern":
            left = list(filter(None, (attrs.get("u1") or "").split(","))) + _names_to_unicode(attrs.get("g1"), by_name)
            right = list(filter(None, (attrs.get("u2") or "").split(","))) + _names_to_unicode(attrs.get("g2"), by_name)
            if attrs.get("k") is None:
                continue
            for a in left:
                for b in right:
                    kerning[(a, b)] = float(attrs["k"])
    if font is None:
        warnings.warn("font is missing `font-face` element")
        return None
    font.glyphs.update(glyphs)
    font.hkern.update(kerning)
    if missing is not None:
        font.missing_glyph = missing
    return font


# ---------------------------------------------------------------------------------------------------------------------
# shapes -> path data (through the same %g-formatted strings the reference builds, S:3365-3413)
# ---------------------------------------------------------------------------------------------------------------------
def rect_path_data(x, y, width, height, rx=None, ry=None) -> str:
    if rx is None or ry is None:
        r = rx if rx is not None else ry
        rx, ry = (r, r) if r is not None else (0, 0)
    rounded = rx > 0 and ry > 0
    d = [f"M{x + rx:g},{y:g}", f"H{x + width - rx:g}"]
    if rounded:
        d.append(f"A{rx:g},{ry:g},0,0,1,{x + width:g},{y + ry:g}")
    d.append(f"V{y + height - ry:g}")
    if rounded:
        d.append(f"A{rx:g},{ry:g},0,0,1,{x + width - rx:g},{y + height:g}")
    d.append(f"H{x + rx:g}")
    if rounded:
        d.append(f"A{rx:g},{ry:g},0,0,1,{x:g},{y + height - ry:g}")
    d.append(f"V{y + ry:g}")
    if rounded:
        d.append(f"A{rx:g},{ry:g},0,0,1,{x + rx:g},{y:g}")
    d.append("z")
    return " ".join(d)


def ellipse_path_data(cx, cy, rx, ry) -> str:
    if rx is None or ry is None:
        r = rx if rx is not None else ry
        if r is None:
            return ""
        rx = ry = r
    return " ".join([
        f"M{cx + rx:g},{cy:g}", f"A{rx:g},{ry:g},0,0,1,{cx:g},{cy + ry:g}", f"A{rx:g},{ry:g},0,0,1,{cx - rx:g},{cy:g}",
        f"A{rx:g},{ry:g},0,0,1,{cx:g},{cy - ry:g}", f"A{rx:g},{ry:g},0,0,1,{cx + rx:g},{cy:g}", "z",
    ])


# ---------------------------------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------------------------------
_IMAGE_MIME_TYPES = {"image/png": "PNG", "image/jpeg": "JPEG", "image/jpg": "JPEG"}
_IMAGE_EXTENSIONS = {".png": "PNG", ".jpg": "JPEG", ".jpeg": "JPEG", ".jpe": "JPEG"}


class _Loader:
    def __init__(self, fg, width, fonts=None, base_dir=None, languages=("en",)):
        self.matcher = None   # css.Matcher when the document has style rules; None: `props` is `_expand_style`
        self.own: dict = {}        # element -> its own cascaded properties (with rules only)
        self.computed: dict = {}   # element -> its properties with what it inherits, for the keyword ``inherit``
        self.css_seen: set = set()   # what the style sheets have warned about (each kind once per document)
        self.languages = tuple(_keyword(tag) for tag in ([languages] if isinstance(languages, str) else languages or ()))
        self.viewports: dict = {}    # id -> (<svg> element, inherited properties where it stands), for <use> with a size
        self.use_size: dict = {}     # <svg> element -> the (width, height) a <use> gives it while it is instantiated
        self.fonts = FontsDB() if fonts is None else fonts
        self.ids: dict = {}
        self.shape_paths: dict = {}   # id -> (path data, transform, pathLength) of the basic shapes and paths, for <textPath>
        self.size = None
        self.fg = fg
        self.width = width
        self.base_dir = base_dir   # the document's directory (<image> files resolve against it); None: not from a file
        self.warned_zero_dash = False

    # -- style -----------------------------------------------------------------------------------------------------------
    def css_warn(self, key, message):
        if key not in self.css_seen:
            self.css_seen.add(key)
            warnings.warn(message)

    def stylesheets(self, root, css=None):
        """Collect the document's <style> elements (a sheet applies to the whole document wherever it stands) and the caller's
        `css`, which goes last: at equal specificity it wins.  Parents and siblings are mapped only if a rule was found."""
        sheet = None
        if root.find(".//{*}style") is not None:
            for element in root.iter():
                if not isinstance(element.tag, str) or element.tag.split("}")[-1] != "style":
                    continue
                kind = element.attrib.get("type")
                if kind is not None and kind.strip() and _keyword(kind) != "text/css":
                    warnings.warn(f"style of type {kind.strip()!r} is not read (only text/css is)")
                    continue
                text = "".join(element.itertext())
                one = parse_css(text, self.css_seen)
                sheet = one if sheet is None else sheet + one
        if css is not None:
            one = css if isinstance(css, Stylesheet) else parse_css(css, self.css_seen)
            sheet = one if sheet is None else sheet + one
        if sheet is not None and len(sheet):
            self.matcher = Matcher(sheet, root)

    def props(self, element, inherit=None) -> dict:
        """An element's properties on top of what the parent hands down.  Without style rules: its attributes with the inline
        ``style`` folded in (`_expand_style`).  With rules, later layers overwriting earlier ones: presentation attributes,
        the rules' normal declarations by specificity and source order, the inline ``style``'s, the rules' ``!important`` ones,
        the inline ``style``'s.  Property names of declarations are lower case; ``inherit`` takes the parent's value."""
        if self.matcher is None:
            return _expand_style(element.attrib, inherit)
        own = self.own.get(element)
        if own is None:
            own = dict(element.attrib)
            style = own.pop("style", None)
            layers = [d for decls in self.matcher.declarations(element) for d in decls]
            inline = parse_declarations(style, self.css_warn) if style is not None else ()
            parent = None
            ordered = ([d for d in layers if not d[2]] + [d for d in inline if not d[2]]
                       + [d for d in layers if d[2]] + [d for d in inline if d[2]])
            for name, value, _important in ordered:
                word = _keyword(value)
                if word in _CSS_WIDE or "var(" in word or name.startswith("--"):
                    self.css_warn("css-wide", "initial, unset and custom properties (var()) are not supported: the declaration is dropped")
                elif word == "inherit":
                    if parent is None:   # (the parent's full dictionary, kept on the walk)
                        parent = {**(inherit or {}), **self.computed.get(self.matcher.parent.get(element), {})}
                    if name in parent:
                        own[name] = parent[name]
                    else:
                        own.pop(name, None)
                else:
                    own[name] = value
            self.own[element] = own
        attrs = dict(own) if inherit is None else {**inherit, **own}
        if inherit is not None:
            self.computed[element] = dict(attrs)
        return attrs

    def image_pixels(self, href):
        """The RGBA pixels an <image> href points at, or None (+ warning): a PNG or JPEG data URI or local file.  The name or
        MIME type says whether the source is worth reading; the decoder is picked by the data's first bytes.  Nothing is ever
        fetched from the network."""
        if not href:
            warnings.warn("image without href")
            return None
        href = href.strip()
        if href[:5].lower() == "data:":
            head, _, payload = href[5:].partition(",")
            params = [p.strip().lower() for p in head.split(";")]
            if params[0] not in _IMAGE_MIME_TYPES or "base64" not in params[1:]:
                warnings.warn(f"unsupported image data: {head or 'text/plain'} (base64 PNG and JPEG are read)")
                return None
            try:
                data = base64.b64decode("".join(payload.split()), validate=True)
            except (binascii.Error, ValueError) as e:
                warnings.warn(f"bad base64 image data: {e}")
                return None
            where, kind = "data URI", _IMAGE_MIME_TYPES[params[0]]
        else:
            if re.match(r"[A-Za-z][A-Za-z0-9+.-]*:", href) and not re.match(r"[A-Za-z]:[\\/]", href):
                warnings.warn(f"image not loaded (only data URIs and local files are read): {href}")
                return None
            kind = _IMAGE_EXTENSIONS.get(os.path.splitext(href)[1].lower())
            if kind is None:
                warnings.warn(f"unsupported image format (PNG and JPEG are read): {href}")
                return None
            if self.base_dir is None:
                warnings.warn(f"image file not loaded (the document is not from a file): {href}")
                return None
            path = os.path.join(self.base_dir, href)
            try:
                with open(path, "rb") as f:
                    data = f.read()
            except OSError as e:
                warnings.warn(f"image file not readable: {href}: {e}")
                return None
            where = href
        # (a JPEG named .png, or the other way round, is read as what it is)
        if data[:len(_PNG_SIGNATURE)] == _PNG_SIGNATURE:
            kind = "PNG"
        elif data[:len(_JPEG_SIGNATURE)] == _JPEG_SIGNATURE:
            kind = "JPEG"
        try:
            return read_png(data) if kind == "PNG" else read_jpeg(data)
        except ValueError as e:
            # (PNG keeps the text it had.  A JPEG source used to be turned away as "unsupported image data" before its bytes
            #  were looked at; one that cannot be decoded still is, now with what is wrong with it)
            what = f"undecodable {kind} ({where}): {e}"
            warnings.warn(what if kind == "PNG" else f"unsupported image data: {what}")
            return None

    def image(self, attrs) -> list:
        """<image>: a fill of the visible part of its viewport with the image as the paint (Scene.image)."""
        if _invisible(attrs):
            return []
        href = attrs.get("href")
        if href is None:
            href = next((v for k, v in attrs.items() if k.endswith("}href")), None)
        pixels = self.image_pixels(href)
        if pixels is None:
            return []
        h, w = pixels.shape[:2]
        x, y = parse_size(attrs.get("x", "0")), parse_size(attrs.get("y", "0"))
        width, height = parse_size(attrs.get("width")), parse_size(attrs.get("height"))
        if width is None and height is None:   # (SVG 2 `auto`: the intrinsic size, or the aspect ratio kept)
            width, height = float(w), float(h)
        elif width is None:
            width = height * w / h
        elif height is None:
            height = width * h / w
        par = attrs.get("preserveAspectRatio", "xMidYMid meet")
        try:
            parse_preserve_aspect_ratio(par)
        except ValueError:
            warnings.warn(f"invalid preserveAspectRatio: {par!r}, using xMidYMid meet")
            par = "xMidYMid meet"
        if x is None or y is None or not (width > 0 and height > 0):
            warnings.warn(f"image with an empty or invalid viewport: {x}, {y}, {width}, {height}")
            return []
        smooth = attrs.get("image-rendering", "auto").strip().lower() not in _NEAREST
        node = Scene.image(pixels, x, y, width, height, par, smooth)
        return [] if node is None else [node]

    # -- leaves --------------------------------------------------------------------------------------------------------
    def shape(self, attrs, path=None) -> list:
        """Fill and stroke scenes of one shape from its (inherited + own) attributes (S:3136-3178); none under
        ``visibility: hidden`` / ``collapse`` (text runs come through here too: a hidden run still advances the pen)."""
        if _invisible(attrs):
            return []
        if path is None:
            d = attrs.get("d")
            if d is None:
                return []
            path = Path.from_svg(d)
        out = []
        fill = attrs.get("fill")
        if fill is not None:
            fill = attrs.get("color") if fill == "currentColor" else parse_paint(fill, self.ids)
        elif self.fg is not None:
            fill = self.fg
        else:
            fill = np.array([0, 0, 0, 1], dtype=np.float64)
        if fill is not None:
            node = Scene.fill(path, fill, attrs.get("fill-rule", PATH_FILL_NONZERO))
            opacity = parse_float(attrs.get("fill-opacity"))
            out.append(node if opacity is None else node.opacity(opacity))
        stroke = attrs.get("stroke")
        stroke = attrs.get("color") if stroke == "currentColor" else parse_paint(stroke, self.ids)
        if stroke is not None:
            node = Scene.stroke(path, stroke, parse_float(attrs.get("stroke-width", "1")), attrs.get("stroke-linecap"),
                                attrs.get("stroke-linejoin"), *self.dashes(attrs))
            opacity = parse_float(attrs.get("stroke-opacity"))
            out.append(node if opacity is None else node.opacity(opacity))
        return out

    def dashes(self, attrs):
        """(dasharray, dashoffset, path_length) of a stroke from ``stroke-dasharray`` / ``stroke-dashoffset`` / ``pathLength``
        (beyond the reference); dasharray None: a solid stroke.  Lengths are comma and / or white space separated sizes.  A
        percentage needs the viewport, which is not known here, and a negative length is an error: both warn and draw solid."""
        text = attrs.get("stroke-dasharray")
        if text is None or _keyword(text) in ("none", ""):
            return None, 0.0, None
        values = []
        for word in text.replace(",", " ").split():
            if word.endswith("%"):
                warnings.warn(f"stroke-dasharray=\"{text.strip()}\" needs the viewport, which is not known here: the stroke is solid")
                return None, 0.0, None
            value = parse_size(word)
            if value is None or not math.isfinite(value):
                warnings.warn(f"invalid stroke-dasharray: {text.strip()}: the stroke is solid")
                return None, 0.0, None
            if value < 0:
                warnings.warn(f"negative stroke-dasharray length: {text.strip()}: the stroke is solid")
                return None, 0.0, None
            values.append(value)
        if not values or not sum(values) > 0:
            return None, 0.0, None
        if len(values) * (2 if len(values) & 1 else 1) > 64:
            warnings.warn("stroke-dasharray with more than 64 lengths (an odd list counts twice): the stroke is solid")
            return None, 0.0, None
        if any(v == 0 for v in (values * 2 if len(values) & 1 else values)[0::2]) and not self.warned_zero_dash:
            self.warned_zero_dash = True   # (once per document)
            warnings.warn("stroke-dasharray: dashes of length 0 are not drawn (no dots from round or square caps)")
        offset = attrs.get("stroke-dashoffset")
        if offset is not None and offset.strip().endswith("%"):
            warnings.warn(f"stroke-dashoffset=\"{offset.strip()}\" needs the viewport, which is not known here: ignored")
            offset = None
        offset = parse_size(offset, 0.0)
        try:
            length = parse_float(attrs.get("pathLength"))
        except ValueError:
            warnings.warn(f"invalid pathLength: {attrs.get('pathLength')}")
            length = None
        if length is not None and not (length > 0 and math.isfinite(length)):
            length = None
        return values, 0.0 if offset is None or not math.isfinite(offset) else offset, length

    def marker(self, element, attrs, inherit) -> Marker:
        """<marker> -> Marker (beyond the reference); its content inherits from the place of definition, as a pattern's does."""
        def size(key, default):
            text = attrs.get(key)
            if text is not None and _keyword(text) in ("left", "center", "right", "top", "bottom"):
                warnings.warn(f"marker: {key}=\"{text.strip()}\" is not supported: 0 is used")
                return 0.0
            value = parse_size(text, default)
            return default if value is None or not math.isfinite(value) else value

        content = self.children(element, inherit)
        units = attrs.get("markerUnits", "strokeWidth")
        if units not in ("strokeWidth", UNITS_USER):
            warnings.warn(f"invalid marker units: {units}")
            units = "strokeWidth"
        orient = _keyword(attrs.get("orient", "0"))
        if orient not in (ORIENT_AUTO, ORIENT_AUTO_START_REVERSE):
            try:
                orient = float(orient[:-3] if orient.endswith("deg") else orient)
                if not math.isfinite(orient):
                    raise ValueError(orient)
            except ValueError:
                warnings.warn(f"invalid marker orient: {attrs.get('orient')}: 0 is used")
                orient = 0.0
        par = attrs.get("preserveAspectRatio", "xMidYMid meet")
        try:
            parse_preserve_aspect_ratio(par)
        except ValueError:
            warnings.warn(f"invalid preserveAspectRatio: {par!r}, using xMidYMid meet")
            par = "xMidYMid meet"
        try:
            viewbox = parse_floats(attrs.get("viewBox"), 4, 4)
        except ValueError:
            warnings.warn(f"invalid marker viewBox: {attrs.get('viewBox')}")
            viewbox = None
        return Marker(Scene.group(content) if content else None, (size("refX", 0.0), size("refY", 0.0)),
                      (size("markerWidth", 3.0), size("markerHeight", 3.0)), None if viewbox is None else tuple(viewbox), par,
                      units == "strokeWidth", orient, _keyword(attrs.get("overflow", "hidden")) not in ("visible", "auto"))

    def marked_shape(self, attrs) -> list:
        """A path, line, polyline or polygon: `shape`, and behind its fill and stroke the markers its ``marker-start`` /
        ``marker-mid`` / ``marker-end`` ask for -- with or without a fill or a stroke, scaled by ``stroke-width`` even then,
        untouched by ``fill-opacity`` / ``stroke-opacity``."""
        refs = []
        for key in _MARKER_PROPERTIES:
            text = attrs.get(key)
            target = None
            if text is not None and _keyword(text) != "none":
                target = _resolve_url(text, self.ids)
                if not isinstance(target, Marker):
                    if target is not None or _URL.match(text.strip()) is None:
                        warnings.warn(f"{key}: not a marker referenced: {text.strip()}")
                    target = None
            refs.append(target)
        d = attrs.get("d")
        if d is None or not any(refs) or _invisible(attrs):
            return self.shape(attrs)
        path = Path.from_svg(d)
        return self.shape(attrs, path) + [Scene.markers(path, *refs, stroke_width=parse_float(attrs.get("stroke-width", "1")))]

    def text(self, element, attrs) -> list:
        """<text> with nested <tspan>: one transformed shape per run of characters (S:3716-3788).

        The pen starts at (0, 0); ``x`` / ``y`` set it, ``dx`` / ``dy`` move it, and each run advances it by its set width.
        White space collapses to single blanks; a run keeps one leading blank unless the previous run ended in one, and
        one trailing blank.  ``text-anchor`` shifts the whole element by its total advance measured from the ``x`` of
        the <text> itself.
        """
        def run(text, attrs, pen, after_blank):
            ox, oy = pen
            for key in ("x", "dx", "y", "dy"):  # consumed here, so that they do not reach the runs that follow
                value = parse_size(attrs.pop(key, None))
                if value is None:
                    continue
                if key == "x":
                    ox = value
                elif key == "y":
                    oy = value
                elif key == "dx":
                    ox += value
                else:
                    oy += value
            words, blank = _collapse(text, after_blank)
            if words is None:
                return [], (ox, oy), after_blank
            size = parse_float(attrs.get("font-size", f"{FONT_SIZE}"))
            font = self.fonts.resolve(attrs.get("font-family"), _font_weight(attrs.get("font-weight")), None, _font_variations(attrs))
            if font is None:
                return [], (ox, oy), after_blank
            if isinstance(font, SfntFont):   # (a TrueType or CFF face: the outline is made on the device, at the first render; the advance is host arithmetic)
                advance = font.str_to_glyphs(words)[1] * (size / font.units_per_em)
                node = Scene.text(font, size, words, dict(attrs), self.shape)
                return [node.transform(Transform().translate(ox, oy))], (ox + advance, oy), blank
            path, advance = font.str_to_path(size, words)
            place = Transform().translate(ox, oy)
            return [node.transform(place) for node in self.shape(attrs, path)], (ox + advance, oy), blank

        def walk(element, attrs, pen, after_blank):
            out, pen, after_blank = run(element.text, attrs, pen, after_blank)
            # whether children are descended into is decided by the tag of ``element`` itself (S:3766-3767)
            descend = element.tag.split("}")[-1] in ("text", "tspan", "a")   # (<a> inside text is a <tspan>)
            for child in element:
                own = self.props(child, attrs) if descend else None
                if own is not None and _display_none(own):   # (sets nothing and advances nothing)
                    pass
                elif descend and child.tag.split("}")[-1] == "textPath":   # (beyond the reference; the pen stays where it is)
                    nodes = self.text_path(child, own)
                    on_path.extend(nodes)
                    out.extend(nodes)
                elif descend:
                    nodes, pen, after_blank = walk(child, own, pen, after_blank)
                    out.extend(nodes)
                nodes, pen, after_blank = run(child.tail, attrs, pen, after_blank)
                out.extend(nodes)
            return out, pen, after_blank

        on_path: list = []   # the nodes of <textPath> children: ``text-anchor`` moves those along their paths instead
        start_x = parse_float(attrs.get("x", "0"))
        nodes, (end_x, _), _ = walk(element, attrs, (0, 0), True)
        anchor = attrs.get("text-anchor")
        if anchor in ("middle", "end"):
            shift = Transform().translate((start_x - end_x) / (2 if anchor == "middle" else 1), 0)
            nodes = [node if any(node is n for n in on_path) else node.transform(shift) for node in nodes]
        return nodes

    def text_path(self, element, attrs) -> list:
        """<textPath> inside <text> (beyond the reference): one lazy node that sets the runs of the element and of its nested
        <tspan>s along the referenced shape -- white space, font, size and paint per run as `text` has them; the distance along
        the path goes on from run to run, ``dx`` moves along the path, ``dy`` across it, ``x`` / ``y`` are ignored."""
        href = attrs.get("href")
        if href is None:
            href = next((v for k, v in attrs.items() if k.endswith("}href")), None)
        target = self.shape_paths.get(href[1:]) if href and href.startswith("#") else None
        if target is None:
            warnings.warn(f"textPath: not a shape referenced: {href}")
            return []
        for key, default in (("method", "align"), ("spacing", "exact"), ("side", "left")):
            value = attrs.get(key)
            if value is not None and _keyword(value) != default:
                warnings.warn(f"textPath: {key}=\"{value.strip()}\" is not supported: {default} is used")
        d, transform, length = target
        path = Path.from_svg(d)
        tr = parse_transform(transform)
        if tr is not None:
            path = path.transform(tr)
        try:
            length = parse_float(length)
        except ValueError:
            warnings.warn(f"invalid pathLength: {length}")
            length = None
        if length is not None and not (length > 0 and math.isfinite(length)):
            length = None
        offset, percent = attrs.get("startOffset", "0").strip(), False
        if offset.endswith("%"):
            offset, percent = offset[:-1], True
        try:
            offset = (parse_float(offset) if percent else parse_size(offset, 0.0)) or 0.0
        except ValueError:
            offset = math.nan
        if not math.isfinite(offset):
            warnings.warn(f"invalid startOffset: {attrs.get('startOffset')}: 0 is used")
            offset, percent = 0.0, False
        anchor = attrs.get("text-anchor")
        if anchor is not None and _keyword(anchor) not in ANCHORS:
            warnings.warn(f"invalid text-anchor: {anchor}")
            anchor = None
        runs = []

        def run(text, attrs, after_blank, moves):
            for key in ("x", "y", "dx", "dy"):  # consumed here, so that they do not reach the runs that follow
                value = parse_size(attrs.pop(key, None))
                if value is not None and key in moves:
                    moves[key] += value
            words, blank = _collapse(text, after_blank)
            if words is None:
                return after_blank
            font = self.fonts.resolve(attrs.get("font-family"), _font_weight(attrs.get("font-weight")), None, _font_variations(attrs))
            if font is None:
                return after_blank
            runs.append(TextRun(words, font, parse_float(attrs.get("font-size", f"{FONT_SIZE}")), dict(attrs), moves["dx"], moves["dy"]))
            moves["dx"] = moves["dy"] = 0.0
            return blank

        def walk(element, attrs, after_blank, moves):
            after_blank = run(element.text, attrs, after_blank, moves)
            for child in element:
                if child.tag.split("}")[-1] in ("tspan", "a"):
                    own = self.props(child, attrs)
                    if not _display_none(own):
                        after_blank = walk(child, own, after_blank, moves)
                after_blank = run(child.tail, attrs, after_blank, moves)
            return after_blank

        walk(element, attrs, True, {"dx": 0.0, "dy": 0.0})   # (moves: the dx / dy met since the last run that was set)
        if not runs:
            return []
        return [Scene.text_on_path(path, runs, offset, percent, length, None if anchor is None else _keyword(anchor), self.shape)]

    def passes(self, element) -> bool:
        """Whether a child of <switch> passes its conditions.  ``requiredExtensions``: any value fails, even an empty one (no
        extension is implemented); ``requiredFeatures`` always passes (SVG 2); ``systemLanguage``: a comma list that passes when
        one entry is one of the loader's `languages` or a prefix of one up to a ``-``, compared case-insensitively."""
        attrib = element.attrib
        if attrib.get("requiredExtensions") is not None:
            return False
        wanted = attrib.get("systemLanguage")
        if wanted is None:
            return True
        for entry in wanted.split(","):
            entry = _keyword(entry)
            if entry and any(tag == entry or tag.startswith(entry + "-") for tag in self.languages):
                return True
        return False

    def symbol(self, element, attrs, inherit) -> Symbol:
        """<symbol> -> Symbol (beyond the reference); its content inherits from the place of definition, as a marker's does."""
        content = self.children(element, inherit)
        par = attrs.get("preserveAspectRatio", "xMidYMid meet")
        try:
            parse_preserve_aspect_ratio(par)
        except ValueError:
            warnings.warn(f"invalid preserveAspectRatio: {par!r}, using xMidYMid meet")
            par = "xMidYMid meet"
        try:
            viewbox = parse_floats(attrs.get("viewBox"), 4, 4)
        except ValueError:
            warnings.warn(f"invalid symbol viewBox: {attrs.get('viewBox')}")
            viewbox = None

        def size(key, default=None):
            text = attrs.get(key)
            if text is not None and text.strip().endswith("%"):
                warnings.warn(f"symbol: {key}=\"{text.strip()}\" needs the viewport, which is not known here: ignored")
                return default
            value = parse_size(text, default)
            return default if value is None or not math.isfinite(value) else value

        return Symbol(Scene.group(content) if content else None, None if viewbox is None else tuple(viewbox), par,
                      size("x", 0.0), size("y", 0.0), size("width"), size("height"),
                      _keyword(attrs.get("overflow", "hidden")) not in ("visible", "auto"))

    def children(self, element, inherit) -> list:
        out = []
        for child in element:
            out.extend(self.element(child, inherit))
        return out

    # -- containers ----------------------------------------------------------------------------------------------------
    def svg(self, element, attrs, inherit, top) -> list:
        group = self.children(element, inherit)
        if not group:
            return []
        scene = Scene.group(group)
        x, y = parse_size(attrs.get("x", "0")), parse_size(attrs.get("y", "0"))
        w, h = parse_size(attrs.get("width")), parse_size(attrs.get("height"))
        if element in self.use_size:   # (a <use> with a size: its width and height override the target's)
            w, h = (given if given is not None else own for given, own in zip(self.use_size[element], (w, h)))
        viewbox = [0, 0, w, h] if w is not None and h is not None else None
        width = self.width if top else None
        if width is not None:
            w, h = (width, int(width * h / w)) if w is not None and h is not None else (width, None)
        viewbox = parse_floats(attrs.get("viewBox"), 4, 4) or viewbox
        if viewbox is not None:
            scene = scene.transform(viewbox_transform((x, y, w, h), viewbox))
            _vx, _vy, vw, vh = viewbox
            if h is None and w is None:
                h, w = vh, vw
            elif h is None:
                h = vh * w / vw
            elif w is None:
                w = vw * h / vh
        elif x > 0 and y > 0:
            scene = scene.transform(Transform().translate(x, y))
        if w is not None and h is not None:
            if top:
                self.size = (w, h)
            else:  # a nested viewport clips its content
                frame = [(PATH_LINE, [[x, y], [x + w, y]]), (PATH_LINE, [[x + w, y], [x + w, y + h]]),
                         (PATH_LINE, [[x + w, y + h], [x, y + h]]), (PATH_CLOSED, [[x, y + h], [x, y]])]
                scene = scene.clip(Scene.fill(Path([frame]), np.ones(4)))
        return [scene]

    def element(self, element, inherit, top=False) -> list:
        tag = element.tag.split("}")[-1]
        attrs = self.props(element, inherit)
        if "marker" in attrs:   # (the shorthand, never handed down itself: this element's; its own longhands go first)
            short, own = attrs.pop("marker"), self.props(element)
            attrs.update({k: short for k in _MARKER_PROPERTIES if k not in own})
        ids = self.ids
        if tag in _DISPLAYED and _display_none(attrs):   # (nothing of it or below it; its id stays known, and stands for nothing)
            if attrs.get("id") is not None:
                ids[attrs["id"]] = _NOTHING
            return []
        up = inherit
        inherit = {k: v for k, v in attrs.items() if k in _INHERITED}
        group: list = []
        if tag == "svg":
            if not top and attrs.get("id") is not None:
                self.viewports[attrs["id"]] = (element, up)
            group = self.svg(element, attrs, inherit, top)
        elif tag == "path":
            group = self.marked_shape(attrs)
        elif tag in ("g", "a"):   # (a link is a group; links are not recorded)
            group = self.children(element, inherit)
        elif tag == "switch":   # (the first direct child that passes its conditions, and nothing else)
            for child in element:
                if self.passes(child):
                    group = self.element(child, inherit)
                    break
        elif tag in ("style", "foreignObject"):   # (the sheets were read before the walk; foreign content draws nothing)
            return []
        elif tag == "symbol":   # (never drawn where it stands)
            if attrs.get("id") is not None:
                ids[attrs["id"]] = self.symbol(element, attrs, inherit)
            return []
        elif tag == "defs":
            self.children(element, inherit)
        elif tag in ("linearGradient", "radialGradient"):
            if attrs.get("id") is not None:
                ids[attrs["id"]] = _gradient(element, tag == "linearGradient", None if self.matcher is None else self)
            return []
        elif tag == "clipPath":
            inherit.setdefault("fill-rule", attrs.get("clip-rule"))
            if attrs.get("id") is not None:
                content = self.children(element, inherit)
                if content:
                    scene = Scene.group(content)
                    tr = parse_transform(attrs.get("transform"))
                    if tr is not None:
                        scene = scene.transform(tr)
                    ids[attrs["id"]] = (scene, attrs.get("clipPathUnits") == UNITS_BBOX)
            return []
        elif tag == "mask":
            if attrs.get("id") is not None:
                scene = Scene.group(self.children(element, inherit))
                tr = parse_transform(attrs.get("transform"))
                if tr is not None:
                    scene = scene.transform(tr)
                ids[attrs["id"]] = (scene, attrs.get("maskContentUnits") == UNITS_BBOX)
        elif tag == "filter":
            if attrs.get("id") is not None:
                ids[attrs["id"]] = _filter(element, self)
        elif tag == "pattern":  # S:2914-2951
            if attrs.get("id") is not None:
                w, h = parse_float(attrs.get("width")), parse_float(attrs.get("height"))
                if w is None or h is None:
                    return []
                content = Scene.group(self.children(element, inherit))
                tr = parse_transform(attrs.get("patternTransform"))
                ids[attrs["id"]] = Pattern(
                    content, attrs.get("patternContentUnits", UNITS_USER) == UNITS_BBOX,
                    parse_floats(attrs.get("viewBox"), 4, 4), parse_float(attrs.get("x", "0")), parse_float(attrs.get("y", "0")),
                    w, h, Transform() if tr is None else tr, attrs.get("patternUnits", UNITS_BBOX) == UNITS_BBOX)
        elif tag == "marker":
            if attrs.get("id") is not None:
                ids[attrs["id"]] = self.marker(element, attrs, inherit)
            return []
        elif tag == "rect":
            x, y = parse_size(attrs.pop("x", "0")), parse_size(attrs.pop("y", "0"))
            w, h = parse_size(attrs.pop("width")), parse_size(attrs.pop("height"))
            attrs["d"] = rect_path_data(x, y, w, h, parse_size(attrs.get("rx")), parse_size(attrs.get("ry")))
            group = self.shape(attrs)
        elif tag == "circle":
            cx, cy = parse_size(attrs.pop("cx", "0")), parse_size(attrs.pop("cy", "0"))
            r = parse_size(attrs.pop("r"))
            attrs["d"] = ellipse_path_data(cx, cy, r, r)
            group = self.shape(attrs)
        elif tag == "ellipse":
            cx, cy = parse_size(attrs.pop("cx", "0")), parse_size(attrs.pop("cy", "0"))
            attrs["d"] = ellipse_path_data(cx, cy, parse_size(attrs.pop("rx")), parse_size(attrs.pop("ry")))
            group = self.shape(attrs)
        elif tag == "polygon":
            attrs["d"] = f"M{attrs.pop('points')}z"
            group = self.marked_shape(attrs)
        elif tag == "polyline":
            attrs["d"] = f"M{attrs.pop('points')}"
            group = self.marked_shape(attrs)
        elif tag == "line":
            x1, y1 = parse_size(attrs.pop("x1", "0")), parse_size(attrs.pop("y1", "0"))
            x2, y2 = parse_size(attrs.pop("x2", "0")), parse_size(attrs.pop("y2", "0"))
            attrs["d"] = f"M{x1},{y1} {x2},{y2}"
            group = self.marked_shape(attrs)
        elif tag in ("title", "desc", "metadata"):
            return []
        elif tag == "font":
            font = _font(element, None if self.matcher is None else self)
            if font is not None:
                self.fonts.register(font, attrs.get("id"))
                if attrs.get("id") is not None:
                    ids[attrs["id"]] = font
            return []
        elif tag == "text":
            group = self.text(element, attrs)
        elif tag == "use":
            x, y = attrs.get("x"), attrs.get("y")
            if x is not None or y is not None:
                attrs["transform"] = attrs.get("transform", "") + f" translate({x}, {y})"
            href = attrs.get("href")
            if href is None:
                href = next((v for k, v in attrs.items() if k.endswith("}href")), None)
            if href and href.startswith("#"):
                item = ids.get(href[1:])
                size = (None, None)
                if isinstance(item, Symbol) or href[1:] in self.viewports:   # (what a width and a height mean something to)
                    size = [attrs.get(key) for key in ("width", "height")]
                    if any(v is not None and v.strip().endswith("%") for v in size):
                        warnings.warn("use: a percentage width or height needs the viewport, which is not known here: ignored")
                        size = [None if v is not None and v.strip().endswith("%") else v for v in size]
                    size = tuple(parse_size(v) for v in size)
                if isinstance(item, Symbol):
                    placed = item.instance(0.0, 0.0, *size)   # (x and y are in the transform already)
                    group = [] if placed is None else [placed]
                elif isinstance(item, Scene) and href[1:] in self.viewports and any(v is not None for v in size):
                    target, where = self.viewports[href[1:]]
                    if target not in self.use_size:   # (not a <use> of an <svg> from inside itself)
                        self.use_size[target] = size
                        try:
                            group = self.element(target, where)
                        finally:
                            del self.use_size[target]
                            ids[href[1:]] = item
                elif isinstance(item, Scene) and item is not _NOTHING:
                    group = [item]
        elif tag == "image":
            group = self.image(attrs)
        else:
            warnings.warn(f"unsupported element type: {tag}")

        if tag in _PATH_SHAPES and attrs.get("id") is not None and attrs.get("d") is not None:
            # (what a <textPath> may reference: the shape's path data, parsed when one does)
            self.shape_paths[attrs["id"]] = (attrs["d"], attrs.get("transform"), attrs.get("pathLength"))
        if not group:
            return group
        isolation = attrs.get("isolation")
        if isolation is not None and _keyword(isolation) not in ("auto", "isolate"):
            warnings.warn(f"unsupported isolation: {isolation}")
        elif isolation is not None and _keyword(isolation) == "isolate":
            group = _isolated(group)
        # decorations, innermost first: filter, group opacity, clip-path, mask; the element's transform goes last, so that
        # clips and masks live in the transformed space (S:3031-3071); beyond the reference, mix-blend-mode outside all of them
        # (it places the element among its siblings)
        name = attrs.get("filter")
        if name is not None:
            flt = _resolve_url(name, ids)
            if isinstance(flt, Filter):
                group = [Scene.group(group).filter(flt)]
            else:
                warnings.warn(f"not a filter referenced {name}: {type(flt)}")
        opacity = parse_float(attrs.get("opacity"))
        if opacity is not None:
            group = [Scene.group(group).opacity(opacity)]
        for key, wrap in (("clip-path", "clip"), ("mask", "mask")):
            ref = attrs.get(key)
            if ref is None:
                continue
            target = _resolve_url(ref, ids)
            if isinstance(target, tuple):
                scene, bbox_units = target
                group = [getattr(Scene.group(group), wrap)(scene, bbox_units)]
            else:
                warnings.warn(f"{key} expected {ref}: {type(target)}")
        tr = parse_transform(attrs.get("transform"))
        if tr is not None:
            group = [node.transform(tr) for node in group]
        blend = attrs.get("mix-blend-mode")
        if blend is not None:
            mode = BLEND_MODES.get(_keyword(blend))
            if mode is None:   # (plus-lighter, plus-darker and anything else: drawn as normal)
                warnings.warn(f"unsupported mix-blend-mode: {blend}")
            elif mode != BLEND_MODES["normal"]:
                group = [Scene.group(group).blend(mode)]
        if attrs.get("id") is not None:
            ids[attrs["id"]] = Scene.group(group)
        return group


def svg_scene(file, fg=None, width=None, fonts=None, base_dir=None, *, css=None, languages=("en",)):
    """Load an SVG document from a file object: ``(Scene | None, ids, size)`` with ``size = (width, height)`` of the
    outermost viewport (S:2803-3083).  ``width`` rescales the document to that many pixels, ``fg`` replaces the default
    black of shapes without a ``fill``, ``fonts`` is the ``FontsDB`` text is set from (<font> elements of the document are
    added to it), ``base_dir`` the directory relative <image> files are read from (None: only data URIs).  ``css``: extra
    author style, text or a ``Stylesheet``, that goes after the document's own <style> sheets (at equal specificity it wins);
    ``languages``: the language tags a <switch> tests ``systemLanguage`` against.  Nothing outside the document is read for
    style: ``<?xml-stylesheet?>``, <link> and ``@import`` are never fetched."""
    loader = _Loader(fg, width, fonts, base_dir, languages)
    root = etree.parse(file).getroot()
    loader.stylesheets(root, css)
    inherit = dict(color=np.array([0.0, 0.0, 0.0, 1.0]) if fg is None else fg)
    group = loader.element(root, inherit, top=True)
    if not group:
        return None, loader.ids, loader.size
    return Scene.group(group), loader.ids, loader.size


def svg_scene_from_str(text: str, fg=None, width=None, fonts=None, *, css=None, languages=("en",)):
    return svg_scene(io.StringIO(text), fg, width, fonts, css=css, languages=languages)


def svg_scene_from_filepath(path: str, fg=None, width=None, fonts=None, *, css=None, languages=("en",)):
    path = os.path.expanduser(path)
    base_dir = os.path.dirname(os.path.abspath(path))
    if os.path.splitext(path)[1] in (".gz", ".svgz"):
        with gzip.open(path, mode="rt", encoding="utf-8") as f:
            return svg_scene(f, fg, width, fonts, base_dir, css=css, languages=languages)
    with open(path, encoding="utf-8") as f:
        return svg_scene(f, fg, width, fonts, base_dir, css=css, languages=languages)


def _output_format(output, format):
    if format is None:
        ext = os.path.splitext(os.fspath(output))[1].lower() if isinstance(output, (str, os.PathLike)) else ""
        return "jpeg" if ext in (".jpg", ".jpeg", ".jpe") else "png"
    if format not in ("png", "jpeg"):
        raise ValueError(f"render_svg: format is 'png' or 'jpeg', not {format!r}")
    return format


def render_svg(svg, output=None, bg=None, fg=None, width=None, id=None, transform=None, linear_rgb=False, fonts=None,
               level=None, threads=None, format=None, quality: int = 90, subsampling: str = "4:2:0", *, encoder: str = "host",
               filter=None, huffman=None, css=None, languages=("en",), palette=None, dither=None, color=None, depth=None):
    """Document in, PNG out: the steps of the reference's command line (S:3796-3877) as one library call, every pixel
    operation on the device.  ``svg`` is a file path or a file object; ``bg`` / ``fg`` are colours as ``parse_color``
    returns them; ``id`` renders a single element (on its own bounding box); ``transform`` is applied on top of the x/y
    swap of presentation space; ``level`` / ``threads`` go to the PNG writer (the defaults, 9 and 1, write the reference's exact
    file, ``threads`` > 1 the same pixels much faster), and so do ``encoder``, ``filter`` and ``huffman``
    (``encoder="device"``: filters and deflate on the device, ``canvas_to_png`` has the details) and ``palette`` (an indexed
    file of at most that many colours, quantised on the device) with ``dither`` ("ordered" or "diffusion").  ``color`` ("rgba",
    "rgb", "grey-alpha", "grey") and ``depth`` (8 or 16) choose the PNG's sample format (``canvas_to_png`` has the rules): "rgb"
    and "grey" have no alpha, so the image lies over ``bg``, or over opaque white when there is none, as a JPEG does.  Returns
    the PNG bytes (also written to ``output``: a path or a binary file object) or None when there is nothing to draw.

    ``format`` is "png" or "jpeg"; None takes it from ``output`` when that is a path ending in ``.jpg``, ``.jpeg`` or
    ``.jpe`` (any case) and is PNG otherwise.  (Before JPEG output existed such a path received PNG bytes.)  A JPEG goes
    through ``Layer.write_jpeg`` with ``quality`` and ``subsampling``: it has no alpha, so the image lies over ``bg``, or over
    opaque white when there is none; its colour transform, DCT and quantiser run on the device, which makes it far quicker
    to write than the PNG.  ``css`` and ``languages`` are ``svg_scene``'s."""
    format = _output_format(output, format)
    if format == "png":   # (bad arguments are refused before the document is read)
        from . import png as png_encoder  # noqa: PLC0415

        png_encoder.dither_argument(dither, png_encoder.palette_argument(palette, png_encoder.encoder_arguments(encoder, level, threads, filter, huffman)[0], filter))
        png_format = png_encoder.format_arguments(color, depth, palette)
    elif color is not None or depth is not None:
        raise ValueError("render_svg: color and depth belong to the PNG format")
    view = Transform().matrix(0, 1, 0, 1, 0, 0)
    if transform is not None:
        view = view @ transform
    if isinstance(svg, (str, os.PathLike)):
        scene, ids, size = svg_scene_from_filepath(os.fspath(svg), fg=fg, width=width, fonts=fonts, css=css, languages=languages)
    else:
        scene, ids, size = svg_scene(svg, fg=fg, width=width, fonts=fonts, css=css, languages=languages)
    if scene is not None and id is not None:
        scene, size = ids.get(id), None
        if isinstance(scene, Symbol):   # (a symbol by id: one instance at the origin, on its own viewport when it has one)
            symbol = scene
            scene, size = symbol.instance(0, 0, None, None), symbol.viewport()
            size = None if None in size else size
        elif not isinstance(scene, Scene):
            raise KeyError(f"no object with id: {id}")
        if scene is _NOTHING:
            return None
    if scene is None:
        return None
    if size is not None:
        w, h = size
        result = scene.render(view, viewport=[0, 0, int(h), int(w)], linear_rgb=linear_rgb)
    else:
        result = scene.render(view, linear_rgb=linear_rgb)
    if result is None:
        return None
    layer, _hull = result
    if size is not None:
        layer = layer.convert(pre_alpha=True, linear_rgb=linear_rgb).on_canvas(int(h), int(w))
    if format == "jpeg":
        return layer.write_jpeg(output, bg=bg, quality=quality, subsampling=subsampling)
    if png_format is not None and png_format[0] in (0, 2):   # (no alpha in the file: write_png puts the layer over bg, or over white)
        png = layer.write_png(None, level, threads, encoder=encoder, filter=filter, huffman=huffman, color=color, depth=depth, bg=bg).getvalue()
    else:
        if bg is not None:
            layer = layer.background(bg)
        png = layer.write_png(None, level, threads, encoder=encoder, filter=filter, huffman=huffman, palette=palette, dither=dither,
                              color=color, depth=depth).getvalue()
    if isinstance(output, (str, os.PathLike)):
        with open(output, "wb") as f:
            f.write(png)
    elif output is not None:
        output.write(png)
    return png
