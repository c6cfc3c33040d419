"""svgrasterize.py_amd -- MI355X-native anti-aliased path coverage + paint + compositing behind
the Scene / Path / Transform / Layer API of aslpavel/svgrasterize.py.

Import as ``svgrasterize_amd`` (alias module at the repository root).  Every pixel operation
runs in hand-written HIP kernels (csrc/svgr_hip.hip) called through the C ABI in include/svgr.h;
there is no CPU fallback.
"""
from ._abi import Context, SvgrError, load_library  # noqa: F401
from .geometry import (  # noqa: F401
    ConvexHull, Path, Transform,
    PATH_LINE, PATH_QUAD, PATH_CUBIC, PATH_ARC, PATH_CLOSED, PATH_UNCLOSED,
    PATH_FILL_NONZERO, PATH_FILL_EVENODD,
)
from .layer import (  # noqa: F401
    Layer, canvas_to_png, canvas_to_jpeg, canvas_create, canvas_compose, canvas_merge_at, canvas_merge_union, canvas_merge_intersect,
    CANVAS_COMPOSE_OVER, COMPOSE_OVER, COMPOSE_OUT, COMPOSE_IN, COMPOSE_ATOP, COMPOSE_XOR,
    BLEND_MODES,
)
from .paint import GradLinear, GradRadial, ImagePaint, Pattern  # noqa: F401
from .jpeg import read_jpeg, write_jpeg  # noqa: F401
from .png import read_png  # noqa: F401
from .filters import (  # noqa: F401
    Filter, blur_kernel, COLOR_MATRIX_LUM, FE_SOURCE_ALPHA, FE_SOURCE_GRAPHIC, FE_BLEND, FE_COLOR_MATRIX, FE_COMPOSITE,
    FE_GAUSSIAN_BLUR, FE_MERGE, FE_MORPHOLOGY, FE_OFFSET,
)
from .scene import (  # noqa: F401
    Scene, HitLeaf, render_canvas, build_batch, clear_render_cache, set_render_cache,
    RENDER_FILL, RENDER_STROKE, RENDER_GROUP, RENDER_OPACITY, RENDER_CLIP, RENDER_MASK, RENDER_TRANSFORM, RENDER_FILTER, RENDER_BLEND,
    RENDER_MARKERS,
)
from .markers import Marker, Symbol  # noqa: F401
from .css import Stylesheet, parse_css  # noqa: F401
from .textpath import TextOnPath, TextOutline, TextRun  # noqa: F401
from .fonts import Font, FontsDB, Glyph  # noqa: F401
from .truetype import TrueTypeFont, read_ttf  # noqa: F401
from .opentype_cff import CFFFont, read_font, read_otf  # noqa: F401
from .truetype_var import Axis  # noqa: F401
from .svg import render_svg, svg_scene, svg_scene_from_filepath, svg_scene_from_str  # noqa: F401
from .tensor import render_to_tensor, render_svgs_to_tensor  # noqa: F401
from .hit import elements_at  # noqa: F401
from .sdf import SdfAtlas, SdfCell  # noqa: F401
from .quant import quantize  # noqa: F401
from .diff import coverage, coverage_backward, coverage_tensor  # noqa: F401
from .diff import compose, compose_backward, compose_tensor, render_tensor  # noqa: F401
from .diff import (GradientPaints, compose_painted, compose_painted_backward, compose_painted_tensor, gradient_paints,  # noqa: F401
                   render_painted_tensor)
from .diff import (Group, Groups, LoweredScene, compose_grouped, compose_grouped_backward, compose_grouped_tensor, group_program,  # noqa: F401
                   lower_scene, render_grouped_tensor)
from .diff import compose_masked, compose_masked_backward, compose_masked_tensor, mask_program, render_masked_tensor  # noqa: F401

__all__ = ["Scene", "Path", "Transform", "Layer", "ConvexHull", "render_canvas", "svg_scene", "svg_scene_from_str",
           "svg_scene_from_filepath", "render_svg", "FontsDB", "clear_render_cache", "set_render_cache", "ImagePaint", "read_png", "read_jpeg",
           "write_jpeg", "canvas_to_jpeg", "Marker", "TextOnPath", "TextRun", "TextOutline", "TrueTypeFont", "read_ttf", "Axis", "CFFFont", "read_otf", "read_font",
           "parse_css", "Stylesheet", "Symbol", "render_to_tensor", "render_svgs_to_tensor", "elements_at", "SdfAtlas", "SdfCell", "quantize",
           "coverage", "coverage_backward", "coverage_tensor", "compose", "compose_backward", "compose_tensor", "render_tensor",
           "GradientPaints", "gradient_paints", "compose_painted", "compose_painted_backward", "compose_painted_tensor", "render_painted_tensor",
           "Group", "Groups", "group_program", "compose_grouped", "compose_grouped_backward", "compose_grouped_tensor", "render_grouped_tensor",
           "LoweredScene", "lower_scene", "mask_program", "compose_masked", "compose_masked_backward", "compose_masked_tensor",
           "render_masked_tensor"]
