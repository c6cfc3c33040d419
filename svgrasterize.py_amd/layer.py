"""Layer: the value type of the hot path (reference S:61-233), with the image resident in HBM.

The reference's Layer is ``NamedTuple(image, offset, pre_alpha, linear_rgb)`` whose image is a
float64 numpy array of shape (rows, cols, 1|4).  This class keeps the same four fields, the same
tuple unpacking and the same methods, but the pixels live in a device buffer until somebody
reads ``.image``; from then on the materialised numpy array is the source of truth (callers such
as the reference's font_speciment.py mutate it in place) and device ops re-upload it.

compose / convert / opacity run as HIP kernels on double images with the reference's operation
order (csrc/svgr_hip.hip: k_layer_*).
"""
from __future__ import annotations

from typing import Sequence

import warnings

import ctypes as C
import math

import numpy as np

from . import _abi

COMPOSE_OVER, COMPOSE_OUT, COMPOSE_IN, COMPOSE_ATOP, COMPOSE_XOR = 0, 1, 2, 3, 4
COMPOSE_PRE_ALPHA = {COMPOSE_OVER, COMPOSE_OUT, COMPOSE_IN, COMPOSE_ATOP, COMPOSE_XOR}
FLOAT = np.float64
# feComponentTransfer / feConvolveMatrix / feDisplacementMap codes of the C ABI (include/svgr.h)
TRANSFER_TYPES = {"identity": 0, "table": 1, "discrete": 2, "linear": 3, "gamma": 4}
EDGE_MODES = {"duplicate": 0, "wrap": 1, "none": 2}
CHANNELS = {"R": 0, "G": 1, "B": 2, "A": 3}
LIGHT_DISTANT, LIGHT_POINT, LIGHT_SPOT = 0, 1, 2   # svgr_layer_lighting's light kinds
# mix-blend-mode codes of svgr_layer_mix_blend (SVGR_BLEND_*), in the order of Compositing and Blending Level 1
(BLEND_NORMAL, BLEND_MULTIPLY, BLEND_SCREEN, BLEND_OVERLAY, BLEND_DARKEN, BLEND_LIGHTEN, BLEND_COLOR_DODGE, BLEND_COLOR_BURN,
 BLEND_HARD_LIGHT, BLEND_SOFT_LIGHT, BLEND_DIFFERENCE, BLEND_EXCLUSION, BLEND_HUE, BLEND_SATURATION, BLEND_COLOR,
 BLEND_LUMINOSITY) = range(16)
BLEND_MODES = {name: code for code, name in enumerate((
    "normal", "multiply", "screen", "overlay", "darken", "lighten", "color-dodge", "color-burn", "hard-light", "soft-light",
    "difference", "exclusion", "hue", "saturation", "color", "luminosity"))}
BLEND_NAMES = {code: name for name, code in BLEND_MODES.items()}
_TURB_M = 2147483647


def turbulence_seed(seed) -> int:
    """feTurbulence ``seed``, truncated toward zero and brought into int64 without changing the lattice it selects: the set-up
    clamps seeds above 2^31 - 2 and folds seeds <= 0 by their C remainder modulo 2^31 - 2.  A seed that is not finite is a
    ValueError, as every non-finite parameter of the filter primitives."""
    seed = float(seed)
    if not math.isfinite(seed):
        raise ValueError(f"feTurbulence seed must be finite: {seed}")
    s = int(seed)
    if s > _TURB_M - 1:
        return _TURB_M - 1
    if s <= 0:
        return -((-s) % (_TURB_M - 1))   # (C's `s % (m - 1)` of a negative s)
    return s


def light_frame(transform, light):
    """(kind, params) of svgr_layer_lighting: `light` (filters.DistantLight / PointLight / SpotLight, user space) in the device
    frame (d0, d1, z).  A point (x, y, z) goes to (transform(x, y), z s), s = sqrt(|det M|) of the linear part M; a distant light
    to (v / |v| cos(elevation), sin(elevation)), v = M (cos(azimuth), sin(azimuth)).  Exact for similarity transforms, an
    approximation under anisotropic ones."""
    from .filters import DistantLight, PointLight, SpotLight

    lin = np.asarray(transform.m, dtype=FLOAT)[:2, :2]
    scale = math.sqrt(abs(lin[0, 0] * lin[1, 1] - lin[0, 1] * lin[1, 0]))
    params = np.zeros(8, dtype=FLOAT)
    if isinstance(light, DistantLight):
        az, el = math.radians(float(light.azimuth)), math.radians(float(light.elevation))
        v = lin @ np.array([math.cos(az), math.sin(az)])
        norm = math.sqrt(v[0] * v[0] + v[1] * v[1])
        if norm > 0:
            params[0:2] = v / norm * math.cos(el)
        params[2] = math.sin(el)
        return LIGHT_DISTANT, params
    if not isinstance(light, (PointLight, SpotLight)):
        raise ValueError(f"unknown light source: {light!r}")
    params[0:2] = transform(np.array([float(light.x), float(light.y)]))
    params[2] = float(light.z) * scale
    if isinstance(light, PointLight):
        return LIGHT_POINT, params
    at = np.array([*transform(np.array([float(light.points_at_x), float(light.points_at_y)])), float(light.points_at_z) * scale])
    d = at - params[0:3]
    norm = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if norm > 0:
        params[3:6] = d / norm
    params[6] = float(light.specular_exponent)
    cone = light.limiting_cone_angle
    params[7] = -1.0 if cone is None else math.cos(math.radians(abs(float(cone))))
    return LIGHT_SPOT, params


def _bbox_arr(offset, shape):
    return (C.c_int64 * 4)(int(offset[0]), int(offset[1]), int(shape[0]), int(shape[1]))


class Layer:
    # `_ops`: the svgr_layer_convert ops the pixels in `_dev` still need to be what `pre_alpha` / `linear_rgb` say they are.  A
    # conversion of a device-resident layer is first only this note: the kernel that reads the layer next (compose OVER, opacity)
    # converts on the way in, everybody else gets the converted pixels from `_device()` / `.image` (one svgr_layer_convert_to).
    __slots__ = ["_host", "_dev", "_shape", "offset", "pre_alpha", "linear_rgb", "_ops"]

    def __init__(self, image, offset, pre_alpha: bool, linear_rgb: bool):
        image = np.asarray(image)
        if image.ndim != 3 or image.shape[2] not in (1, 4):
            raise ValueError("Layer image must have shape (rows, cols, 1|4)")
        self._host = image
        self._dev = None
        self._shape = tuple(image.shape)
        self.offset = offset
        self.pre_alpha = pre_alpha
        self.linear_rgb = linear_rgb
        self._ops = 0

    @classmethod
    def _from_device(cls, buf: "_abi.DeviceBuffer", shape, offset, pre_alpha, linear_rgb, ops: int = 0) -> "Layer":
        self = object.__new__(cls)
        self._host = None
        self._dev = buf
        self._shape = tuple(map(int, shape))
        self.offset = offset
        self.pre_alpha = pre_alpha
        self.linear_rgb = linear_rgb
        self._ops = ops
        return self

    # -- NamedTuple compatibility ---------------------------------------------------------
    def __iter__(self):
        yield self.image
        yield self.offset
        yield self.pre_alpha
        yield self.linear_rgb

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return (self.image, self.offset, self.pre_alpha, self.linear_rgb)[i]

    @property
    def image(self) -> np.ndarray:
        if self._host is None:
            self._host = self._device().download(self._shape, FLOAT)
            self._dev = None  # the host array may be mutated by the caller from now on
        return self._host

    # -- device residency -----------------------------------------------------------------
    def _device(self) -> "_abi.DeviceBuffer":
        """Device buffer holding the current pixels as float64 (uploads a host-resident image)."""
        if self._host is not None:
            return _abi.Context.get().from_host(np.ascontiguousarray(self._host, dtype=FLOAT))
        if self._ops:   # (a noted conversion nobody folded into a kernel of their own: now)
            ctx = _abi.Context.get()
            buf = ctx.alloc(int(np.prod(self._shape)) * 8)
            _abi._check(ctx.lib.svgr_layer_convert_to(ctx.handle, buf.handle, self._dev.handle, self._shape[0] * self._shape[1], self._ops))
            self._dev, self._ops = buf, 0
        return self._dev

    @property
    def on_device(self) -> bool:
        return self._host is None

    # -- reference properties --------------------------------------------------------------
    @property
    def x(self) -> int:
        return self.offset[0]

    @property
    def y(self) -> int:
        return self.offset[1]

    @property
    def width(self) -> int:
        return self._shape[1]

    @property
    def height(self) -> int:
        return self._shape[0]

    @property
    def channels(self) -> int:
        return self._shape[2]

    @property
    def bbox(self):
        return (*self.offset, *self._shape[:2])

    def translate(self, x: int, y: int) -> "Layer":
        out = object.__new__(Layer)
        out._host, out._dev, out._shape, out._ops = self._host, self._dev, self._shape, self._ops
        out.offset = (self.x + x, self.y + y)
        out.pre_alpha, out.linear_rgb = self.pre_alpha, self.linear_rgb
        return out

    def _retag(self, pre_alpha, linear_rgb) -> "Layer":
        out = object.__new__(Layer)
        out._host, out._dev, out._shape, out._ops = self._host, self._dev, self._shape, self._ops
        out.offset, out.pre_alpha, out.linear_rgb = self.offset, pre_alpha, linear_rgb
        return out

    def _copy_device(self) -> "_abi.DeviceBuffer":
        ctx = _abi.Context.get()
        if self._host is not None:
            return ctx.from_host(np.ascontiguousarray(self._host, dtype=FLOAT))
        n = int(np.prod(self._shape))
        out = ctx.alloc(n * 8)
        if self._ops:   # (the copy is the conversion's output)
            _abi._check(ctx.lib.svgr_layer_convert_to(ctx.handle, out.handle, self._dev.handle, self._shape[0] * self._shape[1], self._ops))
        else:
            _abi._check(ctx.lib.svgr_buf_copy(ctx.handle, out.handle, self._dev.handle, n * 8))
        return out

    # -- Layer.convert  S:129-164 ----------------------------------------------------------
    def convert(self, pre_alpha: bool | None = None, linear_rgb: bool | None = None) -> "Layer":
        pre_alpha = self.pre_alpha if pre_alpha is None else pre_alpha
        linear_rgb = self.linear_rgb if linear_rgb is None else linear_rgb
        if self.channels == 1:
            return self._retag(pre_alpha, linear_rgb)  # single channel is alpha: flags only
        ops = 0
        cur_pre = self.pre_alpha
        if self.linear_rgb != linear_rgb:
            if cur_pre:
                ops |= _abi.CONVERT_PRE_TO_STRAIGHT
                cur_pre = False
            ops |= _abi.CONVERT_SRGB_TO_LINEAR if linear_rgb else _abi.CONVERT_LINEAR_TO_SRGB
        if cur_pre != pre_alpha:
            # the kernel applies 1,2,4,8 in that order; "straight -> pre" is last, "pre -> straight" first
            if pre_alpha:
                ops |= _abi.CONVERT_STRAIGHT_TO_PRE
            else:
                ops |= _abi.CONVERT_PRE_TO_STRAIGHT
        if ops == 0:
            return self
        ctx = _abi.Context.get()
        if self._host is not None:
            buf = self._copy_device()
            _abi._check(ctx.lib.svgr_layer_convert(ctx.handle, buf.handle, self._shape[0] * self._shape[1], ops))
            return Layer._from_device(buf, self._shape, self.offset, pre_alpha, linear_rgb)
        # device-resident: noted, not run (`_ops`).  On top of an earlier note the two sets run as one pass when the kernel's order
        # (1, 2, 4, 8) is theirs: every new op behind every noted one; otherwise the noted ones run now.
        if self._ops and (self._ops.bit_length() > (ops & -ops).bit_length() - 1):
            self._device()
        return Layer._from_device(self._dev, self._shape, self.offset, pre_alpha, linear_rgb, self._ops | ops)

    # -- Layer.background  S:166-169 -------------------------------------------------------
    def background(self, color) -> "Layer":
        """The layer over a solid background colour (premultiplied linear RGBA, like every paint)."""
        layer = self.convert(pre_alpha=True, linear_rgb=True)
        ctx = _abi.Context.get()
        buf = layer._copy_device()
        rgba = np.ascontiguousarray(color, dtype=np.float64).reshape(4)
        _abi._check(ctx.lib.svgr_layer_background(ctx.handle, buf.handle, layer._shape[0] * layer._shape[1], rgba.ctypes.data))
        return Layer._from_device(buf, layer._shape, layer.offset, True, True)

    def show(self, format=None) -> None:
        """Print the layer on the terminal through the optional ``imshow`` module (debugging aid, S:220-232)."""
        try:
            from imshow import show  # noqa: PLC0415
        except ImportError:
            warnings.warn("to be able to show layer on terminal imshow is required")
            return
        show(self.convert(pre_alpha=False, linear_rgb=False).image, format=format)
        print()

    # -- Layer.opacity  S:171-175 ----------------------------------------------------------
    def opacity(self, opacity: float, linear_rgb: bool = False) -> "Layer":
        layer = self.convert(pre_alpha=True, linear_rgb=linear_rgb)
        ctx = _abi.Context.get()
        if layer._host is not None:
            buf = layer._copy_device()
            _abi._check(ctx.lib.svgr_layer_scale(ctx.handle, buf.handle, int(np.prod(layer._shape)), float(opacity)))
        elif layer._ops:   # (the conversion and the factor in one pass)
            buf = ctx.alloc(int(np.prod(layer._shape)) * 8)
            _abi._check(ctx.lib.svgr_layer_convert_scale_to(ctx.handle, buf.handle, layer._dev.handle, layer._shape[0] * layer._shape[1],
                                                            layer._ops, float(opacity)))
        else:
            buf = ctx.alloc(int(np.prod(layer._shape)) * 8)
            _abi._check(ctx.lib.svgr_layer_scale_to(ctx.handle, buf.handle, layer._dev.handle, int(np.prod(layer._shape)), float(opacity)))
        return Layer._from_device(buf, layer._shape, layer.offset, True, linear_rgb)

    # -- Layer.convolve  S:106-118 ---------------------------------------------------------
    def color_matrix(self, matrix: np.ndarray) -> "Layer":
        """Apply a 4x5 colour matrix on straight-alpha linear RGBA (Layer.color_matrix, S:95-104)."""
        if not isinstance(matrix, np.ndarray) or matrix.shape != (4, 5):
            raise ValueError("expected 4x5 matrix")
        if self.channels != 4:
            raise ValueError("color_matrix expects an RGBA layer")
        layer = self.convert(pre_alpha=False, linear_rgb=True)
        ctx = _abi.Context.get()
        buf = layer._copy_device() if layer is self else layer._device()  # (a converted layer owns a fresh buffer)
        m = np.ascontiguousarray(matrix, dtype=FLOAT)
        _abi._check(ctx.lib.svgr_layer_color_matrix(ctx.handle, buf.handle, layer.height * layer.width, m.ctypes.data_as(_abi._P)))
        return Layer._from_device(buf, layer._shape, layer.offset, pre_alpha=False, linear_rgb=True)

    def morphology(self, x: int, y: int, method: str) -> "Layer":
        """Morphology = min / max pooling with stride 1 (Layer.morphology S:120-127, pooling S:419-468); the window is
        x rows by y columns of this layer's array, the result shrinks by the window and keeps the offset."""
        if method not in ("min", "max"):
            raise ValueError(f"invalid poll method: {method}")
        if self.channels != 4:
            raise ValueError("morphology expects an RGBA layer")
        layer = self.convert(pre_alpha=True, linear_rgb=True)
        rows, cols = layer.height, layer.width
        x, y = int(x), int(y)
        if x < 1 or y < 1 or x > rows + 1 or y > cols + 1:
            raise ValueError("morphology window does not fit the layer")  # (the reference: negative dimensions, S:455-461)
        ctx = _abi.Context.get()
        if x == rows + 1 or y == cols + 1:
            # One more than the layer: the reference's strided view has a zero-length axis and the result is an empty image
            # (S:455-466), i.e. the shape is eroded / dilated away.  Layers here hold at least one pixel: a transparent one.
            shape = (max(rows - x + 1, 1), max(cols - y + 1, 1), 4)
            out = ctx.alloc(shape[0] * shape[1] * 32)
            out.zero()
            return Layer._from_device(out, shape, layer.offset, pre_alpha=True, linear_rgb=True)
        shape = (rows - x + 1, cols - y + 1, 4)
        out = ctx.alloc(shape[0] * shape[1] * 32)
        src = layer._device()
        _abi._check(ctx.lib.svgr_layer_morphology(ctx.handle, out.handle, src.handle, rows, cols, x, y, int(method == "max")))
        return Layer._from_device(out, shape, layer.offset, pre_alpha=True, linear_rgb=True)

    def luminance_mask(self, linear_rgb: bool) -> "Layer":
        """RENDER_MASK's mask layer (S:733-736): luminance of the straight-alpha colour times alpha, one channel."""
        if self.channels != 4:
            raise ValueError("luminance mask expects an RGBA layer")
        layer = self.convert(pre_alpha=False, linear_rgb=linear_rgb)
        ctx = _abi.Context.get()
        n = layer.height * layer.width
        out = ctx.alloc(max(n, 1) * 8)
        src = layer._device()
        _abi._check(ctx.lib.svgr_layer_luminance(ctx.handle, out.handle, src.handle, n))
        return Layer._from_device(out, (layer.height, layer.width, 1), layer.offset, pre_alpha=False, linear_rgb=linear_rgb)

    def convolve(self, kernel: np.ndarray) -> "Layer":
        """Full 2-D convolution on straight-alpha linear RGBA; offset moves by half the kernel."""
        if self.channels != 4:
            raise ValueError("convolve expects an RGBA layer")
        layer = self.convert(pre_alpha=False, linear_rgb=True)
        kernel = np.ascontiguousarray(kernel, dtype=FLOAT)
        kw, kh = kernel.shape
        ctx = _abi.Context.get()
        rows, cols = layer.height, layer.width
        out_shape = (rows + kw - 1, cols + kh - 1, 4)
        out = ctx.alloc(out_shape[0] * out_shape[1] * 32)
        if layer._host is None and layer._ops:   # (the conversion rides in the blur's first pass)
            _abi._check(ctx.lib.svgr_layer_convolve_ops(ctx.handle, out.handle, layer._dev.handle, rows, cols,
                                                        _abi.ptr(kernel), kw, kh, layer._ops))
        else:
            src = layer._device()
            _abi._check(ctx.lib.svgr_layer_convolve(ctx.handle, out.handle, src.handle, rows, cols, _abi.ptr(kernel), kw, kh))
        offset = (int(layer.x - kw / 2), int(layer.y - kh / 2))
        return Layer._from_device(out, out_shape, offset, pre_alpha=False, linear_rgb=True)

    # -- filter primitives beyond the reference (filters.py; DESIGN.md "Filter primitives beyond the reference") ------
    # Pixel [i, j] of a layer at offset (o0, o1) is the device point (o0 + i + 0.5, o1 + j + 0.5); user space is
    # `transform.invert` of that.  Every result is linear RGB.
    @classmethod
    def flood(cls, color, offset, shape) -> "Layer":
        """feFlood: a (rows, cols) layer at `offset` filled with `color`, straight-alpha linear RGBA."""
        rows, cols = int(shape[0]), int(shape[1])
        rgba = np.ascontiguousarray(color, dtype=FLOAT).reshape(4)
        ctx = _abi.Context.get()
        buf = ctx.alloc(max(rows * cols, 1) * 32)
        buf.zero()   # (then the background kernel's `0 + colour * (1 - 0)` is the colour itself)
        _abi._check(ctx.lib.svgr_layer_background(ctx.handle, buf.handle, rows * cols, _abi.ptr(rgba)))
        return Layer._from_device(buf, (rows, cols, 4), (int(offset[0]), int(offset[1])), pre_alpha=False, linear_rgb=True)

    @classmethod
    def turbulence(cls, transform, offset, shape, base_frequency, num_octaves: int = 1, seed=0, stitch_tile=None,
                   fractal_noise: bool = False) -> "Layer":
        """feTurbulence over a (rows, cols) layer at `offset`: the Filter Effects noise of the user-space point of every pixel
        centre.  `base_frequency` = (fx, fy) >= 0; `seed` is truncated toward zero; `stitch_tile` = (x, y, width, height) in
        user space stitches the noise to that tile, None does not.  Straight-alpha linear RGBA.  Every number must be finite and
        a stitch tile of positive width and height (ValueError before any launch)."""
        rows, cols = int(shape[0]), int(shape[1])
        fx, fy = (float(f) for f in base_frequency)
        seed = turbulence_seed(seed)
        tile = np.ascontiguousarray((0, 0, 0, 0) if stitch_tile is None else stitch_tile, dtype=FLOAT).reshape(4)
        inv = np.ascontiguousarray(transform.invert.m6(), dtype=FLOAT)
        ctx = _abi.Context.get()
        buf = ctx.alloc(max(rows * cols, 1) * 32)
        offset = (int(offset[0]), int(offset[1]))
        _abi._check(ctx.lib.svgr_layer_turbulence(ctx.handle, buf.handle, _bbox_arr(offset, (rows, cols)), _abi.ptr(inv), fx, fy,
                                                  _abi.ptr(tile), seed, int(num_octaves), int(bool(fractal_noise)),
                                                  int(stitch_tile is not None)))
        return Layer._from_device(buf, (rows, cols, 4), offset, pre_alpha=False, linear_rgb=True)

    def component_transfer(self, funcs) -> "Layer":
        """feComponentTransfer on straight-alpha linear RGBA: `funcs` = four transfer functions (R, G, B, A), each None
        (identity) or one of ("identity",), ("table", values), ("discrete", values), ("linear", slope, intercept),
        ("gamma", amplitude, exponent, offset).  The extent stays this layer's: pixels outside it stay transparent."""
        if self.channels != 4:
            raise ValueError("component_transfer expects an RGBA layer")
        if len(funcs) != 4:
            raise ValueError("component_transfer expects four transfer functions (R, G, B, A)")
        types = np.zeros(4, dtype=np.int32)
        params = np.tile(np.array([1.0, 0.0, 1.0, 1.0, 0.0]), (4, 1))   # slope, intercept, amplitude, exponent, offset
        counts = np.zeros(4, dtype=np.int64)
        tables = []
        for k, fn in enumerate(funcs):
            kind = "identity" if fn is None else fn[0]
            if kind not in TRANSFER_TYPES:
                raise ValueError(f"unknown transfer function type: {kind}")
            types[k] = TRANSFER_TYPES[kind]
            if kind in ("table", "discrete"):
                values = np.asarray(fn[1], dtype=FLOAT).reshape(-1)
                if values.size == 0:
                    types[k] = TRANSFER_TYPES["identity"]
                counts[k] = values.size
                tables.append(values)
            elif kind == "linear":
                params[k, 0:2] = fn[1:3]
            elif kind == "gamma":
                params[k, 2:5] = fn[1:4]
        values = np.ascontiguousarray(np.concatenate(tables) if tables else np.zeros(1), dtype=FLOAT)
        params = np.ascontiguousarray(params, dtype=FLOAT)
        if not (np.isfinite(params).all() and np.isfinite(values).all()):   # (the entry's own rule, ahead of the copy below)
            raise ValueError("component_transfer: parameters and table values must be finite")
        layer = self.convert(pre_alpha=False, linear_rgb=True)
        ctx = _abi.Context.get()
        buf = layer._copy_device() if layer is self else layer._device()  # (a converted layer owns a fresh buffer)
        _abi._check(ctx.lib.svgr_layer_component_transfer(ctx.handle, buf.handle, layer.height * layer.width, _abi.ptr(types),
                                                          _abi.ptr(params), _abi.ptr(counts), _abi.ptr(values)))
        return Layer._from_device(buf, layer._shape, layer.offset, pre_alpha=False, linear_rgb=True)

    def convolve_matrix(self, kernel, divisor=None, bias: float = 0.0, target=None, edge_mode: str = "duplicate",
                        preserve_alpha: bool = False) -> "Layer":
        """feConvolveMatrix in device pixels: `kernel` = (orderY, orderX) (rows = vertical = this layer's first axis),
        `target` = (targetX, targetY) (default: order // 2), `divisor` None or 0 = the kernel's sum (1 if that is 0),
        `edge_mode` duplicate / wrap / none at this layer's edges.  Without `preserve_alpha` all four premultiplied
        channels are convolved (result premultiplied); with it the straight colour is convolved and alpha kept."""
        if self.channels != 4:
            raise ValueError("convolve_matrix expects an RGBA layer")
        kernel = np.ascontiguousarray(kernel, dtype=FLOAT)
        if kernel.ndim != 2:
            raise ValueError("convolve_matrix expects a 2-D kernel (orderY, orderX)")
        order_y, order_x = kernel.shape
        tx, ty = (order_x // 2, order_y // 2) if target is None else (int(target[0]), int(target[1]))
        if divisor is None or divisor == 0:
            divisor = float(kernel.sum()) or 1.0
        if edge_mode not in EDGE_MODES:
            raise ValueError(f"invalid edge mode: {edge_mode}")
        if not (np.isfinite(kernel).all() and math.isfinite(divisor) and math.isfinite(bias)):   # (ahead of the conversion below)
            raise ValueError("convolve_matrix: kernel, divisor and bias must be finite")
        layer = self.convert(pre_alpha=not preserve_alpha, linear_rgb=True)
        ctx = _abi.Context.get()
        rows, cols = layer.height, layer.width
        out = ctx.alloc(max(rows * cols, 1) * 32)
        src = layer._device()
        _abi._check(ctx.lib.svgr_layer_convolve_matrix(ctx.handle, out.handle, src.handle, rows, cols, _abi.ptr(kernel), order_x, order_y,
                                                       tx, ty, float(divisor), float(bias), EDGE_MODES[edge_mode],
                                                       int(bool(preserve_alpha))))
        return Layer._from_device(out, layer._shape, layer.offset, pre_alpha=not preserve_alpha, linear_rgb=True)

    def displacement_map(self, map: "Layer", transform, scale: float, x_channel: str = "A", y_channel: str = "A") -> "Layer":
        """feDisplacementMap of this layer (`in`) by `map` (`in2`): the result has the map's extent, and pixel [i, j] is the
        pixel of this layer that contains the map pixel's centre moved by L @ (scale * (map[X] - 0.5), scale * (map[Y] - 0.5)),
        L the linear part of `transform`; X / Y are the selected channels of the straight-alpha map.  Premultiplied."""
        if self.channels != 4 or map.channels != 4:
            raise ValueError("displacement_map expects RGBA layers")
        if x_channel not in CHANNELS or y_channel not in CHANNELS:
            raise ValueError(f"invalid channel selector: {x_channel}, {y_channel}")
        src = self.convert(pre_alpha=True, linear_rgb=True)
        disp = map.convert(pre_alpha=False, linear_rgb=True)
        lin = np.ascontiguousarray(np.asarray(transform.m, dtype=FLOAT)[:2, :2]).reshape(4)
        ctx = _abi.Context.get()
        out = ctx.alloc(max(disp.height * disp.width, 1) * 32)
        s_buf, d_buf = src._device(), disp._device()
        _abi._check(ctx.lib.svgr_layer_displacement_map(ctx.handle, out.handle, _bbox_arr(disp.offset, disp._shape), d_buf.handle,
                                                        s_buf.handle, _bbox_arr(src.offset, src._shape), _abi.ptr(lin), float(scale),
                                                        CHANNELS[x_channel], CHANNELS[y_channel]))
        return Layer._from_device(out, disp._shape, disp.offset, pre_alpha=True, linear_rgb=True)

    def lighting(self, transform, offset, shape, light, color, surface_scale: float, constant: float,
                 specular_exponent=None) -> "Layer":
        """feDiffuseLighting (`specular_exponent` None) or feSpecularLighting over the (rows, cols) region at `offset`, lit by
        `light` (``light_frame``) in `color` (linear RGB).  The surface is this layer's alpha times `surface_scale` in device
        pixels, 0 outside this layer.  Diffuse is opaque; specular is premultiplied (alpha = its largest colour channel)."""
        if self.channels != 4:
            raise ValueError("lighting expects an RGBA layer")
        rows, cols = int(shape[0]), int(shape[1])
        offset = (int(offset[0]), int(offset[1]))
        kind, params = light_frame(transform, light)
        rgb = np.ascontiguousarray(color, dtype=FLOAT).reshape(3)
        specular = specular_exponent is not None
        ctx = _abi.Context.get()
        out = ctx.alloc(max(rows * cols, 1) * 32)
        # only alpha is read, and no noted conversion changes alpha: the pixels as they are
        src = self._dev if self._host is None else self._device()
        _abi._check(ctx.lib.svgr_layer_lighting(ctx.handle, out.handle, _bbox_arr(offset, (rows, cols)), src.handle,
                                                _bbox_arr(self.offset, self._shape), kind, _abi.ptr(params), _abi.ptr(rgb),
                                                float(surface_scale), float(constant),
                                                float(specular_exponent) if specular else 1.0, int(specular)))
        return Layer._from_device(out, (rows, cols, 4), offset, pre_alpha=specular, linear_rgb=True)

    # -- filter primitive subregions and feTile: copies, so the result keeps this layer's alpha convention and colour space ------
    @classmethod
    def transparent(cls, offset, pre_alpha: bool = True, linear_rgb: bool = True) -> "Layer":
        """The empty result of the filter chain (a subregion without pixels): layers hold at least one pixel, so one
        transparent pixel at `offset`."""
        buf = _abi.Context.get().alloc(32)
        buf.zero()
        return cls._from_device(buf, (1, 1, 4), (int(offset[0]), int(offset[1])), pre_alpha, linear_rgb)

    def window(self, offset, shape) -> "Layer":
        """This layer seen through the (rows, cols) box at `offset`: its pixels where it covers the box, transparent black
        elsewhere, bit for bit.  One pass that writes the box whole (``svgr_layer_compose_over`` with this one source)."""
        if self.channels != 4:
            raise ValueError("window expects an RGBA layer")
        rows, cols = int(shape[0]), int(shape[1])
        offset = (int(offset[0]), int(offset[1]))
        if rows <= 0 or cols <= 0:
            return Layer.transparent(offset, self.pre_alpha, self.linear_rgb)
        if offset == (int(self.x), int(self.y)) and (rows, cols) == self._shape[:2]:
            return self
        ctx = _abi.Context.get()
        out = ctx.alloc(rows * cols * 32)
        src = self._dev if self._host is None else self._device()   # (a noted conversion runs as the pixels are read)
        _abi._check(ctx.lib.svgr_layer_compose_over(ctx.handle, out.handle, _bbox_arr(offset, (rows, cols)), 1, (_abi._P * 1)(src.handle),
                                                    _bbox_arr(self.offset, self._shape), (C.c_int32 * 1)(4),
                                                    (C.c_uint32 * 1)(self._ops if self._host is None else 0)))
        return Layer._from_device(out, (rows, cols, 4), offset, self.pre_alpha, self.linear_rgb)

    def tile(self, offset, shape, tile_offset, tile_shape) -> "Layer":
        """feTile: the (rows, cols) = `shape` box at `offset` filled with repeats of the tile -- this layer seen through the
        `tile_shape` box at `tile_offset`, transparent where the layer does not reach it: result[r, c] = tile[(r - tile row0) mod
        tile rows, (c - tile col0) mod tile cols] in device coordinates (floor modulo).  A copy, bit for bit, in one launch
        (``svgr_layer_tile``)."""
        if self.channels != 4:
            raise ValueError("tile expects an RGBA layer")
        rows, cols = int(shape[0]), int(shape[1])
        offset = (int(offset[0]), int(offset[1]))
        if rows <= 0 or cols <= 0 or int(tile_shape[0]) <= 0 or int(tile_shape[1]) <= 0:
            raise ValueError("tile expects a tile and an output of at least one pixel")
        ctx = _abi.Context.get()
        out = ctx.alloc(rows * cols * 32)
        src = self._device()
        _abi._check(ctx.lib.svgr_layer_tile(ctx.handle, out.handle, _bbox_arr(offset, (rows, cols)), src.handle,
                                            _bbox_arr(self.offset, self._shape), _bbox_arr(tile_offset, tile_shape)))
        return Layer._from_device(out, (rows, cols, 4), offset, self.pre_alpha, self.linear_rgb)

    # -- Layer.compose  S:177-207 ----------------------------------------------------------
    @staticmethod
    def compose(layers: Sequence["Layer"], method: int = COMPOSE_OVER, linear_rgb: bool = False) -> "Layer | None":
        if not layers:
            return None
        if len(layers) == 1:
            return layers[0]  # returned as is, unconverted (S:190-191)
        arithmetic = isinstance(method, tuple) and len(method) == 4
        if method not in COMPOSE_PRE_ALPHA and not arithmetic:
            raise ValueError(f"invalid compose mode: {method}")
        if arithmetic or method not in (COMPOSE_OVER, COMPOSE_IN):
            # OUT / ATOP / XOR / feComposite arithmetic: every layer zero-extended to the union canvas, blended one
            # after the other (canvas_merge_union(full=True), S:348-361).  Arithmetic composes straight alpha (S:193).
            pre = not arithmetic
            conv = [l.convert(pre_alpha=pre, linear_rgb=linear_rgb) for l in layers]
            ctx = _abi.Context.get()
            r0 = min(int(l.x) for l in conv)
            c0 = min(int(l.y) for l in conv)
            r1 = max(int(l.x) + l.height for l in conv)
            c1 = max(int(l.y) + l.width for l in conv)
            shape = (r1 - r0, c1 - c0, 4)
            out = ctx.alloc(shape[0] * shape[1] * 32)
            out.zero()
            obb = _bbox_arr((r0, c0), shape)
            k4 = np.array(method if arithmetic else (0, 0, 0, 0), dtype=FLOAT)
            for i, l in enumerate(conv):
                src = l._device()
                if i == 0:
                    _abi._check(ctx.lib.svgr_layer_over(ctx.handle, out.handle, obb, src.handle, _bbox_arr(l.offset, l._shape),
                                                        l.channels, 1))
                else:
                    _abi._check(ctx.lib.svgr_layer_blend(ctx.handle, out.handle, obb, src.handle, _bbox_arr(l.offset, l._shape),
                                                         l.channels, 5 if arithmetic else int(method), k4.ctypes.data_as(_abi._P)))
            offset = (min(l.x for l in conv), min(l.y for l in conv))
            return Layer._from_device(out, shape, offset, pre, linear_rgb)
        conv = [l.convert(pre_alpha=True, linear_rgb=linear_rgb) for l in layers]
        ctx = _abi.Context.get()
        lib = ctx.lib
        if method == COMPOSE_OVER:
            r0 = min(int(l.x) for l in conv)
            c0 = min(int(l.y) for l in conv)
            r1 = max(int(l.x) + l.height for l in conv)
            c1 = max(int(l.y) + l.width for l in conv)
            shape = (r1 - r0, c1 - c0, 4)
            out = ctx.alloc(shape[0] * shape[1] * 32)
            # one pass over the union: every layer read once, converted as it is read (svgr_layer_compose_over)
            n = len(conv)
            srcs = [l._dev if l._host is None else l._device() for l in conv]   # (uploads of host-resident layers stay referenced)
            handles = (_abi._P * n)(*[b.handle for b in srcs])
            bbs = (C.c_int64 * (4 * n))(*[int(v) for l in conv for v in (l.offset[0], l.offset[1], l._shape[0], l._shape[1])])
            chs = (C.c_int32 * n)(*[l.channels for l in conv])
            ops = (C.c_uint32 * n)(*[l._ops if l._host is None else 0 for l in conv])
            _abi._check(lib.svgr_layer_compose_over(ctx.handle, out.handle, _bbox_arr((r0, c0), shape), n, handles, bbs, chs, ops))
            offset = (min(l.x for l in conv), min(l.y for l in conv))
            return Layer._from_device(out, shape, offset, True, linear_rgb)
        # COMPOSE_IN: intersection, S:382-416
        r0 = max(int(l.x) for l in conv)
        c0 = max(int(l.y) for l in conv)
        r1 = min(int(l.x) + l.height for l in conv)
        c1 = min(int(l.y) + l.width for l in conv)
        if r0 >= r1 or c0 >= c1:
            return None
        shape = (r1 - r0, c1 - c0, 4)
        out = ctx.alloc(shape[0] * shape[1] * 32)
        # one pass over the intersection: the first layer cropped, the others multiplied in, each converted as it is read
        n = len(conv)
        srcs = [l._dev if l._host is None else l._device() for l in conv]   # (uploads of host-resident layers stay referenced)
        handles = (_abi._P * n)(*[b.handle for b in srcs])
        bbs = (C.c_int64 * (4 * n))(*[int(v) for l in conv for v in (l.offset[0], l.offset[1], l._shape[0], l._shape[1])])
        chs = (C.c_int32 * n)(*[l.channels for l in conv])
        ops = (C.c_uint32 * n)(*[l._ops if l._host is None else 0 for l in conv])
        _abi._check(lib.svgr_layer_compose_in(ctx.handle, out.handle, _bbox_arr((r0, c0), shape), n, handles, bbs, chs, ops))
        offset = (max(l.x for l in conv), max(l.y for l in conv))
        return Layer._from_device(out, shape, offset, True, linear_rgb)

    @staticmethod
    def mix_blend(backdrop: "Layer | None", source: "Layer | None", mode: int, linear_rgb: bool = False, *,
                  reuse_backdrop: bool = False) -> "Layer | None":
        """`source` blended over `backdrop` with the mix-blend-mode `mode` (``BLEND_*``), both converted to premultiplied in the
        requested colour space as `compose` converts them; the result covers the union of their extents.  With either input
        None the other is returned as it is.  `reuse_backdrop`: the caller owns the backdrop's pixels and drops the backdrop
        (a result made for this blend), so when the source lies inside it the blend runs in place over the source's
        rectangle alone; otherwise a fresh layer is written in one pass over the union."""
        if backdrop is None:
            return source
        if source is None:
            return backdrop
        mode = int(mode)
        if mode not in BLEND_NAMES:
            raise ValueError(f"invalid blend mode: {mode}")
        b = backdrop.convert(pre_alpha=True, linear_rgb=linear_rgb)
        s = source.convert(pre_alpha=True, linear_rgb=linear_rgb)
        ctx = _abi.Context.get()
        # (an upload, or a conversion noted on the converted copy alone, is run into a fresh buffer by _device(); an unconverted
        #  layer's buffer is the caller's)
        fresh = reuse_backdrop or b._host is not None or (b is not backdrop and b._ops != 0)
        bdev = b._device()
        sdev = s._device()
        bbb, sbb = _bbox_arr(b.offset, b._shape), _bbox_arr(s.offset, s._shape)
        inside = (b.channels == 4 and b.x <= s.x and b.y <= s.y and s.x + s.height <= b.x + b.height and
                  s.y + s.width <= b.y + b.width)
        if fresh and inside:
            _abi._check(ctx.lib.svgr_layer_mix_blend(ctx.handle, bdev.handle, bbb, bdev.handle, bbb, 4, sdev.handle, sbb,
                                                     s.channels, mode))
            return Layer._from_device(bdev, b._shape, b.offset, True, linear_rgb)
        r0, c0 = min(b.x, s.x), min(b.y, s.y)
        shape = (max(b.x + b.height, s.x + s.height) - r0, max(b.y + b.width, s.y + s.width) - c0, 4)
        out = ctx.alloc(shape[0] * shape[1] * 32)
        _abi._check(ctx.lib.svgr_layer_mix_blend(ctx.handle, out.handle, _bbox_arr((r0, c0), shape), bdev.handle, bbb, b.channels,
                                                 sdev.handle, sbb, s.channels, mode))
        return Layer._from_device(out, shape, (r0, c0), True, linear_rgb)

    def on_canvas(self, rows: int, cols: int) -> "Layer":
        """This layer merged onto a transparent (rows, cols) canvas at the origin and clipped to [0, 1]: the
        ``canvas_merge_at`` step in front of the PNG writer (S:304-327, S:3866-3870).  Stays on the device."""
        ctx = _abi.Context.get()
        layer = self.convert(pre_alpha=True)
        canvas = ctx.alloc(rows * cols * 32)
        canvas.zero()
        src = layer._device()  # (a host-resident layer's upload is a temporary: it must outlive the call)
        _abi._check(ctx.lib.svgr_layer_over(ctx.handle, canvas.handle, _bbox_arr((0, 0), (rows, cols)), src.handle,
                                            _bbox_arr(layer.offset, layer._shape), layer.channels, 0))
        _abi._check(ctx.lib.svgr_layer_clip01(ctx.handle, canvas.handle, rows * cols * 4))
        return Layer._from_device(canvas, (rows, cols, 4), (0, 0), True, layer.linear_rgb)

    def to_canvas_f32(self, rows: int, cols: int, clip01: bool = True) -> np.ndarray:
        """Place this layer on a zero (rows, cols, 4) canvas (canvas_merge_at, S:304-327) and
        return float32 premultiplied RGBA."""
        ctx = _abi.Context.get()
        layer = self.convert(pre_alpha=True)
        canvas = ctx.alloc(rows * cols * 32)
        canvas.zero()
        src = layer._device()
        _abi._check(ctx.lib.svgr_layer_over(ctx.handle, canvas.handle, _bbox_arr((0, 0), (rows, cols)),
                                            src.handle, _bbox_arr(layer.offset, layer._shape),
                                            layer.channels, 0))
        out32 = ctx.alloc(rows * cols * 16)
        _abi._check(ctx.lib.svgr_layer_to_f32(ctx.handle, out32.handle, canvas.handle, rows * cols * 4, int(clip01)))
        return out32.download((rows, cols, 4), np.float32)

    def _to_rgba8_device(self):
        """(device buffer, rows, cols): the bytes of ``to_rgba8``, still on the device."""
        if self.channels != 4:
            raise ValueError("Only RGBA layers are supported")
        ctx = _abi.Context.get()
        layer = self.convert(pre_alpha=False, linear_rgb=False)
        src = layer._device()
        rows, cols = layer._shape[0], layer._shape[1]
        out = ctx.alloc(max(rows * cols * 4, 4))
        _abi._check(ctx.lib.svgr_layer_to_rgba8(ctx.handle, out.handle, src.handle, rows * cols))
        return out, rows, cols

    def to_rgba8(self) -> np.ndarray:
        """(rows, cols, 4) uint8: straight-alpha sRGB, ``np.round(image * 255).astype(np.uint8)`` (S:211-212, S:262),
        converted and quantised on the device; only the bytes cross PCIe (4 B per pixel instead of 32)."""
        out, rows, cols = self._to_rgba8_device()
        return out.download((rows, cols, 4), np.uint8)

    def _png_samples_device(self, fmt, kind, bg):
        """(device buffer, rows, cols, depth): the packed samples of the layer under a format of ``png.format_arguments``."""
        from . import png  # noqa: PLC0415

        colour_type, depth = fmt[0], 8 if fmt[1] is None else fmt[1]
        layer = self
        if kind == _abi.PNG_SRC_RGBA_F64:
            if colour_type in (0, 2):   # (no alpha in the file: the layer goes over its background first, as write_jpeg does)
                layer = layer.background((1.0, 1.0, 1.0, 1.0) if bg is None else bg)
            layer = layer.convert(pre_alpha=False, linear_rgb=False)
        rows, cols = layer._shape[0], layer._shape[1]
        if rows <= 0 or cols <= 0:
            raise ValueError(f"a PNG image has at least one pixel, not {cols} x {rows}")
        return png.samples_device(layer._device(), kind, rows, cols, colour_type, depth), rows, cols, depth

    def write_png(self, output=None, level=None, threads=None, *, encoder: str = "host", filter=None, huffman=None, palette=None, dither=None,
                  color=None, depth=None, bg=None):
        """PNG of the layer (Layer.write_png, S:209-213): 8-bit RGBA, filter 0, one IDAT -- byte-identical to the
        reference's file at the reference's zlib level 9 (``level``, default 9, trades size for speed; ``threads``, default 1,
        compresses in parallel pieces; the pixels are the same).  ``encoder="device"`` filters and compresses on the device
        instead (``canvas_to_png`` has the details): the bytes go from the 8-bit conversion straight into the filter kernel
        and only the compressed stream crosses PCIe.  It takes ``filter`` and ``huffman`` in place of ``level`` and
        ``threads``.  ``palette`` (True, or the largest number of entries, 2 .. 256) writes an indexed file instead: the colours
        are quantised on the device (``quantize``) and only the index rows reach either encoder; ``dither`` ("ordered" or
        "diffusion"; None and "none": no dithering) goes with it.

        ``color`` ("rgba", "rgb", "grey-alpha", "grey"; "gray" is read too) and ``depth`` (8 or 16) choose another sample format
        (``canvas_to_png`` has the rules); with neither, the file is the one described above.  The samples are made on the
        device from the float layer, so depth 16 keeps what 8 bits round away.  "rgb" and "grey" have no alpha: the layer goes
        over ``bg`` first (premultiplied linear RGBA like every paint; default opaque white), as in ``write_jpeg``; with the
        other two ``bg`` is a ValueError.  A one-channel layer (``Path.mask``) is written with ``color="grey"`` only.  Neither
        goes with ``palette``."""
        from . import png  # noqa: PLC0415

        args = png.encoder_arguments(encoder, level, threads, filter, huffman)
        max_colors = png.palette_argument(palette, args[0], filter)
        dither = png.dither_argument(dither, max_colors)
        fmt = png.format_arguments(color, depth, palette)
        if fmt is not None:
            kind = png.layer_format_arguments(fmt, self.channels, bg)
            buf, rows, cols, depth = self._png_samples_device(fmt, kind, bg)
            return png.encode_samples(buf, rows, cols, fmt[0], depth, output, args)
        if bg is not None:
            raise ValueError('bg goes with the formats without alpha, color="rgb" and color="grey"')
        if max_colors is not None:
            buf, rows, cols = self._to_rgba8_device()
            kw = {"huffman": huffman} if args[0] == "device" else {"level": args[1], "threads": args[2]}
            return png.encode_indexed(buf, rows, cols, output, max_colors, encoder=args[0], dither=dither, **kw)
        if args[0] == "device":
            buf, rows, cols = self._to_rgba8_device()
            return png.encode_rgba8(buf, rows, cols, output, filter, huffman)
        return canvas_to_png(self.to_rgba8(), output, level=args[1], threads=args[2])

    def write_jpeg(self, output=None, bg=None, **kw) -> bytes:
        """Baseline JFIF JPEG of the layer (beyond the reference); returns the file's bytes, also written to ``output`` (a path
        or a binary file object).  JPEG has no alpha: the layer goes over ``bg`` (premultiplied linear RGBA like every paint;
        default opaque white) in float on the device, is quantised to 8 bits there, and the bytes go straight into the encoder's
        device stage -- only the int16 DCT coefficients cross PCIe.  ``kw``: ``jpeg.write_jpeg``'s ``quality``,
        ``subsampling``, ``grey``, ``optimize``, ``restart_interval``."""
        from . import jpeg  # noqa: PLC0415

        unknown = set(kw) - {"quality", "subsampling", "grey", "optimize", "restart_interval"}
        if unknown:
            raise TypeError(f"write_jpeg: unexpected arguments {sorted(unknown)}")
        args = {"quality": 90, "subsampling": "4:2:0", "grey": False, "optimize": True, "restart_interval": 0, **kw}
        jpeg.quant_tables(args["quality"])   # (bad arguments are refused before any device work)
        if args["subsampling"] not in jpeg.SUBSAMPLINGS:
            raise ValueError(f"JPEG subsampling is one of {', '.join(jpeg.SUBSAMPLINGS)}, not {args['subsampling']!r}")
        if self.channels != 4:
            raise ValueError("Only RGBA layers are supported")
        buf, rows, cols = self.background((1.0, 1.0, 1.0, 1.0) if bg is None else bg)._to_rgba8_device()
        return jpeg._encode_rgba8(buf, rows, cols, output, **args)

    # -- tensor output (beyond the reference; tensor.py) -----------------------------------------------------------------------
    def to_array(self, size=None, *, dtype=np.float32, layout="chw", channels="rgba", alpha="premultiplied", linear_rgb=False,
                 bg=None, mean=None, std=None) -> np.ndarray:
        """The layer packed on the device and downloaded as numpy: ``dtype`` float32, float16 or uint8 (rounded to nearest-even;
        uint8 is ``round(v * 255)`` saturated), ``layout`` "chw" (planar) or "hwc", ``channels`` "rgba", "rgb", "alpha" or "luma".
        ``size=(rows, cols)`` places the layer on a transparent plane at the origin, as ``on_canvas`` does; without it the plane
        is the layer's own extent.  ``alpha`` ("premultiplied" or "straight") and ``linear_rgb`` say what the pixels are to be
        (``Layer.convert``); ``bg``, three premultiplied colour values in that colour space, puts the picture over an opaque
        background; ``mean`` / ``std`` (one value, or one per output channel) give ``(v - mean) / std``.  Only the packed
        bytes cross PCIe: 2 per value for float16 where ``Layer.image`` moves 8.  Needs no torch."""
        from . import tensor  # noqa: PLC0415

        return tensor.to_array(self, size, dtype=dtype, layout=layout, channels=channels, alpha=alpha, linear_rgb=linear_rgb, bg=bg,
                               mean=mean, std=std)

    def to_tensor(self, out=None, size=None, *, dtype=None, layout="chw", channels="rgba", alpha="premultiplied", linear_rgb=False,
                  bg=None, mean=None, std=None):
        """``to_array`` into a ``torch.Tensor`` on the context's device, never leaving it.  ``dtype`` is torch.float32 (the
        default), float16, bfloat16 or uint8.  ``out`` may be any view whose last three dimensions are (C, rows, cols) or
        (rows, cols, C) with unit stride along a row's elements -- ``batch[n]``, a window ``big[:, 1:1 + rows, 3:3 + cols]`` --;
        nothing outside it is written.  A wrong dtype is a TypeError, a wrong shape or device a ValueError, before any device
        work.  The call orders itself against ``torch.cuda.current_stream()`` on the device: torch work queued on ``out``
        before and after it is safe, and the host is not made to wait.  torch must have been imported, and have touched CUDA,
        before this package's first call (tensor.py)."""
        from . import tensor  # noqa: PLC0415

        return tensor.to_tensor(self, out, size, dtype=dtype, layout=layout, channels=channels, alpha=alpha, linear_rgb=linear_rgb,
                                bg=bg, mean=mean, std=std)

    @staticmethod
    def from_tensor(t, offset=(0, 0), pre_alpha=True, linear_rgb=False, channels=None, layout=None) -> "Layer":
        """A device-resident layer from a ``torch.Tensor`` on the device (or a numpy array, which is uploaded as it is): float32,
        float16, bfloat16 or uint8 (``v / 255``), widened exactly.  (C, rows, cols) or (rows, cols, C) -- told apart by which
        end holds 1, 3 or 4, torch's channels-first when both do, or by ``layout`` --, or (rows, cols) alpha.  3 channels are RGB with
        alpha 1; 1 channel (``channels`` "alpha" or "luma") gives a 1-channel layer.  ``pre_alpha`` and ``linear_rgb`` say what
        the values ARE; nothing is converted."""
        from . import tensor  # noqa: PLC0415

        return tensor.from_tensor(t, offset, pre_alpha, linear_rgb, channels, layout)

    def __repr__(self):
        return "Layer(x={}, y={}, w={}, h={}, pre_alpha={}, linear_rgb={})".format(
            self.x, self.y, self.width, self.height, self.pre_alpha, self.linear_rgb
        )


def _deflate_parallel(raw: bytes, level: int, threads: int) -> bytes:
    """A zlib stream of ``raw`` built from independently compressed pieces, one per worker thread at a time (the pigz
    construction: every piece but the last is a raw deflate stream ended with a sync flush, so the concatenation is one
    valid deflate stream; zlib header in front, Adler-32 of the whole input behind).  zlib releases the GIL, so the
    pieces really run side by side.  Decodes to the same bytes as the one-shot stream; only the file bytes differ."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    piece = max(1 << 20, -(-len(raw) // (threads * 4)))
    spans = [(o, min(o + piece, len(raw))) for o in range(0, len(raw), piece)] or [(0, 0)]
    view = memoryview(raw)

    def work(k):
        lo, hi = spans[k]
        comp = zlib.compressobj(level, zlib.DEFLATED, -15)
        return comp.compress(view[lo:hi]) + comp.flush(zlib.Z_FINISH if k == len(spans) - 1 else zlib.Z_SYNC_FLUSH)

    with ThreadPoolExecutor(max_workers=threads) as pool:
        parts = list(pool.map(work, range(len(spans))))
    # CMF/FLG: deflate, 32 KiB window; FLEVEL is informative only (2 bits), FCHECK makes the pair a multiple of 31
    cmf, flevel = 0x78, (0 if level < 2 else 1 if level < 6 else 2 if level == 6 else 3) << 6
    flg = flevel + (31 - ((cmf << 8) + flevel) % 31) % 31
    return bytes([cmf, flg]) + b"".join(parts) + (zlib.adler32(raw) & 0xFFFFFFFF).to_bytes(4, "big")


def canvas_to_png(canvas, output=None, level=None, threads=None, *, encoder: str = "host", filter=None, huffman=None, palette=None, dither=None,
                  color=None, depth=None):
    """(height, width, 4) -> PNG (canvas_to_png, S:249-274).  ``canvas`` is either the uint8 array of
    ``Layer.to_rgba8`` or float RGBA in [0, 1] (quantised like the reference: ``np.round(canvas * 255)``).
    ``level`` (default 9) is zlib's; ``threads`` (default 1) > 1 compresses the scanlines in parallel pieces: same pixels, a
    different (slightly larger) file than the reference's, written several times faster (4096 x 4096 at level 9: seconds -> a
    few tenths).

    ``encoder="device"`` (beyond the reference) uploads the bytes and makes the scanline filters and the deflate stream on
    the device: ``filter`` is "adaptive" (default: per row the type libpng's heuristic picks), "none", "sub", "up", "average"
    or "paeth"; ``huffman`` is "dynamic" (default: one code pair made to measure for the whole image) or "fixed".  The file
    decodes to the same pixels and differs from the host encoder's in its bytes.  ``level`` and ``threads`` do not apply to
    it (TypeError); an unknown value is a ValueError before any device work.

    ``palette`` (beyond the reference; None and False: as above) writes an indexed file -- colour type 3 with PLTE, tRNS where an
    entry is not opaque, one IDAT: True allows 256 entries, an int from 2 to 256 that many.  The pixels are uploaded and
    quantised on the device (``quantize``: exact when the image has no more colours than that, a median cut otherwise), the
    index rows are packed there at the smallest depth of 1, 2, 4, 8 that holds the palette, with filter 0.
    ``encoder="host"`` downloads the rows and honours ``level`` and ``threads``; ``encoder="device"`` deflates them on the
    device, honours ``huffman``, and takes no ``filter`` but None or "none" (ValueError).

    ``dither`` (with ``palette`` only; None and "none": every pixel takes its nearest entry) dithers the median cut's image on
    the device: "ordered" with the 8 x 8 Bayer matrix, "diffusion" with Floyd-Steinberg error diffusion (``quantize`` has the
    details).  The palette and the container stay as they are, only the indices change; an image kept exactly is not dithered.
    An unknown word is a ValueError, anything but a string or None a TypeError, a dither without ``palette`` a ValueError.

    ``color`` and ``depth`` (beyond the reference; with neither, everything above) choose the sample format: ``color`` is "rgba"
    (colour type 6, the default), "rgb" (2), "grey-alpha" (4) or "grey" (0) -- "gray" is read too --, ``depth`` 8 (the default) or
    16; one IDAT, no ancillary chunks.  The array is then either the samples themselves -- uint8 or uint16 with as many channels
    as the colour has, (h, w) or (h, w, 1) for grey; uint16 means depth 16, uint8 at depth 16 widens exactly (``v * 257``) -- or
    straight-alpha sRGB RGBA, (h, w, 4) float or uint8 (``v / 255``), from which the samples are made on the device: a sample is
    ``rint(v * M)`` saturated to [0, M] with M = 255 or 65535, NaN giving 0, 16-bit samples most significant byte first; grey is
    the Rec. 709 luma ``(0.2126 * r + 0.7152 * g) + 0.0722 * b`` of the encoded values (grey in, grey out, at every level);
    "rgb" and "grey" ignore alpha, as ``canvas_to_jpeg`` does.  Both encoders take every format: "host" writes filter 0 rows,
    "device" all six ``filter`` words over rows of any pixel size.  An unknown word or depth is a ValueError, a colour that is no
    string a TypeError, a shape that does not go with the colour a ValueError that says what does, either keyword with
    ``palette`` a ValueError; all before any device work."""
    import io
    import zlib

    from . import png  # noqa: PLC0415

    args = png.encoder_arguments(encoder, level, threads, filter, huffman)
    max_colors = png.palette_argument(palette, args[0], filter)
    dither = png.dither_argument(dither, max_colors)
    fmt = png.format_arguments(color, depth, palette)
    if fmt is not None:
        rows, cols, colour_type, depth, samples, source, kind = png.canvas_source(canvas, fmt)
        if samples is None:
            samples = png.samples_device(source, kind, rows, cols, colour_type, depth)
        return png.encode_samples(samples, rows, cols, colour_type, depth, output, args)
    canvas = np.asarray(canvas)
    if canvas.dtype != np.uint8:
        canvas = np.round(canvas * 255.0).astype(np.uint8)
    if canvas.ndim != 3 or canvas.shape[2] != 4:
        raise ValueError("Only RGBA layers are supported")
    height, width, _ = canvas.shape
    if max_colors is not None:
        kw = {"huffman": huffman} if args[0] == "device" else {"level": args[1], "threads": args[2]}
        return png.encode_indexed(canvas, height, width, output, max_colors, encoder=args[0], dither=dither, **kw)
    if args[0] == "device":
        return png.encode_rgba8(canvas, height, width, output, filter, huffman)
    _, level, threads = args

    # filter byte 0 in front of every scanline, then ONE deflate stream (deflate output does not depend on how the
    # input is chunked, so one call gives the bytes of the reference's row-by-row loop)
    rows = np.zeros((height, 1 + width * 4), dtype=np.uint8)
    rows[:, 1:] = canvas.reshape(height, width * 4)
    if threads > 1:
        data = _deflate_parallel(rows.tobytes(), level, threads)
    else:
        comp = zlib.compressobj(level=level)
        data = comp.compress(rows.tobytes()) + comp.flush()
    return png.write_container(io.BytesIO() if output is None else output, width, height, data)


def canvas_to_jpeg(canvas, output=None, **kw) -> bytes:
    """(height, width, 4) -> JPEG bytes, ``canvas_to_png``'s sibling (beyond the reference).  ``canvas`` is the uint8 array
    of ``Layer.to_rgba8`` or float RGBA in [0, 1] (quantised like ``canvas_to_png``); it is uploaded and encoded by
    ``jpeg.write_jpeg``, which takes ``kw``.  Alpha is ignored."""
    from . import jpeg  # noqa: PLC0415

    canvas = np.asarray(canvas)
    if canvas.dtype != np.uint8:
        canvas = np.round(canvas * 255.0).astype(np.uint8)
    if canvas.ndim != 3 or canvas.shape[2] != 4:
        raise ValueError("Only RGBA layers are supported")
    return jpeg.write_jpeg(canvas, output, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# Module-level canvas functions of the reference (S:235-416) for callers that use them directly on numpy arrays.  The
# arithmetic runs in the same device kernels as Layer.compose (k_layer_over / k_layer_in / k_layer_blend); the arrays
# cross PCIe once in each direction per call, so inside a render the Layer methods (which stay in HBM) are the fast way.
# ---------------------------------------------------------------------------------------------------------------------
def canvas_create(width, height, bg=None):
    """(canvas, transform): a float64 (height, width, 4) canvas, transparent or filled with ``bg``, and the transform from
    (x, y) to its pixel coordinates (canvas_create, S:235-246)."""
    from .geometry import Transform  # noqa: PLC0415

    if bg is None:
        canvas = np.zeros((height, width, 4), dtype=FLOAT)
    else:
        canvas = np.array(np.broadcast_to(bg, (height, width, 4)), dtype=FLOAT)
    return canvas, Transform().matrix(0, 1, 0, 1, 0, 0)


def _image3(image, what):
    a = np.asarray(image, dtype=FLOAT)
    if a.ndim == 2:
        a = a[..., None]
    if a.ndim != 3 or a.shape[2] not in (1, 4):
        raise ValueError(f"{what}: expected an image of shape (rows, cols), (rows, cols, 1) or (rows, cols, 4)")
    return np.ascontiguousarray(a)


def _compose_on_device(mode, dst3, src3):
    """blend(dst, src) for two images of equal rows x cols on the device; returns the (rows, cols, 4) result buffer."""
    arithmetic = isinstance(mode, tuple) and len(mode) == 4
    if mode not in COMPOSE_PRE_ALPHA and not arithmetic:
        raise ValueError(f"invalid compose mode: {mode}")
    if dst3.shape[:2] != src3.shape[:2]:
        raise ValueError("canvas_compose: images must have the same rows x cols")
    rows, cols = dst3.shape[:2]
    ctx = _abi.Context.get()
    lib = ctx.lib
    bb = _bbox_arr((0, 0), (rows, cols))
    d_in, s_in = ctx.from_host(dst3), ctx.from_host(src3)
    out = ctx.alloc(max(rows * cols, 1) * 32)
    _abi._check(lib.svgr_layer_crop4(ctx.handle, out.handle, bb, d_in.handle, bb, dst3.shape[2]))  # 1 channel -> 4
    if arithmetic or mode not in (COMPOSE_OVER, COMPOSE_IN):
        k4 = np.array(mode if arithmetic else (0, 0, 0, 0), dtype=FLOAT)
        _abi._check(lib.svgr_layer_blend(ctx.handle, out.handle, bb, s_in.handle, bb, src3.shape[2], 5 if arithmetic else int(mode),
                                         k4.ctypes.data_as(_abi._P)))
    elif mode == COMPOSE_OVER:
        _abi._check(lib.svgr_layer_over(ctx.handle, out.handle, bb, s_in.handle, bb, src3.shape[2], 0))
    else:
        _abi._check(lib.svgr_layer_in(ctx.handle, out.handle, bb, s_in.handle, bb, src3.shape[2]))
    return out


def canvas_compose(mode, dst, src):
    """Compose two alpha-premultiplied images, ``src`` onto ``dst`` (canvas_compose, S:277-298): Porter-Duff OVER / OUT /
    IN / ATOP / XOR or the feComposite ``(k1, k2, k3, k4)`` arithmetic.  Images are (rows, cols[, 1 | 4]) arrays of equal
    rows x cols; a single channel is alpha and broadcasts over RGBA like numpy would."""
    d3, s3 = _image3(dst, "dst"), _image3(src, "src")
    out = _compose_on_device(mode, d3, s3)
    res = out.download(d3.shape[:2] + (4,), FLOAT)
    # numpy's broadcast decides the channels of the reference's result: OUT and IN are `src * f(dst_a)` and keep src's,
    # the other modes add a dst term and take the wider of the two.  An alpha-only result sits in every channel here.
    only_src = mode in (COMPOSE_OUT, COMPOSE_IN)
    if s3.shape[2] == 1 and (only_src or d3.shape[2] == 1):
        res = res[..., 3:]
        if np.ndim(src) == 2 and (only_src or np.ndim(dst) == 2):
            res = res[..., 0]
    return res


from functools import partial as _partial  # noqa: E402

CANVAS_COMPOSE_OVER = _partial(canvas_compose, COMPOSE_OVER)


def _blend_mode(blend):
    """The compose mode of a ``partial(canvas_compose, mode)`` (what the reference passes as ``blend``), else None."""
    if isinstance(blend, _partial) and blend.func is canvas_compose and len(blend.args) == 1 and not blend.keywords:
        return blend.args[0]
    return None


def canvas_merge_at(base, overlay, offset, blend=CANVAS_COMPOSE_OVER):
    """Blend ``overlay`` onto ``base`` at ``offset`` = (row, col), in place, clipping the touched region to [0, 1]
    (canvas_merge_at, S:304-327).  Returns ``base``, or None when nothing overlaps."""
    x, y = int(offset[0]), int(offset[1])
    b_h, b_w = base.shape[:2]
    o_h, o_w = overlay.shape[:2]
    r0, r1 = min(max(x, 0), b_h), min(max(x + o_h, 0), b_h)
    c0, c1 = min(max(y, 0), b_w), min(max(y + o_w, 0), b_w)
    if r1 <= r0 or c1 <= c0:
        return None
    region = base[r0:r1, c0:c1]
    part = overlay[r0 - x:r1 - x, c0 - y:c1 - y]
    mode = _blend_mode(blend)
    if mode is None:  # the caller's own blend function
        region[...] = np.clip(blend(region, part), 0, 1)
        return base
    out = _compose_on_device(mode, _image3(region, "base"), _image3(part, "overlay"))
    ctx = _abi.Context.get()
    n = (r1 - r0) * (c1 - c0) * 4
    _abi._check(ctx.lib.svgr_layer_clip01(ctx.handle, out.handle, n))
    res = out.download((r1 - r0, c1 - c0, 4), FLOAT)
    region[...] = res if region.ndim == 3 and region.shape[2] == 4 else res[..., 3:].reshape(region.shape)
    return base


def _as_layers(layers):
    return [Layer(_image3(image, "layer"), (int(offset[0]), int(offset[1])), True, True) for image, offset in layers]


def canvas_merge_union(layers, full=True, blend=CANVAS_COMPOSE_OVER):
    """Blend ``[(image, (row, col)), ...]`` in order into one image that holds them all; returns (image, offset)
    (canvas_merge_union, S:330-379).  ``full`` picks the reference's formulation (every layer zero-extended to the union
    first); for source-over both give the same pixels."""
    if not layers:
        raise ValueError("can not blend zero layers")
    if len(layers) == 1:
        return layers[0]
    mode = _blend_mode(blend)
    if mode is not None and mode != COMPOSE_IN:  # (Layer.compose takes IN to the intersection; here it stays on the union)
        out = Layer.compose(_as_layers(layers), mode, linear_rgb=True)
        return out.image, (out.x, out.y)
    r0 = min(int(o[0]) for _, o in layers)
    c0 = min(int(o[1]) for _, o in layers)
    r1 = max(int(o[0]) + im.shape[0] for im, o in layers)
    c1 = max(int(o[1]) + im.shape[1] for im, o in layers)
    output = None
    for image, (x, y) in layers:
        ext = np.zeros((r1 - r0, c1 - c0, 4), dtype=FLOAT)
        ext[x - r0:x - r0 + image.shape[0], y - c0:y - c0 + image.shape[1]] = image
        output = ext if output is None else blend(output, ext)
    return output, (r0, c0)


def canvas_merge_intersect(layers, blend=CANVAS_COMPOSE_OVER):
    """Blend ``[(image, (row, col)), ...]`` on the region covered by all of them; (image, offset) or None when that region
    is empty (canvas_merge_intersect, S:382-416)."""
    if not layers:
        raise ValueError("can not blend zero layers")
    if len(layers) == 1:
        return layers[0]
    r0 = max(int(o[0]) for _, o in layers)
    c0 = max(int(o[1]) for _, o in layers)
    r1 = min(int(o[0]) + im.shape[0] for im, o in layers)
    c1 = min(int(o[1]) + im.shape[1] for im, o in layers)
    if r0 >= r1 or c0 >= c1:
        return None
    crop = lambda im, o: im[r0 - int(o[0]):r1 - int(o[0]), c0 - int(o[1]):c1 - int(o[1])]  # noqa: E731
    mode = _blend_mode(blend)
    (first, f_off), *rest = layers
    output = _image3(crop(first, f_off), "layer")
    if output.shape[2] == 1:
        output = np.ascontiguousarray(np.broadcast_to(output, output.shape[:2] + (4,)))
    for image, off in rest:
        part = crop(image, off)
        output = blend(output, part) if mode is None else canvas_compose(mode, output, part)
    return output, (r0, c0)
