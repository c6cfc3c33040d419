"""Tensor output: a layer packed on the device into the element type and layout a framework wants (beyond the reference).

``Layer.image`` leaves the device as (rows, cols, 4) float64, 32 bytes per pixel.  ``Layer.to_array`` and ``Layer.to_tensor``
run one kernel (svgr_layer_to_tensor, csrc/svgr_tensor.h) that selects the channels, applies an optional background and a
per-channel ``(v - mean) / std``, rounds to float32 / float16 / bfloat16 / uint8 and writes planar CHW or interleaved HWC --
``to_array`` into a buffer of the library's, of which only the packed bytes are downloaded; ``to_tensor`` straight into a
``torch.Tensor`` on the device, which may be a slice of a batch or a window of a larger picture.  ``Layer.from_tensor`` is the
way back.  DESIGN.md 7p has the arithmetic.

Import order.  torch brings its own HIP runtime.  The two libraries share one runtime -- and with it streams, events and
pointers -- only when torch was imported, and had touched CUDA, BEFORE the first call into this package; the other way round
torch finds no device.  The torch entry points import torch lazily and say so when the order was wrong; ``to_array`` needs no
torch at all.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _abi
from .geometry import Transform
from .layer import Layer, _bbox_arr

LAYOUTS = ("chw", "hwc")
CHANNELS = {"rgba": _abi.TENSOR_RGBA, "rgb": _abi.TENSOR_RGB, "alpha": _abi.TENSOR_ALPHA, "luma": _abi.TENSOR_LUMA}
N_CHANNELS = {"rgba": 4, "rgb": 3, "alpha": 1, "luma": 1}
ALPHAS = ("premultiplied", "straight")
_NUMPY_DTYPES = {np.dtype(np.float32): _abi.TENSOR_F32, np.dtype(np.float16): _abi.TENSOR_F16, np.dtype(np.uint8): _abi.TENSOR_U8}
_ELEM_BYTES = {_abi.TENSOR_F32: 4, _abi.TENSOR_F16: 2, _abi.TENSOR_BF16: 2, _abi.TENSOR_U8: 1}
IMPORT_ORDER = ("torch finds no device in a process whose HIP runtime svgrasterize_amd has initialised first: import torch and "
                "touch CUDA (torch.cuda.init()) before the first svgrasterize_amd call")


class _Options(NamedTuple):
    layout: str
    channels: str
    premultiplied: bool
    linear_rgb: bool
    bg: tuple | None
    scale: tuple
    bias: tuple


def _options(layout, channels, alpha, linear_rgb, bg, mean, std) -> _Options:
    """The keywords of to_array / to_tensor, checked (before any device work) and brought into the kernel's terms."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout is one of {', '.join(LAYOUTS)}, not {layout!r}")
    if channels not in CHANNELS:
        raise ValueError(f"channels is one of {', '.join(CHANNELS)}, not {channels!r}")
    if alpha not in ALPHAS:
        raise ValueError(f"alpha is one of {', '.join(ALPHAS)}, not {alpha!r}")
    n = N_CHANNELS[channels]
    if bg is not None:
        if alpha != "premultiplied":
            raise ValueError("bg needs premultiplied input (alpha='premultiplied')")
        bg = tuple(float(v) for v in np.asarray(bg, dtype=np.float64).reshape(-1)[:4])
        if len(bg) not in (3, 4) or not np.isfinite(bg).all():
            raise ValueError("bg is three finite colour values (premultiplied, in the output's colour space)")
        bg = bg[:3]

    def per_channel(v, what, default):
        if v is None:
            return np.full(n, default, dtype=np.float64)
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        if v.size == 1:
            v = np.repeat(v, n)
        if v.size != n or not np.isfinite(v).all():
            raise ValueError(f"{what} is one finite value or one per output channel ({n} for channels={channels!r})")
        return v

    mean, std = per_channel(mean, "mean", 0.0), per_channel(std, "std", 1.0)
    if (std == 0.0).any():
        raise ValueError("std must not be zero")
    scale, bias = 1.0 / std, -mean / std
    if not (np.isfinite(scale).all() and np.isfinite(bias).all()):
        raise ValueError("1 / std and mean / std must be finite")
    pad = (1.0,) * (4 - n), (0.0,) * (4 - n)
    return _Options(layout, channels, alpha == "premultiplied", bool(linear_rgb), bg, tuple(scale) + pad[0], tuple(bias) + pad[1])


def _size(layer: Layer, size):
    if size is None:
        return layer.height, layer.width
    rows, cols = (int(v) for v in size)
    if rows < 0 or cols < 0:
        raise ValueError("size is (rows, cols), neither negative")
    return rows, cols


def _desc(dtype, channels, rows, cols, strides, offset=0, source=_abi.TENSOR_SRC_RGBA_F64, bg=None, scale=None, bias=None):
    d = _abi.TensorDesc()
    d.source, d.dtype, d.channels, d.has_bg = source, dtype, CHANNELS[channels], int(bg is not None)
    d.bg = (C.c_double * 3)(*(bg or (0.0, 0.0, 0.0)))
    d.scale = (C.c_double * 4)(*(scale or (1.0,) * 4))
    d.bias = (C.c_double * 4)(*(bias or (0.0,) * 4))
    d.rows, d.cols = rows, cols
    d.stride_c, d.stride_h, d.stride_w = strides
    d.offset = offset
    return d


def _dense_strides(layout, n, rows, cols):
    return (rows * cols, cols, 1) if layout == "chw" else (1, cols * n, n)


def _pack(ctx, layer: Layer, opt: _Options, dtype, rows, cols, placed: bool, dst, strides, offset=0):
    """svgr_layer_to_tensor of `layer`, converted as `opt` says, into the device buffer `dst`; `placed`: at its offset on the
    plane (Layer.on_canvas's rule), otherwise the plane is the layer's own extent."""
    layer = layer.convert(pre_alpha=opt.premultiplied, linear_rgb=opt.linear_rgb)
    src = layer._device()   # (an upload or a noted conversion run now: a temporary that outlives the call)
    source = _abi.TENSOR_SRC_MASK_F64 if layer.channels == 1 else _abi.TENSOR_SRC_RGBA_F64
    d = _desc(dtype, opt.channels, rows, cols, strides, offset, source, opt.bg, opt.scale, opt.bias)
    bbox = _bbox_arr(layer.offset if placed else (0, 0), layer._shape)
    _abi._check(ctx.lib.svgr_layer_to_tensor(ctx.handle, C.byref(d), src.handle, bbox, dst.handle))


def to_array(layer: Layer, size=None, *, dtype=np.float32, layout="chw", channels="rgba", alpha="premultiplied", linear_rgb=False,
             bg=None, mean=None, std=None) -> np.ndarray:
    """``Layer.to_array``."""
    opt = _options(layout, channels, alpha, linear_rgb, bg, mean, std)
    try:
        code = _NUMPY_DTYPES[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError(f"to_array: dtype is float32, float16 or uint8, not {dtype!r} (numpy has no bfloat16: Layer.to_tensor has)") from None
    rows, cols = _size(layer, size)
    n = N_CHANNELS[channels]
    shape = (n, rows, cols) if layout == "chw" else (rows, cols, n)
    if rows == 0 or cols == 0:
        return np.zeros(shape, dtype=dtype)
    ctx = _abi.Context.get()
    buf = ctx.alloc(rows * cols * n * _ELEM_BYTES[code])
    _pack(ctx, layer, opt, code, rows, cols, size is not None, buf, _dense_strides(layout, n, rows, cols))
    return buf.download(shape, np.dtype(dtype))


# ------------------------------------------------------------------------------------------------------------------------------
# torch
# ------------------------------------------------------------------------------------------------------------------------------
def _torch():
    """torch, imported when a torch entry point is first used, and the import-order rule checked."""
    import torch  # noqa: PLC0415

    if _abi.Context._by_device and not torch.cuda.is_available():
        raise RuntimeError(IMPORT_ORDER)
    return torch


def _torch_dtypes(torch):
    return {torch.float32: _abi.TENSOR_F32, torch.float16: _abi.TENSOR_F16, torch.bfloat16: _abi.TENSOR_BF16, torch.uint8: _abi.TENSOR_U8}


def _context(torch):
    if not torch.cuda.is_available():
        raise RuntimeError("torch reports no device")
    torch.cuda.init()
    return _abi.Context.get()


def _strides3(t, layout, rows, cols, n):
    """(stride_c, stride_h, stride_w) of a 3-D tensor.  A dimension of size 1 has no stride worth the name (torch reports whatever
    the view was made with): it gets the dense one."""
    s = [int(v) for v in t.stride()]
    sc, sh, sw = (s[0], s[1], s[2]) if layout == "chw" else (s[2], s[0], s[1])
    interleaved = sw != 1 or (cols == 1 and layout == "hwc" and n > 1)
    if cols == 1:
        sw = n if interleaved else 1
    if rows == 1:
        sh = cols * (n if interleaved else 1)
    if n == 1:
        sc = 1 if interleaved else rows * sh
    return sc, sh, sw


def _wrap(ctx, torch, t):
    """The tensor's memory as a non-owning buffer: from its first element to the end of its storage."""
    nbytes = t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()
    return ctx.wrap(t.data_ptr(), nbytes)


class _Ordered:
    """The context's stream behind torch's current one on entry, torch's behind the context's on exit: no host wait."""

    def __init__(self, ctx, torch):
        self.ctx, self.stream = ctx, _abi._P(torch.cuda.current_stream(ctx.device).cuda_stream)

    def __enter__(self):
        _abi._check(self.ctx.lib.svgr_stream_wait_for(self.ctx.handle, self.stream))

    def __exit__(self, *exc):
        _abi._check(self.ctx.lib.svgr_stream_signal_to(self.ctx.handle, self.stream))
        return False


def to_tensor(layer: Layer, out=None, size=None, *, dtype=None, layout="chw", channels="rgba", alpha="premultiplied", linear_rgb=False,
              bg=None, mean=None, std=None):
    """``Layer.to_tensor``."""
    opt = _options(layout, channels, alpha, linear_rgb, bg, mean, std)
    rows, cols = _size(layer, size)
    torch = _torch()
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError(f"out is a torch.Tensor, not {type(out).__name__}")
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    code = _torch_dtypes(torch).get(dtype)
    if code is None:
        raise TypeError(f"to_tensor: dtype is torch.float32, float16, bfloat16 or uint8, not {dtype!r}")
    n = N_CHANNELS[channels]
    shape = (n, rows, cols) if layout == "chw" else (rows, cols, n)
    if out is not None:
        if out.dtype != dtype:
            raise TypeError(f"out is {out.dtype}, the call asks for {dtype}")
        if tuple(out.shape) != shape:
            raise ValueError(f"out has shape {tuple(out.shape)}, the call writes {shape} (layout {layout!r})")
        if not out.is_cuda:
            raise ValueError("out must be on the device")
    ctx = _context(torch)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=torch.device("cuda", ctx.device))
    elif out.device.index != ctx.device:
        raise ValueError(f"out is on {out.device}, the library's context on device {ctx.device}")
    if rows == 0 or cols == 0:
        return out
    strides = _strides3(out, layout, rows, cols, n)
    with _Ordered(ctx, torch):
        _pack(ctx, layer, opt, code, rows, cols, size is not None, _wrap(ctx, torch, out), strides)
    return out


def _tensor_layout(shape, layout):
    if layout is not None:
        if layout not in LAYOUTS:
            raise ValueError(f"layout is one of {', '.join(LAYOUTS)}, not {layout!r}")
        return layout
    if shape[0] in (1, 3, 4):   # (torch's own convention first)
        return "chw"
    if shape[2] in (1, 3, 4):
        return "hwc"
    raise ValueError(f"a tensor of shape {tuple(shape)} is neither (C, rows, cols) nor (rows, cols, C) with C of 1, 3 or 4")


def from_tensor(t, offset=(0, 0), pre_alpha=True, linear_rgb=False, channels=None, layout=None) -> Layer:
    """``Layer.from_tensor``."""
    is_numpy = isinstance(t, np.ndarray)
    if is_numpy:
        torch = None
        if t.dtype not in _NUMPY_DTYPES:
            raise TypeError(f"from_tensor: dtype is float32, float16 or uint8, not {t.dtype}")
        code = _NUMPY_DTYPES[t.dtype]
        t = np.ascontiguousarray(t)
    else:
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"from_tensor takes a torch.Tensor or a numpy array, not {type(t).__name__}")
        code = _torch_dtypes(torch).get(t.dtype)
        if code is None:
            raise TypeError(f"from_tensor: dtype is torch.float32, float16, bfloat16 or uint8, not {t.dtype}")
        if not t.is_cuda:
            raise ValueError("the tensor must be on the device")
    if t.ndim == 2:
        t = t[None] if layout in (None, "chw") else t[:, :, None]
        layout = layout or "chw"
    if t.ndim != 3:
        raise ValueError("from_tensor takes a (C, rows, cols) or (rows, cols, C) tensor, or (rows, cols) alpha")
    layout = _tensor_layout(t.shape, layout)
    n, rows, cols = (t.shape[0], t.shape[1], t.shape[2]) if layout == "chw" else (t.shape[2], t.shape[0], t.shape[1])
    n, rows, cols = int(n), int(rows), int(cols)
    if channels is None:
        channels = {4: "rgba", 3: "rgb", 1: "alpha"}.get(n)
    if channels not in CHANNELS or N_CHANNELS[channels] != n:
        raise ValueError(f"channels={channels!r} does not go with {n} channels")
    out_ch = 4 if channels in ("rgba", "rgb") else 1
    if rows == 0 or cols == 0:
        return Layer(np.zeros((rows, cols, out_ch)), offset, pre_alpha, linear_rgb)
    if is_numpy:
        ctx = _abi.Context.get()
        src = ctx.from_host(t)
        strides = _dense_strides(layout, n, rows, cols)
    else:
        ctx = _context(torch)
        if t.device.index != ctx.device:
            raise ValueError(f"the tensor is on {t.device}, the library's context on device {ctx.device}")
        src = _wrap(ctx, torch, t)
        strides = _strides3(t, layout, rows, cols, n)
    d = _desc(code, channels, rows, cols, strides)
    dst = ctx.alloc(rows * cols * out_ch * 8)
    if is_numpy:
        _abi._check(ctx.lib.svgr_tensor_to_layer(ctx.handle, C.byref(d), src.handle, dst.handle))
    else:
        with _Ordered(ctx, torch):
            _abi._check(ctx.lib.svgr_tensor_to_layer(ctx.handle, C.byref(d), src.handle, dst.handle))
    return Layer._from_device(dst, (rows, cols, out_ch), offset, pre_alpha, linear_rgb)


def render_to_tensor(scene, transform, viewport, out=None, **kw):
    """`scene` rendered under `transform` over `viewport` (row0, col0, rows, cols) and packed by ``Layer.to_tensor`` onto the
    viewport's plane; ``kw`` are its keywords (``linear_rgb`` is also the render's).  An empty render gives the background."""
    row0, col0, rows, cols = (int(v) for v in viewport)
    linear_rgb = bool(kw.get("linear_rgb", False))
    _options(kw.get("layout", "chw"), kw.get("channels", "rgba"), kw.get("alpha", "premultiplied"), linear_rgb, kw.get("bg"),
             kw.get("mean"), kw.get("std"))   # (refused before the render)
    result = scene.render(transform if transform is not None else Transform(), viewport=[row0, col0, rows, cols], linear_rgb=linear_rgb)
    layer = Layer.transparent((row0, col0), True, linear_rgb) if result is None else result[0]
    return to_tensor(layer.translate(-row0, -col0), out, (rows, cols), **kw)


def fit_transform(doc_size, size) -> Transform:
    """A document of `doc_size` (width, height) scaled uniformly into `size` (rows, cols) and centred: xMidYMid meet."""
    w, h = float(doc_size[0]), float(doc_size[1])
    rows, cols = size
    s = min(cols / w, rows / h) if w > 0 and h > 0 else 1.0
    return Transform().translate((cols - s * w) / 2.0, (rows - s * h) / 2.0).scale(s)


def _svg_layer(document, size, fonts, css, linear_rgb):
    """The layer of one document fitted to `size` (None: nothing to draw)."""
    import io  # noqa: PLC0415
    import os  # noqa: PLC0415

    from . import svg  # noqa: PLC0415

    if isinstance(document, (str, os.PathLike)) and not str(document).lstrip().startswith("<"):
        scene, _ids, doc_size = svg.svg_scene_from_filepath(os.fspath(document), fonts=fonts, css=css)
    elif isinstance(document, (str, bytes)):
        text = document.decode("utf-8") if isinstance(document, bytes) else document
        scene, _ids, doc_size = svg.svg_scene(io.StringIO(text), fonts=fonts, css=css)
    else:
        scene, _ids, doc_size = svg.svg_scene(document, fonts=fonts, css=css)
    if scene is None:
        return None
    rows, cols = size
    view = Transform().matrix(0, 1, 0, 1, 0, 0)   # (render_svg's swap into presentation space)
    if doc_size is not None:
        view = view @ fit_transform(doc_size, size)
    result = scene.render(view, viewport=[0, 0, rows, cols], linear_rgb=linear_rgb)
    return None if result is None else result[0]


def render_svgs_to_tensor(documents, size, out=None, fonts=None, css=None, **kw):
    """``documents`` (paths, file objects or SVG text) rendered into one batch tensor, (N, C, rows, cols) or (N, rows, cols, C):
    each scaled uniformly to fit ``size`` = (rows, cols) and centred (xMidYMid meet), the rest of its plane transparent, or
    ``bg``; the kernel writes document n straight into ``out[n]``.  ``kw`` are ``Layer.to_tensor``'s keywords."""
    documents = list(documents)
    rows, cols = (int(v) for v in size)
    layout, channels = kw.get("layout", "chw"), kw.get("channels", "rgba")
    linear_rgb = bool(kw.get("linear_rgb", False))
    _options(layout, channels, kw.get("alpha", "premultiplied"), linear_rgb, kw.get("bg"), kw.get("mean"), kw.get("std"))
    torch = _torch()
    n = N_CHANNELS[channels]
    shape = (len(documents), n, rows, cols) if layout == "chw" else (len(documents), rows, cols, n)
    if out is None:
        ctx = _context(torch)
        out = torch.empty(shape, dtype=kw.get("dtype") or torch.float32, device=torch.device("cuda", ctx.device))
    elif not isinstance(out, torch.Tensor):
        raise TypeError(f"out is a torch.Tensor, not {type(out).__name__}")
    elif tuple(out.shape) != shape:
        raise ValueError(f"out has shape {tuple(out.shape)}, the call writes {shape} (layout {layout!r})")
    for k, document in enumerate(documents):
        layer = _svg_layer(document, (rows, cols), fonts, css, linear_rgb)
        if layer is None:
            layer = Layer.transparent((0, 0), True, linear_rgb)
        to_tensor(layer, out[k], (rows, cols), **kw)
    return out
