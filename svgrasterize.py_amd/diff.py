"""Differentiable coverage: a path's exact area coverage over a viewport and its derivative with respect to the control points and
the transform (beyond the reference).

``coverage`` gives, for every path of a packed set, the plane ``Path.mask`` would give placed on the viewport, and the int8 plane
of the fill rule's derivative; ``coverage_backward`` takes that plane and ``d loss / d cover`` to ``d loss / d segs`` and
``d loss / d m6``.  ``coverage_tensor`` is both as a ``torch.autograd.Function`` whose geometry stays on the device.  The kernels
are svgr_cover_forward / svgr_cover_backward (csrc/svgr_cover.h has the arithmetic, DESIGN.md 7w the derivation).

What the derivative is.  Exact for the area coverage of the FLATTENED outline at fixed subdivision: a move that changes how a
cubic is subdivided is not followed across that change.  It is the derivative of ``sum(grad_out * cover)`` under any motion that
keeps every outline closed: the copies of a point that neighbouring segments share must move together (sum their entries;
torch's indexing does).  Where a pixel's accumulated coverage sits on a kink of its fill rule -- the 1e-6 cut, |A| = 1 under
nonzero, an integer under even-odd -- the derivative is not defined and the slope takes one side.

Differentiable compositing: ``compose`` paints the planes as solid fills source-over in paint order, with the renderer's
arithmetic; ``compose_backward`` gives ``d loss / d cover`` and ``d loss / d paints``.  ``compose_tensor`` is both as a
``torch.autograd.Function`` and ``render_tensor`` chains it behind ``coverage_tensor``: geometry and colours to an RGBA image and
back.  The kernels are svgr_compose_forward / svgr_compose_backward (csrc/svgr_compose.h).

Gradient paints: ``compose_painted`` / ``compose_painted_backward`` are ``compose`` and its backward with every path a solid fill or
the renderer's linear or one-circle radial gradient (``GradientPaints``, built by ``gradient_paints``), with derivatives to the
gradients' transforms, end points, centre and radius, stop positions and stop colours.  ``compose_painted_tensor`` and
``render_painted_tensor`` are the torch forms.  The kernels are svgr_compose_painted_forward / svgr_compose_painted_backward
(csrc/svgr_gradpaint.h).

Groups: ``compose_grouped`` / ``compose_grouped_backward`` are ``compose_painted`` and its backward driven by a program with
isolated groups (``Group``, ``group_program``, ``Groups``): a group has an opacity, a clip of its own coverage planes, both or
neither, and the backward also reaches the opacities and the clip planes.  ``compose_grouped_tensor`` and ``render_grouped_tensor``
are the torch forms; ``lower_scene`` makes all the arrays from a ``Scene``.  The kernels are svgr_compose_grouped_forward /
svgr_compose_grouped_backward (csrc/svgr_group.h).
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

from . import _abi
from .tensor import _context, _Ordered, _torch, _wrap

FLATNESS = 0.1
_PLANES = {np.dtype(np.float64): _abi.COVER_F64, np.dtype(np.float32): _abi.COVER_F32}
_MAX_PIXELS = 2 ** 31 - 1


def cover_block() -> int:
    """Segments per workgroup of the segment kernels (their launch seam)."""
    return int(_abi.load_library().svgr_cover_block())


def cover_scan() -> int:
    """Columns one step of the row scan covers (its seam)."""
    return int(_abi.load_library().svgr_cover_scan())


def _viewport(viewport):
    try:
        vp = tuple(int(v) for v in viewport)
    except (TypeError, ValueError):
        raise ValueError("viewport is (row0, col0, rows, cols)") from None
    if len(vp) != 4 or vp[2] <= 0 or vp[3] <= 0 or max(abs(vp[0]), abs(vp[1])) > 2 ** 30:
        raise ValueError("viewport is (row0, col0, rows, cols) with rows > 0 and cols > 0")
    return vp


def _flatness(flatness):
    flatness = float(flatness)
    if not (flatness > 0.0 and np.isfinite(flatness)):
        raise ValueError("flatness must be positive and finite")
    return flatness


def _topology(kinds, path_seg_off, rules, n_segs, n_paths):
    """kinds, offsets and rules on the host, checked: (uint8 (n_segs,), int32 (n_paths + 1,), uint8 (n_paths,))."""
    kinds = np.ascontiguousarray(kinds).reshape(-1)
    off = np.ascontiguousarray(path_seg_off).reshape(-1)
    rules = np.ascontiguousarray(rules).reshape(-1)
    if len(kinds) != n_segs or not np.isin(kinds, (_abi.SEG_LINE, _abi.SEG_CUBIC)).all():
        raise ValueError(f"kinds holds one of SEG_LINE / SEG_CUBIC per segment ({n_segs})")
    if len(off) != n_paths + 1 or n_paths < 1 or off.dtype.kind not in "iu" or off[0] != 0 or off[-1] != n_segs or (np.diff(off.astype(np.int64)) < 0).any():
        raise ValueError("path_seg_off is n_paths + 1 ascending integers from 0 to the number of segments, one entry per row of m6 and one more")
    if len(rules) != n_paths or not np.isin(rules, (0, 1)).all():
        raise ValueError(f"rules holds 0 (nonzero) or 1 (even-odd) per path ({n_paths})")
    return kinds.astype(np.uint8), off.astype(np.int32), rules.astype(np.uint8)


def _geometry(segs, m6):
    segs = np.ascontiguousarray(segs, dtype=np.float64)
    if segs.ndim < 2 or segs.size != segs.shape[0] * 8:
        raise ValueError("segs is (n_segs, 4, 2) or (n_segs, 8): packed() segments")
    m6 = np.ascontiguousarray(m6, dtype=np.float64)
    m6 = m6.reshape(1, 6) if m6.shape == (6,) else m6
    if m6.ndim != 2 or m6.shape[1] != 6:
        raise ValueError("m6 is (n_paths, 6)")
    return segs.reshape(-1, 4, 2), m6


def _refuse_non_finite(segs, kinds, m6):
    used = np.zeros((len(segs), 4), dtype=bool)
    used[:, :2] = True
    used[kinds != _abi.SEG_LINE] = True
    if not np.isfinite(segs[used]).all() or not np.isfinite(m6).all():
        raise ValueError("the control points and the transforms must be finite")


def _n_pixels(n_paths, vp):
    n = n_paths * vp[2] * vp[3]
    if n > _MAX_PIXELS:
        raise _abi.SvgrError(f"{n_paths} planes of {vp[2]} x {vp[3]} pixels are beyond 2^31 - 1 pixels")
    return n


def _desc(n_segs, n_paths, vp, plane, flatness):
    d = _abi.CoverDesc()
    d.n_segs, d.n_paths, d.flatness, d.plane, d.reserved = n_segs, n_paths, flatness, plane, 0
    d.viewport = (C.c_int64 * 4)(*vp)
    return d


def _raise_on_status(word: int):
    if word & _abi.COVER_STATUS_RANGE:
        raise _abi.SvgrError("coverage: a transformed control point is not finite or beyond +-1e9 pixels")
    if word & _abi.COVER_STATUS_DEPTH:
        raise _abi.SvgrError("coverage: the flatten depth cap was hit")


def _h(buf):
    return None if buf is None else buf.handle


def _host_inputs(segs, kinds, path_seg_off, m6, rules, viewport, flatness):
    segs, m6 = _geometry(segs, m6)
    kinds, off, rules = _topology(kinds, path_seg_off, rules, len(segs), len(m6))
    _refuse_non_finite(segs, kinds, m6)
    return segs, kinds, off, m6, rules, _viewport(viewport), _flatness(flatness)


def _upload(ctx, segs, kinds, off, m6):
    some = len(segs) > 0
    return (ctx.from_host(segs) if some else None, ctx.from_host(kinds) if some else None, ctx.from_host(off), ctx.from_host(m6))


def coverage(segs, kinds, path_seg_off, m6, rules, viewport, dtype=np.float64, flatness: float = FLATNESS):
    """``(cover, slope)`` of ``n_paths`` paths over ``viewport = (row0, col0, rows, cols)``.

    ``segs`` / ``kinds`` are ``Path.packed()`` segments in user space, path ``p`` owning ``path_seg_off[p] : path_seg_off[p + 1]``;
    ``m6`` is ``(n_paths, 6)`` and ``rules`` 0 (nonzero) or 1 (even-odd) per path.  ``cover`` is ``(n_paths, rows, cols)`` of
    ``dtype`` (float64 or float32): plane ``p`` is ``Path.mask`` of path ``p`` placed on the viewport.  ``slope`` is the int8
    plane ``coverage_backward`` needs.  Wrong shapes, rules and non-finite geometry are refused before any device work."""
    plane = _PLANES.get(_np_dtype(dtype))
    if plane is None:
        raise TypeError(f"a coverage plane is float64 or float32, not {dtype!r}")
    segs, kinds, off, m6, rules, vp, flatness = _host_inputs(segs, kinds, path_seg_off, m6, rules, viewport, flatness)
    n_paths, shape = len(m6), (len(m6), vp[2], vp[3])
    n_px = _n_pixels(n_paths, vp)
    ctx = _abi.Context.get()
    d_segs, d_kinds, d_off, d_m6 = _upload(ctx, segs, kinds, off, m6)
    d_rules = ctx.from_host(rules)
    cover, slope, status = ctx.alloc(n_px * (8 if plane == _abi.COVER_F64 else 4)), ctx.alloc(n_px), ctx.alloc(4)
    status.zero()
    desc = _desc(len(segs), n_paths, vp, plane, flatness)
    _abi._check(ctx.lib.svgr_cover_forward(ctx.handle, C.byref(desc), _h(d_segs), _h(d_kinds), d_off.handle, d_m6.handle, d_rules.handle,
                                           cover.handle, slope.handle, status.handle))
    _raise_on_status(int(status.download((1,), np.uint32)[0]))
    return cover.download(shape, _np_dtype(dtype)), slope.download(shape, np.int8)


def coverage_backward(segs, kinds, path_seg_off, m6, rules, viewport, slope, grad_out, flatness: float = FLATNESS):
    """``(grad_segs, grad_m6)``: the derivative of ``sum(grad_out * cover)`` from the ``slope`` plane ``coverage`` returned.

    ``grad_out`` has ``cover``'s shape and is float64 or float32.  ``grad_segs`` is ``(n_segs, 4, 2)`` in user space and
    ``packed()`` order (a line's last two points stay 0), ``grad_m6`` ``(n_paths, 6)``.  No atomics: the same bits on every run.
    (``rules`` is checked like ``coverage``'s; the kept ``slope`` is what the pass uses.)"""
    segs, kinds, off, m6, rules, vp, flatness = _host_inputs(segs, kinds, path_seg_off, m6, rules, viewport, flatness)
    n_paths, shape = len(m6), (len(m6), vp[2], vp[3])
    slope, grad_out = np.asarray(slope), np.asarray(grad_out)
    if slope.dtype != np.int8:
        raise TypeError(f"slope is the int8 plane coverage returned, not {slope.dtype}")
    plane = _PLANES.get(grad_out.dtype)
    if plane is None:
        raise TypeError(f"grad_out is float64 or float32, not {grad_out.dtype}")
    if slope.shape != shape or grad_out.shape != shape:
        raise ValueError(f"slope and grad_out are {shape}, not {slope.shape} and {grad_out.shape}")
    _n_pixels(n_paths, vp)
    ctx = _abi.Context.get()
    d_segs, d_kinds, d_off, d_m6 = _upload(ctx, segs, kinds, off, m6)
    d_slope, d_grad = ctx.from_host(slope), ctx.from_host(grad_out)
    g_segs = ctx.alloc(len(segs) * 64) if len(segs) else None
    g_m6, status = ctx.alloc(n_paths * 48), ctx.alloc(4)
    status.zero()
    desc = _desc(len(segs), n_paths, vp, plane, flatness)
    _abi._check(ctx.lib.svgr_cover_backward(ctx.handle, C.byref(desc), _h(d_segs), _h(d_kinds), d_off.handle, d_m6.handle, d_slope.handle,
                                            d_grad.handle, _h(g_segs), g_m6.handle, status.handle))
    _raise_on_status(int(status.download((1,), np.uint32)[0]))
    grad_segs = g_segs.download((len(segs), 4, 2), np.float64) if len(segs) else np.zeros((0, 4, 2))
    return grad_segs, g_m6.download((n_paths, 6), np.float64)


def _np_dtype(dtype):
    try:
        return np.dtype(dtype)
    except TypeError:
        return None


# ------------------------------------------------------------------------------------------------------------------------------
# single paths (Path.coverage / Path.coverage_vjp)
# ------------------------------------------------------------------------------------------------------------------------------
def _path_args(path, transform, fill_rule):
    from .geometry import _RULES, Transform  # noqa: PLC0415

    if fill_rule not in _RULES:
        raise ValueError(f"Invalid fill rule: {fill_rule}")
    segs, kinds = path.packed()
    m6 = (transform if transform is not None else Transform()).m6()
    return segs, kinds, [0, len(segs)], [m6], [_RULES[fill_rule]]


def path_coverage(path, transform, viewport, fill_rule=None, dtype=np.float64):
    """``Path.coverage``."""
    cover, slope = coverage(*_path_args(path, transform, fill_rule), viewport, dtype=dtype)
    return cover[0], slope[0]


def path_coverage_vjp(path, transform, viewport, grad_out, fill_rule=None):
    """``Path.coverage_vjp``."""
    args = _path_args(path, transform, fill_rule)
    grad_out = np.asarray(grad_out)
    if grad_out.dtype not in _PLANES:
        grad_out = grad_out.astype(np.float64)
    _cover, slope = coverage(*args, viewport, dtype=grad_out.dtype)
    grad_segs, grad_m6 = coverage_backward(*args, viewport, slope, grad_out.reshape(slope.shape))
    return grad_segs, grad_m6[0]


# ------------------------------------------------------------------------------------------------------------------------------
# torch
# ------------------------------------------------------------------------------------------------------------------------------
def _buffers(ctx, torch, *tensors):
    return [None if t is None or t.numel() == 0 else _wrap(ctx, torch, t) for t in tensors]


@functools.lru_cache(maxsize=None)
def _function(torch):
    class Coverage(torch.autograd.Function):
        """cover = Coverage.apply(segs, m6, out, kinds, off, rules, viewport, plane, flatness, check)."""

        @staticmethod
        def forward(fn, segs, m6, out, kinds, off, rules, vp, plane, flatness, check):
            ctx = _context(torch)
            n_segs, n_paths = int(segs.shape[0]), int(m6.shape[0])
            dev = segs.device
            cover = out if out is not None else torch.empty((n_paths, vp[2], vp[3]), dtype=torch.float64 if plane == _abi.COVER_F64 else torch.float32, device=dev)
            slope = torch.empty((n_paths, vp[2], vp[3]), dtype=torch.int8, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            segs_c, m6_c = segs.detach().contiguous(), m6.detach().contiguous()
            desc = _desc(n_segs, n_paths, vp, plane, flatness)
            with _Ordered(ctx, torch):
                b = _buffers(ctx, torch, segs_c, kinds, off, m6_c, rules, cover, slope, status)
                _abi._check(ctx.lib.svgr_cover_forward(ctx.handle, C.byref(desc), *[_h(x) for x in b]))
            if check:
                _raise_on_status(int(status.item()) & 0xffffffff)
            fn.save_for_backward(segs_c, m6_c, slope, kinds, off)
            fn.cover_args = (vp, plane, flatness, check)
            if out is not None:
                fn.mark_dirty(out)
            return cover

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(fn, grad):
            segs_c, m6_c, slope, kinds, off = fn.saved_tensors
            vp, plane, flatness, check = fn.cover_args
            ctx = _context(torch)
            grad = grad.contiguous()
            grad_segs, grad_m6 = torch.zeros_like(segs_c), torch.empty_like(m6_c)
            status = torch.zeros(1, dtype=torch.int32, device=grad.device)
            desc = _desc(int(segs_c.shape[0]), int(m6_c.shape[0]), vp, plane, flatness)
            with _Ordered(ctx, torch):
                b = _buffers(ctx, torch, segs_c, kinds, off, m6_c, slope, grad, grad_segs, grad_m6, status)
                _abi._check(ctx.lib.svgr_cover_backward(ctx.handle, C.byref(desc), *[_h(x) for x in b]))
            if check:
                _raise_on_status(int(status.item()) & 0xffffffff)
            return (grad_segs, grad_m6) + (None,) * 8

    return Coverage


def coverage_tensor(segs, m6, *, kinds, path_seg_off, rules, viewport, dtype=None, out=None, check: bool = False, flatness: float = FLATNESS):
    """``coverage`` as a ``torch.autograd.Function``: an ``(n_paths, rows, cols)`` tensor the kernels write in place, whose
    backward is ``coverage_backward``.

    ``segs`` (``(n_segs, 4, 2)`` or ``(n_segs, 8)``) and ``m6`` (``(n_paths, 6)``) are float64 CUDA tensors and may require grad;
    the geometry never crosses the host.  ``kinds``, ``path_seg_off`` and ``rules`` are the topology: host arrays (checked and
    uploaded) or uint8 / int32 / uint8 CUDA tensors (used as they are).  ``dtype`` is torch.float32 (the default) or
    torch.float64; ``out``, if given, receives the result.  The work is ordered behind torch's current stream and torch's stream
    behind it; nothing waits, unless ``check=True``, which reads the kernels' status word -- a control point that is not finite or
    out of range, the flatten depth cap -- and raises on it.  torch must have been imported, and have touched CUDA, before the
    first call into this package (``tensor.IMPORT_ORDER``)."""
    torch = _torch()
    vp, flatness = _viewport(viewport), _flatness(flatness)
    for name, t in (("segs", segs), ("m6", m6)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} is a torch.Tensor, not {type(t).__name__}")
        if t.dtype != torch.float64 or not t.is_cuda:
            raise TypeError(f"{name} is a float64 tensor on the device, not {t.dtype} on {t.device}")
    if segs.dim() < 2 or segs.numel() != segs.shape[0] * 8:
        raise ValueError("segs is (n_segs, 4, 2) or (n_segs, 8): packed() segments")
    if m6.dim() != 2 or m6.shape[1] != 6 or m6.shape[0] < 1:
        raise ValueError("m6 is (n_paths, 6)")
    n_segs, n_paths = int(segs.shape[0]), int(m6.shape[0])
    if dtype is None:
        dtype = out.dtype if out is not None else torch.float32
    plane = {torch.float64: _abi.COVER_F64, torch.float32: _abi.COVER_F32}.get(dtype)
    if plane is None:
        raise TypeError(f"a coverage plane is torch.float32 or torch.float64, not {dtype!r}")
    _n_pixels(n_paths, vp)
    topo = (kinds, path_seg_off, rules)
    if all(isinstance(t, torch.Tensor) for t in topo):
        want = ((torch.uint8, n_segs), (torch.int32, n_paths + 1), (torch.uint8, n_paths))
        for t, (dt, n), name in zip(topo, want, ("kinds", "path_seg_off", "rules")):
            if t.dtype != dt or not t.is_cuda or t.numel() != n or not t.is_contiguous():
                raise TypeError(f"{name} on the device is a contiguous {dt} tensor of {n} elements")
    else:
        host = _topology(*(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in topo), n_segs, n_paths)
        topo = tuple(torch.from_numpy(a).to(segs.device) for a in host)
    ctx = _context(torch)
    if segs.device.index != ctx.device or m6.device != segs.device:
        raise ValueError(f"segs and m6 are on {segs.device} and {m6.device}, the library's context on device {ctx.device}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != (n_paths, vp[2], vp[3]) or not out.is_contiguous() \
                or out.device != segs.device:
            raise ValueError(f"out is a contiguous {dtype} tensor of shape {(n_paths, vp[2], vp[3])} on {segs.device}")
    return _function(torch).apply(segs, m6, out, *topo, vp, plane, flatness, bool(check))


# ------------------------------------------------------------------------------------------------------------------------------
# compositing: solid fills source-over in paint order, and the way back (svgr_compose_forward / svgr_compose_backward)
# ------------------------------------------------------------------------------------------------------------------------------
def compose_block() -> int:
    """Pixels per workgroup step of the compositing kernels (their launch seam)."""
    return int(_abi.load_library().svgr_compose_block())


def compose_groups() -> int:
    """The most workgroups the compositing backward launches: they stride over the pixels (its seam)."""
    return int(_abi.load_library().svgr_compose_groups())


def _is_tensor(x):
    return not isinstance(x, np.ndarray) and hasattr(x, "requires_grad")


def _alpha_split(rgba):
    if not _is_tensor(rgba):
        rgba = np.asarray(rgba, dtype=np.float64)
    if rgba.shape[-1:] != (4,):
        raise ValueError("colours are (..., 4): RGBA")
    return rgba, (_torch() if _is_tensor(rgba) else np)


def premultiply(rgba_straight):
    """Straight ``(..., 4)`` RGBA to the premultiplied form ``compose`` takes: numpy in, numpy out; torch in, torch out (and
    differentiable), so a caller can optimise straight colours.  No kernel."""
    rgba, xp = _alpha_split(rgba_straight)
    a = rgba[..., 3:]
    parts = (rgba[..., :3] * a, a)
    return xp.cat(parts, dim=-1) if xp is not np else np.concatenate(parts, axis=-1)


def unpremultiply(rgba_pre):
    """The inverse of ``premultiply``; where alpha is 0 the colour is 0."""
    rgba, xp = _alpha_split(rgba_pre)
    a = rgba[..., 3:]
    seen = a > 0
    parts = (xp.where(seen, rgba[..., :3] / xp.where(seen, a, a * 0 + 1), a * 0), a)
    return xp.cat(parts, dim=-1) if xp is not np else np.concatenate(parts, axis=-1)


def _compose_bg(bg):
    if bg is None:
        return None
    try:
        bg = np.asarray(bg, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("bg is 4 premultiplied doubles") from None
    if bg.shape != (4,) or not np.isfinite(bg).all():
        raise ValueError("bg is 4 finite premultiplied doubles")
    return tuple(float(v) for v in bg)


def _compose_desc(n_paths, rows, cols, plane, bg):
    d = _abi.ComposeDesc()
    d.n_paths, d.rows, d.cols, d.plane, d.has_bg = n_paths, rows, cols, plane, int(bg is not None)
    d.bg = (C.c_double * 4)(*(bg if bg is not None else (0.0,) * 4))
    return d


def _compose_inputs(cover, paints, bg, dtype=None):
    """cover (n_paths, rows, cols) of a plane type and paints (n_paths, 4) float64 on the host, checked."""
    cover = np.asarray(cover)
    if dtype is not None:
        if _np_dtype(dtype) not in _PLANES:
            raise TypeError(f"a coverage plane is float64 or float32, not {dtype!r}")
        cover = cover.astype(_np_dtype(dtype), copy=False)
    if cover.dtype not in _PLANES:
        raise TypeError(f"cover is float64 or float32, not {cover.dtype}")
    if cover.ndim != 3 or min(cover.shape) < 1:
        raise ValueError(f"cover is (n_paths, rows, cols) with every side positive, not {cover.shape}")
    if isinstance(paints, np.ndarray) and paints.dtype != np.float64:
        raise TypeError(f"paints is float64, not {paints.dtype}")
    try:
        paints = np.ascontiguousarray(paints, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("paints is (n_paths, 4): premultiplied RGBA") from None
    if paints.ndim != 2 or paints.shape[1] != 4:
        raise ValueError(f"paints is (n_paths, 4): premultiplied RGBA, not {paints.shape}")
    if len(paints) != len(cover):
        raise ValueError(f"{len(cover)} planes and {len(paints)} paints")
    if not np.isfinite(paints).all():
        raise ValueError("the paints must be finite")
    return np.ascontiguousarray(cover), paints, _compose_bg(bg)


def compose(cover, paints, bg=None, dtype=None):
    """The ``(rows, cols, 4)`` premultiplied image of ``n_paths`` solid fills painted source-over in paint order.

    ``cover`` is ``(n_paths, rows, cols)``, float64 or float32: what ``coverage`` returns.  ``paints`` is ``(n_paths, 4)`` float64,
    PREMULTIPLIED RGBA in the render's colour space, as the renderer's solid fill takes them (``premultiply`` makes them from
    straight colours); no colour conversion is done.  ``bg``, 4 premultiplied doubles, is what lies under the first path
    (transparent by default).  ``dtype``, if given, is the plane type ``cover`` is cast to first.  The arithmetic is the
    renderer's -- ``mask * paint``, then ``src + dst * (1 - src_a)`` -- in double, without a clamp; a float32 image is rounded once.
    Wrong shapes, dtypes and non-finite paints are refused before any device work."""
    cover, paints, bg = _compose_inputs(cover, paints, bg, dtype)
    n_paths, rows, cols = cover.shape
    _n_pixels(n_paths, (0, 0, rows, cols))
    ctx = _abi.Context.get()
    d_cover, d_paints = ctx.from_host(cover), ctx.from_host(paints)
    image = ctx.alloc(rows * cols * 4 * cover.dtype.itemsize)
    desc = _compose_desc(n_paths, rows, cols, _PLANES[cover.dtype], bg)
    _abi._check(ctx.lib.svgr_compose_forward(ctx.handle, C.byref(desc), d_cover.handle, d_paints.handle, image.handle))
    return image.download((rows, cols, 4), cover.dtype)


def compose_backward(cover, paints, grad_image, bg=None):
    """``(grad_cover, grad_paints)``: the derivative of ``sum(grad_image * compose(cover, paints, bg))``.

    ``grad_image`` has the image's shape and ``cover``'s type.  ``grad_cover`` has ``cover``'s shape and type, ``grad_paints`` is
    ``(n_paths, 4)`` float64; ``bg`` is a constant and has no gradient.  No division (an opaque paint on a covered pixel is no
    special case) and no atomics: the same bits on every run."""
    cover, paints, bg = _compose_inputs(cover, paints, bg)
    n_paths, rows, cols = cover.shape
    grad_image = np.asarray(grad_image)
    if grad_image.dtype != cover.dtype:
        raise TypeError(f"grad_image is {cover.dtype} like cover, not {grad_image.dtype}")
    if grad_image.shape != (rows, cols, 4):
        raise ValueError(f"grad_image is {(rows, cols, 4)}, not {grad_image.shape}")
    _n_pixels(n_paths, (0, 0, rows, cols))
    ctx = _abi.Context.get()
    d_cover, d_paints, d_grad = ctx.from_host(cover), ctx.from_host(paints), ctx.from_host(np.ascontiguousarray(grad_image))
    g_cover, g_paints = ctx.alloc(cover.nbytes), ctx.alloc(n_paths * 32)
    desc = _compose_desc(n_paths, rows, cols, _PLANES[cover.dtype], bg)
    _abi._check(ctx.lib.svgr_compose_backward(ctx.handle, C.byref(desc), d_cover.handle, d_paints.handle, d_grad.handle, g_cover.handle, g_paints.handle))
    return g_cover.download(cover.shape, cover.dtype), g_paints.download((n_paths, 4), np.float64)


@functools.lru_cache(maxsize=None)
def _compose_function(torch):
    class Compose(torch.autograd.Function):
        """image = Compose.apply(planes, paints, out, bg)."""

        @staticmethod
        def forward(fn, planes, paints, out, bg):
            ctx = _context(torch)
            n_paths, rows, cols = (int(v) for v in planes.shape)
            plane = _abi.COVER_F64 if planes.dtype == torch.float64 else _abi.COVER_F32
            planes_c, paints_c = planes.detach().contiguous(), paints.detach().contiguous()
            image = out if out is not None else torch.empty((rows, cols, 4), dtype=planes.dtype, device=planes.device)
            desc = _compose_desc(n_paths, rows, cols, plane, bg)
            with _Ordered(ctx, torch):
                b = _buffers(ctx, torch, planes_c, paints_c, image)
                _abi._check(ctx.lib.svgr_compose_forward(ctx.handle, C.byref(desc), *[_h(x) for x in b]))
            fn.save_for_backward(planes_c, paints_c)
            fn.compose_desc = desc
            if out is not None:
                fn.mark_dirty(out)
            return image

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(fn, grad):
            planes_c, paints_c = fn.saved_tensors
            ctx = _context(torch)
            grad = grad.contiguous()
            if grad.data_ptr() % 16:
                grad = grad.clone(memory_format=torch.contiguous_format)
            grad_planes, grad_paints = torch.empty_like(planes_c), torch.empty_like(paints_c)
            with _Ordered(ctx, torch):
                b = _buffers(ctx, torch, planes_c, paints_c, grad, grad_planes, grad_paints)
                _abi._check(ctx.lib.svgr_compose_backward(ctx.handle, C.byref(fn.compose_desc), *[_h(x) for x in b]))
            need = fn.needs_input_grad
            return grad_planes if need[0] else None, grad_paints if need[1] else None, None, None

    return Compose


def compose_tensor(planes, paints, *, bg=None, out=None):
    """``compose`` as a ``torch.autograd.Function``: a ``(rows, cols, 4)`` premultiplied image of ``planes``' type that the kernel
    writes in place, whose backward is ``compose_backward``.

    ``planes`` is an ``(n_paths, rows, cols)`` float32 or float64 CUDA tensor (``coverage_tensor``'s result), ``paints`` an
    ``(n_paths, 4)`` float64 CUDA tensor of premultiplied colours; either may require grad.  ``bg`` is 4 premultiplied numbers on
    the host, a constant.  ``out``, if given, receives the image.  The work is ordered behind torch's current stream and torch's
    stream behind it; nothing waits.  The import-order rule is ``coverage_tensor``'s (``tensor.IMPORT_ORDER``)."""
    torch = _torch()
    for name, t, kinds in (("planes", planes, (torch.float32, torch.float64)), ("paints", paints, (torch.float64,))):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} is a torch.Tensor, not {type(t).__name__}")
        if t.dtype not in kinds or not t.is_cuda:
            raise TypeError(f"{name} is a {' or '.join(str(k) for k in kinds)} tensor on the device, not {t.dtype} on {t.device}")
    if planes.dim() != 3 or min(planes.shape) < 1:
        raise ValueError(f"planes is (n_paths, rows, cols) with every side positive, not {tuple(planes.shape)}")
    if paints.dim() != 2 or paints.shape[1] != 4 or paints.shape[0] != planes.shape[0]:
        raise ValueError(f"paints is ({planes.shape[0]}, 4): one premultiplied RGBA per plane, not {tuple(paints.shape)}")
    n_paths, rows, cols = (int(v) for v in planes.shape)
    _n_pixels(n_paths, (0, 0, rows, cols))
    bg = _compose_bg(bg)
    ctx = _context(torch)
    if planes.device.index != ctx.device or paints.device != planes.device:
        raise ValueError(f"planes and paints are on {planes.device} and {paints.device}, the library's context on device {ctx.device}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != planes.dtype or tuple(out.shape) != (rows, cols, 4) or not out.is_contiguous() \
                or out.device != planes.device or out.data_ptr() % 16:
            raise ValueError(f"out is a contiguous {planes.dtype} tensor of shape {(rows, cols, 4)} on {planes.device}, aligned to 16 bytes")
    return _compose_function(torch).apply(planes, paints, out, bg)


def render_tensor(segs, m6, paints, *, kinds, path_seg_off, rules, viewport, bg=None, dtype=None, check: bool = False, flatness: float = FLATNESS):
    """Geometry and colours to a ``(rows, cols, 4)`` premultiplied image and back: ``coverage_tensor`` followed by
    ``compose_tensor``, with gradients to ``segs``, ``m6`` and ``paints``.

    Path ``p`` is filled with ``paints[p]`` and painted over the paths before it.  The arguments are ``coverage_tensor``'s and
    ``compose_tensor``'s; ``dtype`` (torch.float32 by default) is the type of the planes and of the image.  Solid fills only: no
    gradients or patterns, clips, groups or strokes."""
    planes = coverage_tensor(segs, m6, kinds=kinds, path_seg_off=path_seg_off, rules=rules, viewport=viewport, dtype=dtype, check=check, flatness=flatness)
    return compose_tensor(planes, paints, bg=bg)


# ------------------------------------------------------------------------------------------------------------------------------
# gradient paints: linear and one-circle radial fills in the compositor (svgr_compose_painted_forward / _backward,
# csrc/svgr_gradpaint.h)
# ------------------------------------------------------------------------------------------------------------------------------
MAX_STOPS = 32
KIND_SOLID, KIND_LINEAR, KIND_RADIAL = 0, 1, 2


class GradientPaints(NamedTuple):
    """What paints every path of a painted composition besides its ``paints`` row.  The topology -- ``kind`` (0 solid, 1 linear,
    2 radial), ``spread`` (0 pad, 1 repeat, 2 reflect) and ``path_stop_off`` (path ``p`` owns the stops
    ``path_stop_off[p] : path_stop_off[p + 1]``; a solid path owns none, a gradient path 1 to 32) -- stays on the host.  ``m6``
    ``(n_paths, 6)`` takes a pixel centre to gradient space, ``geom`` ``(n_paths, 4)`` is ``p0x, p0y, p1x, p1y`` of a linear and
    ``cx, cy, r, -`` of a radial gradient, ``stop_pos`` ``(n_stops,)`` and ``stop_rgba`` ``(n_stops, 4)`` are the stops, premultiplied
    and in the render's colour space.  ``compose_painted_backward`` returns the derivatives in the same shape."""

    kind: object
    spread: object
    path_stop_off: object
    m6: object
    geom: object
    stop_pos: object
    stop_rgba: object


def gradient_paints(paints, transform=None, linear_rgb: bool = False):
    """``(GradientPaints, paint_rows)`` of a list of ``paint.GradLinear``, ``paint.GradRadial`` or 4-number solid colours drawn
    under the render transform ``transform`` (identity by default).

    ``m6`` is the inverse render transform followed by the gradient's inverse ``gradientTransform``, composed into one matrix;
    the stops go through the renderer's colour-space step for ``linear_rgb`` (a gradient's own ``linear_rgb`` wins, as in
    ``Path.fill``).  ``paint_rows`` is ``(n_paths, 4)``: the colour of a solid path as given (premultiplied, in the render's colour
    space: what ``compose`` takes), ones for a gradient path.  A focal radial gradient, ``bbox_units=True``, an unknown spread, no
    stop or more than 32 stops is a ``ValueError``.  Host only: no device work."""
    from .geometry import Transform  # noqa: PLC0415
    from .paint import _SPREAD, GradLinear, GradRadial, _stops_colorspace  # noqa: PLC0415

    user = (transform if transform is not None else Transform()).invert
    kind, spread, off, m6, geom, pos, rgba, rows = [], [], [0], [], [], [], [], []
    for p, paint in enumerate(paints):
        if not isinstance(paint, (GradLinear, GradRadial)):
            try:
                colour = np.asarray(paint, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                colour = np.zeros(0)
            if colour.shape != (4,):
                raise ValueError(f"paint {p} is a GradLinear, a GradRadial or 4 numbers")
            kind.append(KIND_SOLID), spread.append(0), off.append(off[-1]), m6.append(Transform().m6()), geom.append((0.0,) * 4), rows.append(colour)
            continue
        if paint.bbox_units:
            raise ValueError(f"paint {p}: objectBoundingBox units are not supported")
        if paint.spread not in _SPREAD:
            raise ValueError(f"paint {p}: invalid spread method: {paint.spread}")
        if isinstance(paint, GradRadial):
            if paint.fcenter is not None or paint.fradius is not None:
                raise ValueError(f"paint {p}: focal radial gradients are not supported")
            c = np.asarray(paint.center, dtype=np.float64).reshape(2)
            kind.append(KIND_RADIAL), geom.append((c[0], c[1], float(paint.radius), 0.0))
        else:
            p0, p1 = np.asarray(paint.p0, dtype=np.float64).reshape(2), np.asarray(paint.p1, dtype=np.float64).reshape(2)
            kind.append(KIND_LINEAR), geom.append((p0[0], p0[1], p1[0], p1[1]))
        stops = _stops_colorspace(paint.stops, linear_rgb if paint.linear_rgb is None else paint.linear_rgb)
        if not 1 <= len(stops) <= MAX_STOPS:
            raise ValueError(f"paint {p} has {len(stops)} stops: 1 to {MAX_STOPS}")
        tr = user if paint.transform is None else paint.transform.invert @ user
        spread.append(_SPREAD[paint.spread]), m6.append(tr.m6()), rows.append(np.ones(4))
        pos += [o for o, _ in stops]
        rgba += [np.asarray(c, dtype=np.float64).reshape(4) for _, c in stops]
        off.append(len(pos))
    if not kind:
        raise ValueError("no paints")
    gp = GradientPaints(np.array(kind, dtype=np.int32), np.array(spread, dtype=np.int32), np.array(off, dtype=np.int32),
                        np.array(m6, dtype=np.float64).reshape(-1, 6), np.array(geom, dtype=np.float64).reshape(-1, 4), np.array(pos, dtype=np.float64),
                        np.array(rgba, dtype=np.float64).reshape(-1, 4))
    return gp, np.array(rows, dtype=np.float64).reshape(-1, 4)


def _painted_topology(gp, n_paths, n_stops):
    """kind, spread and path_stop_off on the host, checked as svgr_compose_painted_forward checks them: three int32 arrays."""
    if not isinstance(gp, tuple) or len(gp) != 7:
        raise TypeError("gp is a GradientPaints")
    out = []
    for name, a, n in (("kind", gp.kind, n_paths), ("spread", gp.spread, n_paths), ("path_stop_off", gp.path_stop_off, n_paths + 1)):
        if _is_tensor(a):
            raise TypeError(f"gp.{name} stays on the host: a numpy array or a list")
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise TypeError(f"gp.{name} holds integers, not {a.dtype}")
        if a.shape != (n,):
            raise ValueError(f"gp.{name} has {n} entries, not {a.shape}")
        out.append(np.ascontiguousarray(a.astype(np.int64)))
    kind, spread, off = out
    if not np.isin(kind, (KIND_SOLID, KIND_LINEAR, KIND_RADIAL)).all():
        raise ValueError("gp.kind holds 0 (solid), 1 (linear) or 2 (radial) per path")
    if not np.isin(spread, (0, 1, 2)).all():
        raise ValueError("gp.spread holds 0 (pad), 1 (repeat) or 2 (reflect) per path")
    count = np.diff(off)
    if off[0] != 0 or off[-1] != n_stops or (count < 0).any():
        raise ValueError(f"gp.path_stop_off is n_paths + 1 ascending integers from 0 to the number of stops ({n_stops})")
    if (count[kind == KIND_SOLID] != 0).any():
        raise ValueError("a solid path owns no stops")
    if ((count[kind != KIND_SOLID] < 1) | (count[kind != KIND_SOLID] > MAX_STOPS)).any():
        raise ValueError(f"a gradient path owns 1 to {MAX_STOPS} stops")
    return kind.astype(np.int32), spread.astype(np.int32), off.astype(np.int32)


def _origin(origin):
    try:
        o = tuple(int(v) for v in origin)
    except (TypeError, ValueError):
        raise ValueError("origin is (row0, col0)") from None
    if len(o) != 2 or max(abs(o[0]), abs(o[1])) > 2 ** 30:
        raise ValueError("origin is (row0, col0), within +-2^30")
    return o


def _painted_desc(n_paths, rows, cols, plane, bg, origin, topo, n_stops, cls=_abi.PaintedDesc):
    """(svgr_painted_desc, what it points at).  ``cls`` may be a description that begins with one."""
    d = cls()
    d.n_paths, d.rows, d.cols, d.plane, d.has_bg = n_paths, rows, cols, plane, int(bg is not None)
    d.bg = (C.c_double * 4)(*(bg if bg is not None else (0.0,) * 4))
    d.row0, d.col0, d.n_stops = origin[0], origin[1], n_stops
    d.kind, d.spread, d.path_stop_off = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in topo)
    return d, topo


_GP_ARRAYS = (("m6", 6), ("geom", 4), ("stop_pos", None), ("stop_rgba", 4))


def _painted_inputs(cover, paints, gp, bg, origin, dtype=None):
    """Everything of a numpy call on the host, checked: (cover, paints, bg, origin, topo, [m6, geom, stop_pos, stop_rgba])."""
    cover, paints, bg = _compose_inputs(cover, paints, bg, dtype)
    origin = _origin(origin)
    n_paths = len(cover)
    if not isinstance(gp, tuple) or len(gp) != 7:
        raise TypeError("gp is a GradientPaints")
    arrays = []
    for name, width in _GP_ARRAYS:
        a = getattr(gp, name)
        if _is_tensor(a):
            raise TypeError(f"gp.{name} is a numpy array here; compose_painted_tensor takes tensors")
        if isinstance(a, np.ndarray) and a.dtype != np.float64:
            raise TypeError(f"gp.{name} is float64, not {a.dtype}")
        try:
            a = np.ascontiguousarray(a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"gp.{name} is an array of doubles") from None
        want = (n_paths, width) if name in ("m6", "geom") else ((len(a),) if width is None else (len(a), width))
        if a.ndim != len(want) or a.shape != want:
            raise ValueError(f"gp.{name} is {want if name in ('m6', 'geom') else ('n_stops',) + want[1:]}, not {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"gp.{name} must be finite")
        arrays.append(a)
    m6, geom, pos, rgba = arrays
    if len(rgba) != len(pos):
        raise ValueError(f"{len(pos)} stop positions and {len(rgba)} stop colours")
    topo = _painted_topology(gp, n_paths, len(pos))
    kind, _spread, off = topo
    lin, rad = kind == KIND_LINEAR, kind == KIND_RADIAL
    if (geom[lin, :2] == geom[lin, 2:]).all(axis=1).any():
        raise ValueError("a linear gradient needs p0 != p1")
    if (geom[rad, 2] <= 0.0).any():
        raise ValueError("a radial gradient needs r > 0")
    for p in np.nonzero(kind != KIND_SOLID)[0]:
        if (np.diff(pos[off[p]:off[p + 1]]) < 0.0).any():
            raise ValueError(f"the stop positions of path {p} decrease")
    return cover, paints, bg, origin, topo, arrays


def compose_painted(cover, paints, gp, bg=None, origin=(0, 0), dtype=None):
    """``compose`` with gradient paints: the ``(rows, cols, 4)`` premultiplied image of ``n_paths`` fills painted source-over in
    paint order, path ``p`` a solid fill of ``paints[p]`` (``gp.kind[p] == 0``) or the renderer's linear or radial gradient,
    evaluated at the pixel centres of the viewport with origin ``origin = (row0, col0)``, times the coverage, times ``paints[p]``
    component-wise (ones, or an opacity).  ``gp`` is a ``GradientPaints`` of numpy arrays (``gradient_paints`` builds one).  The
    arithmetic is the renderer's, in double; a float32 image is rounded once.  Wrong shapes and dtypes, non-finite values,
    ``p0 == p1``, ``r <= 0``, decreasing stop positions and every error of the topology are refused before any device work."""
    return _tier_forward("painted", cover, paints, gp, None, bg, origin, dtype)


def compose_painted_backward(cover, paints, gp, grad_image, bg=None, origin=(0, 0)):
    """``(grad_cover, grad_paints, grad_gp)``: the derivative of ``sum(grad_image * compose_painted(cover, paints, gp, bg, origin))``.

    ``grad_image`` has the image's shape and ``cover``'s type.  ``grad_gp`` is a ``GradientPaints`` with ``gp``'s topology and the
    derivatives with respect to ``m6``, ``geom``, ``stop_pos`` and ``stop_rgba`` (float64); the rows of solid paths and a radial
    gradient's unused slot are 0.  Where a derivative is not defined -- an offset exactly on a stop, a clamp, a wrap or a fold,
    the radial centre -- one side is taken and nothing is NaN.  No atomics: the same bits on every run."""
    return _tier_backward("painted", cover, paints, gp, None, grad_image, bg, origin)


def _tensor_args(torch, planes, paints_t, gp_t, program=None):
    """The types, dtypes and shapes of a tensor call's arguments, checked: ``(named, n_stops)``, ``named`` the tensors as
    ``(name, tensor, dtypes)``.  The program tiers pass ``program = (groups, opacity_t)``."""
    if not isinstance(gp_t, tuple) or len(gp_t) != 7:
        raise TypeError("gp_t is a GradientPaints")
    if program is not None and not isinstance(program[0], Groups):
        raise TypeError("groups is a Groups")
    named = (("planes", planes, (torch.float32, torch.float64)), ("paints_t", paints_t, (torch.float64,))) \
        + tuple((f"gp_t.{name}", getattr(gp_t, name), (torch.float64,)) for name, _w in _GP_ARRAYS)
    if program is not None:
        named += (("opacity_t", program[1], (torch.float64,)),)
    for name, t, kinds in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} is a torch.Tensor, not {type(t).__name__}")
        if t.dtype not in kinds or not t.is_cuda:
            raise TypeError(f"{name} is a {' or '.join(str(k) for k in kinds)} tensor on the device, not {t.dtype} on {t.device}")
    if planes.dim() != 3 or min(planes.shape) < 1:
        raise ValueError(f"planes is (n_paths, rows, cols) with every side positive, not {tuple(planes.shape)}")
    n_paths = int(planes.shape[0])
    n_stops = int(gp_t.stop_pos.shape[0]) if gp_t.stop_pos.dim() == 1 else -1
    for name, t, want in (("paints_t", paints_t, (n_paths, 4)), ("gp_t.m6", gp_t.m6, (n_paths, 6)), ("gp_t.geom", gp_t.geom, (n_paths, 4)),
                          ("gp_t.stop_pos", gp_t.stop_pos, (max(n_stops, 0),)), ("gp_t.stop_rgba", gp_t.stop_rgba, (max(n_stops, 0), 4))):
        if tuple(t.shape) != want or n_stops < 0:
            raise ValueError(f"{name} is {want}, not {tuple(t.shape)}")
    if program is not None and program[1].dim() != 1:
        raise ValueError(f"opacity_t is (n_opacities,), not {tuple(program[1].shape)}")
    return named, n_stops


def _tensor_places(torch, named, planes, out):
    """Every tensor of ``named`` on ``planes``' device, which is the library's context's; ``out``, if given, fit for the image."""
    ctx = _context(torch)
    for name, t, _k in named:
        if t.device != planes.device or t.device.index != ctx.device:
            raise ValueError(f"{name} is on {t.device}, planes on {planes.device}, the library's context on device {ctx.device}")
    if out is not None:
        shape = (int(planes.shape[1]), int(planes.shape[2]), 4)
        if not isinstance(out, torch.Tensor) or out.dtype != planes.dtype or tuple(out.shape) != shape or not out.is_contiguous() \
                or out.device != planes.device or out.data_ptr() % 16:
            raise ValueError(f"out is a contiguous {planes.dtype} tensor of shape {shape} on {planes.device}, aligned to 16 bytes")


def compose_painted_tensor(planes, paints_t, gp_t, *, bg=None, origin=(0, 0), out=None):
    """``compose_painted`` as a ``torch.autograd.Function``: a ``(rows, cols, 4)`` premultiplied image of ``planes``' type that the
    kernel writes in place, whose backward is ``compose_painted_backward``.

    ``planes`` is an ``(n_paths, rows, cols)`` float32 or float64 CUDA tensor, ``paints_t`` an ``(n_paths, 4)`` float64 CUDA tensor;
    ``gp_t`` is a ``GradientPaints`` whose ``m6``, ``geom``, ``stop_pos`` and ``stop_rgba`` are float64 CUDA tensors and whose
    topology (``kind``, ``spread``, ``path_stop_off``) stays on the host.  Any of the six tensors may require grad.  ``bg``,
    ``origin`` and ``out`` are ``compose_painted``'s and ``compose_tensor``'s, and so are the stream ordering and the import-order
    rule (``tensor.IMPORT_ORDER``).  Only the topology, shapes, dtypes and devices are checked: there is no host wait, so the
    VALUES are not looked at.  Degenerate ones -- ``p0 == p1``, ``r <= 0``, non-finite numbers, decreasing stop positions -- give
    NaN, infinities or a wrong stop, not an error."""
    torch = _torch()
    named, n_stops = _tensor_args(torch, planes, paints_t, gp_t)
    n_paths, rows, cols = (int(v) for v in planes.shape)
    _n_pixels(n_paths, (0, 0, rows, cols))
    topo = _painted_topology(gp_t, n_paths, n_stops)
    bg, origin = _compose_bg(bg), _origin(origin)
    _tensor_places(torch, named, planes, out)
    return _tier_function(torch, "painted").apply(out, (bg, origin, topo), *(t for _n, t, _k in named))


def render_painted_tensor(segs, m6, paints, gp, *, kinds, path_seg_off, rules, viewport, bg=None, dtype=None, check: bool = False,
                          flatness: float = FLATNESS):
    """Geometry, colours and gradients to a ``(rows, cols, 4)`` premultiplied image and back: ``coverage_tensor`` followed by
    ``compose_painted_tensor`` with ``origin`` from ``viewport``, with gradients to ``segs``, ``m6``, ``paints`` and the four
    tensors of ``gp``.  The arguments are theirs; ``dtype`` (torch.float32 by default) is the type of the planes and of the image."""
    vp = _viewport(viewport)
    planes = coverage_tensor(segs, m6, kinds=kinds, path_seg_off=path_seg_off, rules=rules, viewport=vp, dtype=dtype, check=check, flatness=flatness)
    return compose_painted_tensor(planes, paints, gp, bg=bg, origin=(vp[0], vp[1]))


# ------------------------------------------------------------------------------------------------------------------------------
# isolated groups: group opacity and clip paths in the compositor (svgr_compose_grouped_forward / _backward, csrc/svgr_group.h,
# DESIGN.md 7z)
# ------------------------------------------------------------------------------------------------------------------------------
OP_FILL, OP_BEGIN, OP_END = 0, 1, 2
MAX_ITEMS = 1 << 24


def group_depth() -> int:
    """How deep groups may nest below the root (svgr_group_depth())."""
    return int(_abi.load_library().svgr_group_depth())


class Group:
    """An isolated group of a grouped composition: ``children`` is a list of plane indices (fills) and ``Group``s in paint order,
    ``opacity`` a number or None, ``clip`` a list of plane indices (the clip's coverage planes, composed OVER in one channel in
    that order) or None.  The group is painted on a transparent canvas, multiplied by the opacity, then by the clip's mask, and
    composed OVER what lies below: the renderer's ``CLIP(OPACITY(GROUP))``.  ``mask`` is None or the mask's own tree, a list of
    plane indices and ``Group``s: it is painted on a transparent canvas of its own, reduced to luminance times alpha per pixel,
    and multiplies the group after the clip: ``MASK(CLIP(OPACITY(GROUP)))``.  Only ``mask_program`` takes a tree with masks."""

    __slots__ = ("children", "opacity", "clip", "mask")

    def __init__(self, children, opacity=None, clip=None, mask=None):
        self.children, self.opacity, self.clip = list(children), opacity, (None if clip is None else list(clip))
        self.mask = None if mask is None else list(mask)

    def __repr__(self):
        mask = "" if self.mask is None else f", mask={self.mask!r}"
        return f"Group({self.children!r}, opacity={self.opacity!r}, clip={self.clip!r}{mask})"


class Groups(NamedTuple):
    """The program of a grouped composition.  The topology stays on the host: ``items`` ``(n_items, 4)`` int32 -- ``{0, p, 0, 0}``
    paints plane ``p``, ``{1, index of its END, 0, 0}`` opens a group, ``{2, index of its BEGIN, opacity slot or -1, clip or -1}``
    closes it --, ``clip_off`` and ``clip_planes`` (clip ``c`` is the planes ``clip_planes[clip_off[c] : clip_off[c + 1]]``).
    ``opacity`` is float64 ``(n_opacities,)``: a numpy array, or a CUDA tensor for ``compose_grouped_tensor``."""

    items: object
    clip_off: object
    clip_planes: object
    opacity: object


def group_program(tree):
    """The ``Groups`` of a tree: a list of ints (fills) and ``Group``s in paint order.  Opacity slots and clips are numbered in
    the order their groups CLOSE.  Only the tree's own form is checked here; ``compose_grouped`` checks the program against the
    planes (every plane used exactly once, the depth)."""
    items, clip_off, clip_planes, opacity = [], [0], [], []

    def walk(children):
        if isinstance(children, (Group, int, np.integer)) or not hasattr(children, "__iter__"):
            raise TypeError("a tree is a list of plane indices and Groups")
        for child in children:
            if isinstance(child, Group):
                if child.mask is not None:
                    raise ValueError("a group has a mask: mask_program makes the program of such a tree, compose_masked draws it")
                begin = len(items)
                items.append([OP_BEGIN, -1, 0, 0])
                walk(child.children)
                slot = clip = -1
                if child.opacity is not None:
                    slot = len(opacity)
                    opacity.append(float(child.opacity))
                if child.clip is not None:
                    if len(child.clip) == 0:
                        raise ValueError("a clip has at least one plane")
                    clip = len(clip_off) - 1
                    clip_planes.extend(int(p) for p in child.clip)
                    clip_off.append(len(clip_planes))
                items[begin][1] = len(items)
                items.append([OP_END, begin, slot, clip])
            elif isinstance(child, (int, np.integer)) and not isinstance(child, bool):
                items.append([OP_FILL, int(child), 0, 0])
            else:
                raise TypeError(f"a tree holds plane indices and Groups, not {type(child).__name__}")

    walk(tree)
    return Groups(np.array(items, dtype=np.int32).reshape(-1, 4), np.array(clip_off, dtype=np.int32), np.array(clip_planes, dtype=np.int32),
                  np.array(opacity, dtype=np.float64))


def _program_tables(groups):
    """items, clip_off and clip_planes of a program as int64 arrays of the right dimensions."""
    if not isinstance(groups, Groups):
        raise TypeError("groups is a Groups")
    out = []
    for name, a in (("items", groups.items), ("clip_off", groups.clip_off), ("clip_planes", groups.clip_planes)):
        if _is_tensor(a):
            raise TypeError(f"groups.{name} stays on the host: a numpy array or a list")
        a = np.asarray(a)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"groups.{name} holds integers, not {a.dtype}")
        out.append(np.ascontiguousarray(a.astype(np.int64)))
    items, clip_off, clip_planes = out
    if items.ndim != 2 or items.shape[1] != 4 or len(items) < 1:
        raise ValueError(f"groups.items is (n_items, 4) with at least one item, not {items.shape}")
    if len(items) > MAX_ITEMS:
        raise ValueError(f"a program has at most {MAX_ITEMS} items")
    if clip_off.ndim != 1 or clip_planes.ndim != 1:
        raise ValueError("groups.clip_off and groups.clip_planes are lists of integers")
    return items, clip_off, clip_planes


def _program_uses(items, clip_off, clip_planes, planes, slots, clips):
    """What is left to check once a program's items are walked: the opacity slots, the clips and the planes' uses, counted in
    ``slots``, ``clips`` and ``planes``.  The three tables as the ABI takes them."""
    n_paths = len(planes)
    if (slots != 1).any():
        raise ValueError("every opacity slot is used by exactly one group")
    if sorted(clips) != list(range(len(clips))):
        raise ValueError(f"the {len(clips)} clips are numbered from 0")
    if clips or len(clip_planes):
        count = np.diff(clip_off)
        if len(clip_off) != len(clips) + 1 or clip_off[0] != 0 or clip_off[-1] != len(clip_planes) or (count < 1).any():
            raise ValueError("groups.clip_off is n_clips + 1 strictly ascending integers from 0 to the number of clip planes")
        if ((clip_planes < 0) | (clip_planes >= n_paths)).any():
            raise ValueError(f"a clip plane is not one of {n_paths}")
        np.add.at(planes, clip_planes, 1)
    if (planes != 1).any():
        p = int(np.nonzero(planes != 1)[0][0])
        raise ValueError(f"plane {p} is used {int(planes[p])} times: every plane is used exactly once, by a FILL or as a clip plane")
    if len(clip_off) == 0:
        clip_off = np.zeros(1, dtype=np.int64)
    return np.ascontiguousarray(items, dtype=np.int32), clip_off.astype(np.int32), clip_planes.astype(np.int32)


def _group_topology(groups, n_paths, n_opacities):
    """items, clip_off and clip_planes on the host, checked as svgr_compose_grouped_forward checks them: (three int32 arrays,
    n_groups)."""
    items, clip_off, clip_planes = _program_tables(groups)
    depth_max = group_depth()
    planes, slots, clips = np.zeros(n_paths, dtype=np.int64), np.zeros(n_opacities, dtype=np.int64), {}
    stack, n_groups = [], 0
    for i, (op, a, slot, clip) in enumerate(items.tolist()):
        if op == OP_FILL:
            if not 0 <= a < n_paths:
                raise ValueError(f"item {i}: FILL of plane {a}, not one of {n_paths}")
            planes[a] += 1
        elif op == OP_BEGIN:
            if not i < a < len(items) or items[a, 0] != OP_END or items[a, 1] != i:
                raise ValueError(f"item {i}: BEGIN without its END")
            if len(stack) == depth_max:
                raise ValueError(f"item {i}: groups nest deeper than {depth_max}")
            stack.append(i)
            n_groups += 1
        elif op == OP_END:
            if not stack or stack[-1] != a:
                raise ValueError(f"item {i}: END does not close the open group")
            stack.pop()
            if slot != -1:
                if not 0 <= slot < n_opacities:
                    raise ValueError(f"item {i}: opacity slot {slot}, not one of {n_opacities}")
                slots[slot] += 1
            if clip != -1:
                if clip < 0 or clip in clips:
                    raise ValueError(f"item {i}: clip {clip} is negative or used twice")
                clips[clip] = i
        else:
            raise ValueError(f"item {i}: unknown op {op} (0 FILL, 1 BEGIN, 2 END)")
    if stack:
        raise ValueError(f"item {stack[-1]}: the group is not closed")
    return _program_uses(items, clip_off, clip_planes, planes, slots, clips), n_groups


def _grouped_desc(n_paths, rows, cols, plane, bg, origin, topo, n_stops, gtopo, n_groups, n_opacities):
    """(svgr_grouped_desc, what it points at)."""
    d, _topo = _painted_desc(n_paths, rows, cols, plane, bg, origin, topo, n_stops, _abi.GroupedDesc)
    d.n_items, d.n_groups, d.n_clip_planes, d.n_opacities = len(gtopo[0]), n_groups, len(gtopo[2]), n_opacities
    d.items, d.clip_off, d.clip_planes = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in gtopo)
    return d, (topo, gtopo)


# The painted, grouped and masked entries are one binding in three tiers ("painted", "grouped", "masked": the word in the ABI's
# entry names).  The painted tier has no program: its opacity and gtopo are None, its n_groups 0.
def _tier_desc(n_paths, rows, cols, plane, bg, origin, topo, n_stops, gtopo=None, n_groups=0, n_opacities=0):
    """The tier's description: ``_painted_desc`` without a program, ``_grouped_desc`` with one."""
    if gtopo is None:
        return _painted_desc(n_paths, rows, cols, plane, bg, origin, topo, n_stops)
    return _grouped_desc(n_paths, rows, cols, plane, bg, origin, topo, n_stops, gtopo, n_groups, n_opacities)


def _tier_inputs(tier, cover, paints, gp, groups, bg, origin, dtype=None):
    """``_painted_inputs`` and, for "grouped" and "masked", the tier's program, checked."""
    cover, paints, bg, origin, topo, arrays = _painted_inputs(cover, paints, gp, bg, origin, dtype)
    if tier == "painted":
        return cover, paints, bg, origin, topo, arrays, None, None, 0
    if not isinstance(groups, Groups):
        raise TypeError("groups is a Groups")
    opacity = groups.opacity
    if _is_tensor(opacity):
        raise TypeError(f"groups.opacity is a numpy array here; compose_{tier}_tensor takes a tensor")
    if isinstance(opacity, np.ndarray) and opacity.size and opacity.dtype != np.float64:
        raise TypeError(f"groups.opacity is float64, not {opacity.dtype}")
    try:
        opacity = np.ascontiguousarray(opacity, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("groups.opacity is an array of doubles") from None
    if opacity.ndim != 1:
        raise ValueError(f"groups.opacity is (n_opacities,), not {opacity.shape}")
    if not np.isfinite(opacity).all():
        raise ValueError("groups.opacity must be finite")
    gtopo, n_groups = _PROGRAM_TOPOLOGY[tier](groups, len(cover), len(opacity))
    return cover, paints, bg, origin, topo, arrays, opacity, gtopo, n_groups


def _tier_forward(tier, cover, paints, gp, groups, bg, origin, dtype):
    """``compose_painted``, ``compose_grouped`` or ``compose_masked``: svgr_compose_<tier>_forward on numpy arrays."""
    cover, paints, bg, origin, topo, arrays, opacity, gtopo, n_groups = _tier_inputs(tier, cover, paints, gp, groups, bg, origin, dtype)
    n_paths, rows, cols = cover.shape
    _n_pixels(max(n_paths, n_groups), (0, 0, rows, cols))
    ctx = _abi.Context.get()
    ins, n_op = (arrays, 0) if opacity is None else (arrays + [opacity], len(opacity))
    bufs = [ctx.from_host(cover), ctx.from_host(paints)] + [ctx.from_host(a) if a.size else None for a in ins]
    image = ctx.alloc(rows * cols * 4 * cover.dtype.itemsize)
    desc, _keep = _tier_desc(n_paths, rows, cols, _PLANES[cover.dtype], bg, origin, topo, len(arrays[2]), gtopo, n_groups, n_op)
    _abi._check(getattr(ctx.lib, f"svgr_compose_{tier}_forward")(ctx.handle, C.byref(desc), *[_h(b) for b in bufs], image.handle))
    return image.download((rows, cols, 4), cover.dtype)


def _tier_backward(tier, cover, paints, gp, groups, grad_image, bg, origin):
    """``compose_painted_backward``, ``compose_grouped_backward`` or ``compose_masked_backward``: svgr_compose_<tier>_backward on
    numpy arrays.  ``grad_opacity`` ends the result of the tiers that have opacities."""
    cover, paints, bg, origin, topo, arrays, opacity, gtopo, n_groups = _tier_inputs(tier, cover, paints, gp, groups, bg, origin)
    n_paths, rows, cols = cover.shape
    grad_image = np.asarray(grad_image)
    if grad_image.dtype != cover.dtype:
        raise TypeError(f"grad_image is {cover.dtype} like cover, not {grad_image.dtype}")
    if grad_image.shape != (rows, cols, 4):
        raise ValueError(f"grad_image is {(rows, cols, 4)}, not {grad_image.shape}")
    _n_pixels(max(n_paths, n_groups), (0, 0, rows, cols))
    n_stops = len(arrays[2])
    ins, n_op = (arrays, 0) if opacity is None else (arrays + [opacity], len(opacity))
    ctx = _abi.Context.get()
    bufs = [ctx.from_host(cover), ctx.from_host(paints)] + [ctx.from_host(a) if a.size else None for a in ins]
    bufs.append(ctx.from_host(np.ascontiguousarray(grad_image)))
    shapes = ((n_paths, 4), (n_paths, 6), (n_paths, 4), (n_stops,), (n_stops, 4)) + (() if opacity is None else ((n_op,),))
    g_cover = ctx.alloc(cover.nbytes)
    outs = [ctx.alloc(int(np.prod(s)) * 8) if s[0] else None for s in shapes]   # (no stops, no opacities: no buffers for them)
    desc, _keep = _tier_desc(n_paths, rows, cols, _PLANES[cover.dtype], bg, origin, topo, n_stops, gtopo, n_groups, n_op)
    entry = getattr(ctx.lib, f"svgr_compose_{tier}_backward")
    _abi._check(entry(ctx.handle, C.byref(desc), *[_h(b) for b in bufs], g_cover.handle, *[_h(b) for b in outs]))
    got = [b.download(s, np.float64) if b is not None else np.zeros(s) for b, s in zip(outs, shapes)]
    return (g_cover.download(cover.shape, cover.dtype), got[0], GradientPaints(topo[0], topo[1], topo[2], *got[1:5]), *got[5:])


def compose_grouped(cover, paints, gp, groups, bg=None, origin=(0, 0), dtype=None):
    """``compose_painted`` with isolated groups: the ``(rows, cols, 4)`` premultiplied image of the program ``groups`` (a
    ``Groups``; ``group_program`` builds one from a tree of plane indices and ``Group``s) over the planes of ``cover``.  A fill
    paints its plane exactly as ``compose_painted`` paints a path; a group is painted on a transparent canvas, multiplied by its
    opacity (``Layer.opacity``), then by its clip's mask (the clip's planes composed OVER in one channel, then ``COMPOSE_IN``), and
    composed OVER the canvas below.  Every plane is used exactly once, by a fill or as a clip plane; the rows of ``paints`` and
    ``gp`` of a clip plane are ignored.  Groups nest at most ``group_depth()`` deep.  A program without groups gives
    ``compose_painted``'s bits.  Everything ``compose_painted`` refuses, non-finite opacities and every error of the program are
    refused before any device work."""
    return _tier_forward("grouped", cover, paints, gp, groups, bg, origin, dtype)


def compose_grouped_backward(cover, paints, gp, groups, grad_image, bg=None, origin=(0, 0)):
    """``(grad_cover, grad_paints, grad_gp, grad_opacity)``: the derivative of
    ``sum(grad_image * compose_grouped(cover, paints, gp, groups, bg, origin))``.

    ``grad_cover`` has ``cover``'s shape and type and holds the clip planes' derivatives too: a clip's outline moves through them.
    ``grad_paints`` and ``grad_gp`` are ``compose_painted_backward``'s (the rows of clip planes are 0); ``grad_opacity`` is float64
    ``(n_opacities,)``.  Nothing is divided: an opacity or a mask of 0, an opaque and an empty group are ordinary values.  No
    atomics: the same bits on every run."""
    return _tier_backward("grouped", cover, paints, gp, groups, grad_image, bg, origin)


@functools.lru_cache(maxsize=None)
def _tier_function(torch, tier):
    """The ``torch.autograd.Function`` of a tier, one class per tier: ComposePainted, ComposeGrouped, ComposeMasked."""
    def description(kept, plane, static):   # static: (bg, origin, topo) and, with a program, (gtopo, n_groups)
        n_paths, rows, cols = (int(v) for v in kept[0].shape)
        return _tier_desc(n_paths, rows, cols, plane, *static[:3], int(kept[4].shape[0]), *static[3:], *(int(t.shape[0]) for t in kept[6:]))

    class ComposeTier(torch.autograd.Function):
        """image = ComposeTier.apply(out, static, planes, paints, m6, geom, stop_pos, stop_rgba[, opacity])."""

        @staticmethod
        def forward(fn, out, static, *tensors):
            ctx = _context(torch)
            planes = tensors[0]
            plane = _abi.COVER_F64 if planes.dtype == torch.float64 else _abi.COVER_F32
            kept = tuple(t.detach().contiguous() for t in tensors)
            image = out if out is not None else torch.empty((*planes.shape[1:], 4), dtype=planes.dtype, device=planes.device)
            desc, _keep = description(kept, plane, static)
            with _Ordered(ctx, torch):
                b = _buffers(ctx, torch, *kept, image)
                _abi._check(getattr(ctx.lib, f"svgr_compose_{tier}_forward")(ctx.handle, C.byref(desc), *[_h(x) for x in b]))
            fn.save_for_backward(*kept)
            fn.tier_args = (plane, static)
            if out is not None:
                fn.mark_dirty(out)
            return image

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(fn, grad):
            kept = fn.saved_tensors
            ctx = _context(torch)
            grad = grad.contiguous()
            if grad.data_ptr() % 16:
                grad = grad.clone(memory_format=torch.contiguous_format)
            grads = tuple(torch.empty_like(t) for t in kept)
            desc, _keep = description(kept, *fn.tier_args)
            with _Ordered(ctx, torch):
                b = _buffers(ctx, torch, *kept, grad, *grads)
                _abi._check(getattr(ctx.lib, f"svgr_compose_{tier}_backward")(ctx.handle, C.byref(desc), *[_h(x) for x in b]))
            need = fn.needs_input_grad[2:]
            return (None, None) + tuple(g if need[i] else None for i, g in enumerate(grads))

    ComposeTier.__name__ = ComposeTier.__qualname__ = f"Compose{tier.capitalize()}"
    return ComposeTier


def compose_grouped_tensor(planes, paints_t, gp_t, groups, opacity_t, *, bg=None, origin=(0, 0), out=None):
    """``compose_grouped`` as a ``torch.autograd.Function``, whose backward is ``compose_grouped_backward``.

    ``planes``, ``paints_t`` and ``gp_t`` are ``compose_painted_tensor``'s; ``groups`` is a ``Groups`` whose topology (``items``,
    ``clip_off``, ``clip_planes``) stays on the host and whose ``opacity`` field is not looked at: the opacities are ``opacity_t``,
    a float64 ``(n_opacities,)`` CUDA tensor.  Any of the seven tensors may require grad.  ``bg``, ``origin``, ``out``, the stream
    ordering and the import-order rule (``tensor.IMPORT_ORDER``) are ``compose_painted_tensor``'s.  Only the program, shapes, dtypes
    and devices are checked: there is no host wait, so the VALUES are not looked at."""
    return _program_tensor("grouped", planes, paints_t, gp_t, groups, opacity_t, bg, origin, out)


def _program_tensor(tier, planes, paints_t, gp_t, groups, opacity_t, bg, origin, out):
    """``compose_grouped_tensor`` or ``compose_masked_tensor``: the checks, then the tier's ``torch.autograd.Function``."""
    torch = _torch()
    named, n_stops = _tensor_args(torch, planes, paints_t, gp_t, (groups, opacity_t))
    n_paths, rows, cols = (int(v) for v in planes.shape)
    topo = _painted_topology(gp_t, n_paths, n_stops)
    gtopo, n_groups = _PROGRAM_TOPOLOGY[tier](groups, n_paths, int(opacity_t.shape[0]))
    _n_pixels(max(n_paths, n_groups), (0, 0, rows, cols))
    bg, origin = _compose_bg(bg), _origin(origin)
    _tensor_places(torch, named, planes, out)
    return _tier_function(torch, tier).apply(out, (bg, origin, topo, gtopo, n_groups), *(t for _n, t, _k in named))


def render_grouped_tensor(segs, m6, paints, gp, opacity, *, groups, kinds, path_seg_off, rules, viewport, bg=None, dtype=None, check: bool = False,
                          flatness: float = FLATNESS):
    """Geometry, colours, gradients and groups to a ``(rows, cols, 4)`` premultiplied image and back: ``coverage_tensor`` followed
    by ``compose_grouped_tensor`` with ``origin`` from ``viewport``, with gradients to ``segs`` (a clip's outline included), ``m6``,
    ``paints``, the four tensors of ``gp`` and ``opacity``.  The arguments are theirs."""
    vp = _viewport(viewport)
    planes = coverage_tensor(segs, m6, kinds=kinds, path_seg_off=path_seg_off, rules=rules, viewport=vp, dtype=dtype, check=check, flatness=flatness)
    return compose_grouped_tensor(planes, paints, gp, groups, opacity, bg=bg, origin=(vp[0], vp[1]))


# ------------------------------------------------------------------------------------------------------------------------------
# luminance masks: masked groups in the compositor (svgr_compose_masked_forward / _backward, csrc/svgr_mask.h)
# ------------------------------------------------------------------------------------------------------------------------------
OP_HOLD, OP_END_MASK = 3, 4


def mask_program(tree):
    """``group_program`` for a tree whose ``Group``s may have a ``mask``: the same ``Groups``, with items that may hold
    ``{3, index of its BEGIN, opacity slot or -1, clip or -1}`` (HOLD: closes a masked group and keeps it) and
    ``{4, index of its BEGIN, 0, 0}`` (END_MASK: closes the mask's group, which follows the HOLD at once, and composes the held
    group through it); a BEGIN names its closer, whichever of the three it is.  A tree without masks gives ``group_program``'s
    items.  The program goes to ``compose_masked``, not to ``compose_grouped``."""
    items, clip_off, clip_planes, opacity = [], [0], [], []

    def walk(children):
        if isinstance(children, (Group, int, np.integer)) or not hasattr(children, "__iter__"):
            raise TypeError("a tree is a list of plane indices and Groups")
        for child in children:
            if isinstance(child, Group):
                begin = len(items)
                items.append([OP_BEGIN, -1, 0, 0])
                walk(child.children)
                slot = clip = -1
                if child.opacity is not None:
                    slot = len(opacity)
                    opacity.append(float(child.opacity))
                if child.clip is not None:
                    if len(child.clip) == 0:
                        raise ValueError("a clip has at least one plane")
                    clip = len(clip_off) - 1
                    clip_planes.extend(int(p) for p in child.clip)
                    clip_off.append(len(clip_planes))
                items[begin][1] = len(items)
                items.append([OP_END if child.mask is None else OP_HOLD, begin, slot, clip])
                if child.mask is not None:
                    begin = len(items)
                    items.append([OP_BEGIN, -1, 0, 0])
                    walk(child.mask)
                    items[begin][1] = len(items)
                    items.append([OP_END_MASK, begin, 0, 0])
            elif isinstance(child, (int, np.integer)) and not isinstance(child, bool):
                items.append([OP_FILL, int(child), 0, 0])
            else:
                raise TypeError(f"a tree holds plane indices and Groups, not {type(child).__name__}")

    walk(tree)
    return Groups(np.array(items, dtype=np.int32).reshape(-1, 4), np.array(clip_off, dtype=np.int32), np.array(clip_planes, dtype=np.int32),
                  np.array(opacity, dtype=np.float64))


def _mask_topology(groups, n_paths, n_opacities):
    """``_group_topology`` for a program that may hold masked pairs, checked as svgr_compose_masked_forward checks it."""
    items, clip_off, clip_planes = _program_tables(groups)
    depth_max = group_depth()
    planes, slots, clips = np.zeros(n_paths, dtype=np.int64), np.zeros(n_opacities, dtype=np.int64), {}
    stack, n_groups = [], 0   # the stack holds (index of the BEGIN, op of the closer it names)
    rows = items.tolist()
    for i, (op, a, slot, clip) in enumerate(rows):
        if op == OP_FILL:
            if not 0 <= a < n_paths:
                raise ValueError(f"item {i}: FILL of plane {a}, not one of {n_paths}")
            planes[a] += 1
        elif op == OP_BEGIN:
            if not i < a < len(rows) or rows[a][0] not in (OP_END, OP_HOLD, OP_END_MASK) or rows[a][1] != i:
                raise ValueError(f"item {i}: BEGIN without its closer (an END, a HOLD or an END_MASK)")
            closer, after_hold = rows[a][0], i > 0 and rows[i - 1][0] == OP_HOLD
            if closer == OP_END_MASK and not after_hold:
                raise ValueError(f"item {i}: the BEGIN of an END_MASK does not follow a HOLD")
            if closer != OP_END_MASK and after_hold:
                raise ValueError(f"item {i}: a HOLD is followed by the BEGIN of its mask's group, closed by END_MASK")
            if closer == OP_HOLD and (a + 1 >= len(rows) or rows[a + 1][0] != OP_BEGIN):
                raise ValueError(f"item {a}: a HOLD is followed by the BEGIN of its mask's group and is never the last item")
            if len(stack) == depth_max:
                raise ValueError(f"item {i}: groups nest deeper than {depth_max}")
            stack.append((i, closer))
            n_groups += 1
        elif op in (OP_END, OP_HOLD, OP_END_MASK):
            if not stack or stack[-1][0] != a:
                raise ValueError(f"item {i}: {('END', 'HOLD', 'END_MASK')[op - OP_END]} does not close the open group")
            if stack[-1][1] != op:
                raise ValueError(f"item {i}: the group is closed by another op than its BEGIN names")
            stack.pop()
            if op == OP_END_MASK:
                continue
            if op == OP_HOLD and i + 1 >= len(rows):
                raise ValueError(f"item {i}: a HOLD is never the last item")
            if slot != -1:
                if not 0 <= slot < n_opacities:
                    raise ValueError(f"item {i}: opacity slot {slot}, not one of {n_opacities}")
                slots[slot] += 1
            if clip != -1:
                if clip < 0 or clip in clips:
                    raise ValueError(f"item {i}: clip {clip} is negative or used twice")
                clips[clip] = i
        else:
            raise ValueError(f"item {i}: unknown op {op} (0 FILL, 1 BEGIN, 2 END, 3 HOLD, 4 END_MASK)")
    if stack:
        raise ValueError(f"item {stack[-1][0]}: the group is not closed")
    return _program_uses(items, clip_off, clip_planes, planes, slots, clips), n_groups


_PROGRAM_TOPOLOGY = {"grouped": _group_topology, "masked": _mask_topology}   # the host check of a tier's program


def compose_masked(cover, paints, gp, groups, bg=None, origin=(0, 0), dtype=None):
    """``compose_grouped`` with luminance masks: ``groups`` is a ``mask_program``.  A masked group is painted, multiplied by its
    opacity and its clip as in ``compose_grouped``, and then by its mask's value: the mask's own group (fills, gradients, groups,
    masked groups) painted on a transparent canvas and reduced per pixel to the luminance of its straight colour times its alpha,
    as ``Layer.luminance_mask`` does (divided where alpha > 1e-4, all four channels clipped to [0, 1],
    ``0.2125 r + 0.7154 g + 0.072 b``).  The mask's group counts as a group: towards ``group_depth()`` and in the limits.  A
    program without masks gives ``compose_grouped``'s bits.  Everything ``compose_grouped`` refuses and every wrong pairing of
    HOLD and END_MASK are refused before any device work."""
    return _tier_forward("masked", cover, paints, gp, groups, bg, origin, dtype)


def compose_masked_backward(cover, paints, gp, groups, grad_image, bg=None, origin=(0, 0)):
    """``(grad_cover, grad_paints, grad_gp, grad_opacity)`` of ``compose_masked``, in ``compose_grouped_backward``'s form: a mask
    has no parameter of its own; its gradient reaches the planes, paints and gradient descriptions of the fills inside it.

    The mask's value has kinks, and the derivative takes one documented side at each (csrc/svgr_mask.h): the alpha threshold
    takes the forward's branch, a clip to [0, 1] passes the gradient at 0 and at 1 (an opaque white mask still moves its paint).
    The only division is by an alpha above 1e-4: every finite input, a mask canvas of 0 included, gives finite gradients.  No
    atomics: the same bits on every run."""
    return _tier_backward("masked", cover, paints, gp, groups, grad_image, bg, origin)


def compose_masked_tensor(planes, paints_t, gp_t, groups, opacity_t, *, bg=None, origin=(0, 0), out=None):
    """``compose_masked`` as a ``torch.autograd.Function``, whose backward is ``compose_masked_backward``: the arguments, the
    checks (the program, shapes, dtypes and devices, never the values), ``out``, the stream ordering and the import-order rule are
    ``compose_grouped_tensor``'s; ``groups`` is a ``mask_program``."""
    return _program_tensor("masked", planes, paints_t, gp_t, groups, opacity_t, bg, origin, out)


def render_masked_tensor(segs, m6, paints, gp, opacity, *, groups, kinds, path_seg_off, rules, viewport, bg=None, dtype=None, check: bool = False,
                         flatness: float = FLATNESS):
    """``render_grouped_tensor`` through ``compose_masked_tensor``: gradients reach the outlines, paints and gradient descriptions
    of the fills inside a mask too.  The arguments are theirs; ``groups`` is a ``mask_program``."""
    vp = _viewport(viewport)
    planes = coverage_tensor(segs, m6, kinds=kinds, path_seg_off=path_seg_off, rules=rules, viewport=vp, dtype=dtype, check=check, flatness=flatness)
    return compose_masked_tensor(planes, paints, gp, groups, opacity, bg=bg, origin=(vp[0], vp[1]))


# ------------------------------------------------------------------------------------------------------------------------------
# from a Scene to the differentiable inputs
# ------------------------------------------------------------------------------------------------------------------------------
class LoweredScene(NamedTuple):
    """What ``lower_scene`` makes of a ``Scene``: the inputs of ``coverage`` (``segs``, ``kinds``, ``path_seg_off``, ``rules``,
    ``m6``: one plane per fill, stroke outline and clip path, every node's own transforms baked into ``segs``, the render
    transform in every row of ``m6``), of ``compose_grouped`` (``paints``, ``gp``, ``groups``) and ``sources``: per plane
    ``(role, Path)`` with ``role`` "fill", "stroke", "clip" or, for a fill or stroke inside a mask's scene, "mask", and the node's
    own path (a STROKE node's centre line, not its outline).  With ``masks=True`` ``groups`` is a ``mask_program`` and goes to
    ``compose_masked``."""

    segs: object
    kinds: object
    path_seg_off: object
    rules: object
    m6: object
    paints: object
    gp: object
    groups: object
    sources: object


_NODE_NAMES = ("FILL", "STROKE", "GROUP", "OPACITY", "CLIP", "MASK", "TRANSFORM", "FILTER", "BLEND", "MARKERS")


def lower_scene(scene, transform=None, linear_rgb: bool = False, *, masks: bool = False):
    """The ``LoweredScene`` of ``scene`` drawn under the render transform ``transform`` (identity by default): what
    ``svg_scene_from_filepath`` returns, as the arrays the differentiable route takes.  Host only, apart from the expansion lazy
    nodes (markers, text) and dashed strokes do themselves.

    FILL is a plane under its rule.  STROKE is a nonzero plane of ``path.stroke(...)``'s outline: a gradient reaches the outline's
    points, not the width, the joins or the centre line.  TRANSFORM is baked into the segments (``Path.transform``).  A plain GROUP
    is flattened into its parent: source-over is associative, so the pixels differ from the renderer's separately composited
    group by roundings only (a few units in the last place), not in what is drawn.  OPACITY is a group with an opacity, CLIP a
    group with a clip whose planes are the clip scene's fills (FILL, GROUP and TRANSFORM nodes; the planes come before the
    target's); an OPACITY that is the CLIP's direct target shares its level, any other order takes two.  A clip whose scene has no
    fill hides its target, as in the renderer: neither gets a plane.  Solid paints are converted as the renderer converts them
    (``solid_paint``), gradients go through ``gradient_paints`` under the accumulated transform.

    With ``masks=True`` a MASK is a masked group (``Group(..., mask=...)``) and the returned ``groups`` is a ``mask_program`` for
    ``compose_masked``, which is why the keyword is explicit.  The mask's scene is lowered like any other, so it may hold fills,
    strokes, gradients, opacities, clips and masks; its planes come after its target's and have the role "mask".  A CLIP that is
    the MASK's direct target shares its level, and so does an OPACITY directly under that CLIP; any other order takes a level
    more, and the mask's own group counts towards ``group_depth()`` like its target.  A mask scene that draws nothing hides its
    target, as in the renderer: neither gets a plane; a target that draws nothing is dropped with its mask.

    Refused with a ``ValueError`` that names the node, nothing is dropped silently: ``bbox_units=True`` on a CLIP, a MASK or a
    gradient, MASK nodes without ``masks=True``, FILTER and BLEND nodes, pattern and image paints, what ``gradient_paints`` refuses, a CLIP or anything but FILL, GROUP
    and TRANSFORM inside a clip's scene, groups nested deeper than ``group_depth()``, and a scene that draws nothing."""
    from .geometry import _RULES, Transform, solid_paint  # noqa: PLC0415
    from .paint import is_gradient  # noqa: PLC0415
    from .scene import (RENDER_BLEND, RENDER_CLIP, RENDER_FILL, RENDER_FILTER, RENDER_GROUP, RENDER_MARKERS, RENDER_MASK, RENDER_OPACITY,  # noqa: PLC0415
                        RENDER_STROKE, RENDER_TRANSFORM, Scene, _expanded, _stroked)

    if not isinstance(scene, Scene):
        raise TypeError(f"scene is a Scene, not {type(scene).__name__}")
    render = transform if transform is not None else Transform()
    depth_max = group_depth()
    planes = []   # (path with the node's transforms applied, rule, paint, accumulated transform, role, source)
    in_mask = [0]   # how many mask scenes the walk is inside

    def refuse(kind, why):
        raise ValueError(f"{_NODE_NAMES[kind]} node: {why}")

    def plane(path, acc, rule, role, source, paint):
        if rule not in _RULES:
            raise ValueError(f"{role.upper()} node: invalid fill rule: {rule}")
        planes.append((path.transform(acc), _RULES[rule], paint, acc, role, source))
        return len(planes) - 1

    def clip_planes(node, acc, out):
        if node[0] == RENDER_MARKERS:
            node = _expanded(node)
            if node is None:
                return
        kind, args = node
        if kind == RENDER_FILL:
            out.append(plane(args[0], acc, args[2], "clip", args[0], None))
        elif kind == RENDER_GROUP:
            for child in args:
                clip_planes(child, acc, out)
        elif kind == RENDER_TRANSFORM:
            clip_planes(args[0], acc @ args[1], out)
        elif kind == RENDER_CLIP:
            refuse(kind, "a clip inside a clip's scene is not supported")
        else:
            refuse(kind, "a clip's scene holds FILL, GROUP and TRANSFORM nodes")

    def walk(node, acc, out, depth):
        if node[0] == RENDER_MARKERS:
            node = _expanded(node)
            if node is None:
                return
        kind, args = node
        if kind == RENDER_FILL or kind == RENDER_STROKE:
            paint = args[1]
            if paint is None:   # (the renderer draws nothing)
                return
            if not is_gradient(paint) and not (isinstance(paint, np.ndarray) and paint.shape == (4,)):
                refuse(kind, f"a {type(paint).__name__} paint is not supported: solid colours and gradients are")
            if is_gradient(paint) and paint.bbox_units:
                refuse(kind, "a gradient in objectBoundingBox units (bbox_units=True) is not supported")
            if kind == RENDER_FILL:
                out.append(plane(args[0], acc, args[2], "mask" if in_mask[0] else "fill", args[0], paint))
            else:
                out.append(plane(_stroked(node), acc, None, "mask" if in_mask[0] else "stroke", args[0], paint))
        elif kind == RENDER_GROUP:
            for child in args:
                walk(child, acc, out, depth)
        elif kind == RENDER_TRANSFORM:
            walk(args[0], acc @ args[1], out, depth)
        elif kind == RENDER_OPACITY or kind == RENDER_CLIP or (kind == RENDER_MASK and masks):
            if depth == depth_max:
                refuse(kind, f"groups nest deeper than {depth_max}")
            first = len(planes)
            mask_scene = None
            if kind == RENDER_MASK:
                if args[2]:
                    refuse(kind, "a mask in objectBoundingBox units (bbox_units=True) is not supported")
                mask_scene, node = args[1], args[0]
            clip = None
            if node[0] == RENDER_CLIP:   # (the node itself, or the direct target of the MASK: one level)
                if node[1][2]:
                    refuse(RENDER_CLIP, "a clip in objectBoundingBox units (bbox_units=True) is not supported")
                clip = []
                clip_planes(node[1][1], acc, clip)
                if not clip:   # (the renderer draws nothing)
                    return
                node = node[1][0]
            opacity = None
            if node[0] == RENDER_OPACITY and (kind == RENDER_OPACITY or clip is not None):   # (the node itself, or the direct target of the CLIP: one level)
                opacity, node = float(node[1][1]), node[1][0]
            group = Group([], opacity, clip)
            drawn = len(planes)
            walk(node, acc, group.children, depth + 1)
            if mask_scene is not None:
                if len(planes) == drawn:   # (the target draws nothing: it goes with its mask)
                    del planes[first:]
                    return
                drawn, group.mask = len(planes), []
                in_mask[0] += 1
                walk(mask_scene, acc, group.mask, depth + 1)
                in_mask[0] -= 1
                if len(planes) == drawn:   # (the mask draws nothing: the renderer draws nothing)
                    del planes[first:]
                    return
            out.append(group)
        elif kind == RENDER_MASK:
            refuse(kind, "not supported by the differentiable route without masks: pass masks=True")
        elif kind in (RENDER_FILTER, RENDER_BLEND):
            refuse(kind, "not supported by the differentiable route")
        else:
            raise ValueError(f"unhandled scene type: {kind}")

    tree: list = []
    walk(scene, Transform(), tree, 0)
    if not planes:
        raise ValueError("the scene draws nothing: no plane")
    packed = [p[0].packed() for p in planes]
    segs = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 8) for s, _k in packed])
    kinds = np.concatenate([np.asarray(k, dtype=np.uint8).reshape(-1) for _s, k in packed])
    off = np.concatenate([[0], np.cumsum([len(k) for _s, k in packed])]).astype(np.int32)
    parts, rows = [], []
    for i, (_path, _rule, paint, acc, role, _source) in enumerate(planes):
        if role == "clip":
            paint = np.zeros(4)
        elif not is_gradient(paint):
            paint = solid_paint(paint, linear_rgb)
        try:
            gp, row = gradient_paints([paint], render @ acc, linear_rgb)
        except ValueError as e:
            raise ValueError(f"{role.upper()} node (plane {i}): {e}") from None
        parts.append(gp)
        rows.append(row)
    stop_off = np.concatenate([[0], np.cumsum([len(g.stop_pos) for g in parts])]).astype(np.int32)
    gp = GradientPaints(np.concatenate([g.kind for g in parts]), np.concatenate([g.spread for g in parts]), stop_off,
                        np.concatenate([g.m6 for g in parts]), np.concatenate([g.geom for g in parts]), np.concatenate([g.stop_pos for g in parts]),
                        np.concatenate([g.stop_rgba for g in parts]).reshape(-1, 4))
    m6 = np.tile(np.asarray(render.m6(), dtype=np.float64), (len(planes), 1))
    return LoweredScene(segs, kinds, off, np.array([p[1] for p in planes], dtype=np.uint8), m6, np.concatenate(rows), gp,
                        mask_program(tree) if masks else group_program(tree),
                        tuple((p[4], p[5]) for p in planes))
