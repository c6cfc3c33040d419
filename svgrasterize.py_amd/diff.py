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
"""
from __future__ import annotations

import ctypes as C
import functools

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
