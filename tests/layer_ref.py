"""Plain host references for the per-node layer operations and the blur convolution, one function per operation, each written
from the operation's definition (the reference's formulas, cited by their source lines S:...) in numpy long double -- not from
the kernels' text.  Images are (rows, cols, channels) arrays, boxes are (row0, col0, rows, cols) like the C ABI's.

Every function returns `(want, tol)`: the value in long double (or in the output's own type where the result is a selection,
a copy or a single rounding) and the largest distance a correct double implementation may have from it, as an array, a scalar,
or 0 for "bit for bit".  `assert_within(got, want, tol)` is the comparison: NaNs by position, everything else by distance.

The tolerances are derived, not tuned:

* selection and copy results (crop4, morphology, clip01, over with first = 1, to-float32, to-RGBA8, scale) are exact: the
  result is one of the inputs, a constant, or ONE correctly rounded operation of IEEE doubles, which numpy reproduces.
* short arithmetic (over, in, blend, background, colour matrix, luminance): a formula evaluated in doubles with r roundings
  is within r * u * T of its exact value to first order, where u = 2**-53 is the unit round-off and T the sum of the
  magnitudes of the formula's terms (every rounding is relative to a partial result no larger than T).  The bound used is
  (r + 1) * u * T: the extra unit covers the second-order terms and the reference's own 2**-64.  r is counted WITHOUT
  contraction; a compiler that contracts a * b + c into an fma only removes roundings, so the bound holds both ways.
  At unit magnitude the loosest of them (arithmetic blend: r = 7, four terms) is 8 * 2**-53 * 4 = 3.6e-15, inside the 1e-14
  the known-answer tests use for these operations.
* convolution: per output value 2**-52 * max|x| * [(kw + kh + 4) * sum|K| + 8 * kw * kh * max|K|] -- the fma chains of the
  two passes (kh and kw roundings, 4 more for the rounded row sums, column sums, total and their quotient, each relative
  to at most sum|K| * max|x|, at 2 u apiece), plus the allowance under which the library treats a kernel as rank 1
  (|K - u v^T / S| <= 8 * 2**-52 * max|K| per tap, as documented at its kernel analysis); the second term is dropped
  (`rank1=False`) for kernels that are not rank 1, which are summed as given.
* convert with a power (sRGB <-> linear): 1e-14 absolute on values in [0, 1], the project's own figure for its pow; the
  reference side is evaluated in long double (powl), whose error is 1e-19.  Without a power: short arithmetic.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53   # unit round-off of a double

COMPOSE_OUT, COMPOSE_ATOP, COMPOSE_XOR, COMPOSE_ARITHMETIC = 1, 3, 4, 5
PRE_TO_STRAIGHT, SRGB_TO_LINEAR, LINEAR_TO_SRGB, STRAIGHT_TO_PRE = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------ comparison
def assert_within(got, want, tol, what=""):
    """NaNs of `got` exactly where `want` has them; elsewhere |got - want| <= tol (tol 0: equal values AND equal sign bits)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: {int((gn != wn).sum())} NaN positions differ (got {int(gn.sum())}, want {int(wn.sum())})"
    ok = ~wn
    g, w = got[ok].astype(LD), want[ok].astype(LD)
    with np.errstate(invalid="ignore"):
        err = np.where(g == w, 0, np.abs(g - w))   # (equal infinities are no error)
    t = np.broadcast_to(np.asarray(tol, dtype=LD), want.shape)[ok]
    bad = err > t
    if bad.any():
        i = int(np.argmax(err - t))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values beyond their bound; worst |err| {float(err[i]):.3e} against "
                             f"{float(t[i]):.3e} (got {float(g[i])!r}, want {float(w[i])!r}); max |err| {float(err.max()):.3e}")
    if np.all(np.asarray(tol) == 0):
        assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), f"{what}: a zero differs in sign"


def max_err(got, want):
    ok = ~(np.isnan(want) | np.isnan(got))
    return float(np.abs(np.asarray(got)[ok].astype(LD) - np.asarray(want)[ok].astype(LD)).max(initial=0.0))


def _rgba(px, ch):
    """A source pixel block as 4 channels: a single channel is alpha and is broadcast (S:283-286)."""
    return px if ch == 4 else np.broadcast_to(px, px.shape[:-1] + (4,))


def _overlap(ob, sb):
    """The part of box `sb` inside box `ob`: (slices into the `ob` image, slices into the `sb` image), or None."""
    r0, r1 = max(ob[0], sb[0]), min(ob[0] + ob[2], sb[0] + sb[2])
    c0, c1 = max(ob[1], sb[1]), min(ob[1] + ob[3], sb[1] + sb[3])
    if r0 >= r1 or c0 >= c1:
        return None
    return ((slice(r0 - ob[0], r1 - ob[0]), slice(c0 - ob[1], c1 - ob[1])), (slice(r0 - sb[0], r1 - sb[0]), slice(c0 - sb[1], c1 - sb[1])))


# ------------------------------------------------------------------------------------------ convolution (S:106-118)
def convolve(img, kernel, rank1=True):
    """Full 2-D convolution of (rows, cols, ch) with the (kw, kh) kernel exactly as given:
    out[R, C] = sum_ij K[i, j] * img[R - i, C - j], shape (rows + kw - 1, cols + kh - 1, ch).
    tol: see the module text; `rank1=False` for a kernel built not to be rank 1."""
    img = np.asarray(img)
    k = np.asarray(kernel, dtype=np.float64)
    rows, cols, ch = img.shape
    kw, kh = k.shape
    x, kl = img.astype(LD), k.astype(LD)
    out = np.zeros((rows + kw - 1, cols + kh - 1, ch), dtype=LD)
    if kw * kh <= rows * cols:   # (one pass per tap, or one per source pixel: whichever is fewer)
        for i in range(kw):
            for j in range(kh):
                out[i:i + rows, j:j + cols] += kl[i, j] * x
    else:
        kk = kl[:, :, None]
        for r in range(rows):
            for c in range(cols):
                out[r:r + kw, c:c + kh] += kk * x[r, c]
    xmax = float(np.abs(img).max(initial=0.0))
    tol = 2.0 ** -52 * xmax * ((kw + kh + 4) * float(np.abs(k).sum()) + (8.0 * kw * kh * float(np.abs(k).max()) if rank1 else 0.0))
    return out, tol


def is_rank1(kernel):
    """The documented rule by which the library takes the two-pass routes: more than one tap on both axes, a finite non-zero
    total S, and |K - u v^T / S| <= 8 * 2**-52 * max|K| everywhere, u / v the row / column sums (in extended precision)."""
    k = np.asarray(kernel, dtype=np.float64)
    kl = k.astype(LD)
    u, v, s = kl.sum(1).astype(np.float64), kl.sum(0).astype(np.float64), float(kl.sum())
    if k.shape[0] < 2 or k.shape[1] < 2 or not np.isfinite(s) or s == 0.0:
        return False
    return bool((np.abs(k - np.outer(u, v) / s) <= 8 * 2.0 ** -52 * np.abs(k).max()).all())


# ------------------------------------------------------------------------------------------ Porter-Duff steps (S:277-298)
def over(dst, db, src, sb, first=False):
    """One step of canvas_merge_union(full=False) (S:366-377 + S:286): on the overlap dst = src + dst * (1 - src_alpha), or a
    copy of src when `first` (S:374-375); dst elsewhere untouched.  tol: copy exact; else r = 3 (1 - a, the product, the sum)
    -> 4 u (|src| + |dst (1 - a)|)."""
    out = np.asarray(dst).astype(LD)
    tol = np.zeros(out.shape)
    ov = _overlap(db, sb)
    if ov is not None:
        d_sl, s_sl = ov
        s = _rgba(np.asarray(src)[s_sl].astype(LD), src.shape[2])
        if first:
            out[d_sl] = s
        else:
            d = out[d_sl].copy()   # (what was there before this step: the bound is made from it)
            k = 1 - s[..., 3:]
            out[d_sl] = s + d * k
            tol[d_sl] = (4 * U * (np.abs(s) + np.abs(d * k))).astype(np.float64)
    return out, tol


def in_(dst, db, src, sb):
    """One step of canvas_merge_intersect (S:290): on the overlap dst = src * dst_alpha; elsewhere untouched.
    tol: r = 1 -> 2 u |src dst_alpha|."""
    out = np.asarray(dst).astype(LD)
    tol = np.zeros(out.shape)
    ov = _overlap(db, sb)
    if ov is not None:
        d_sl, s_sl = ov
        s = _rgba(np.asarray(src)[s_sl].astype(LD), src.shape[2])
        v = s * out[d_sl][..., 3:]
        out[d_sl] = v
        tol[d_sl] = (2 * U * np.abs(v)).astype(np.float64)
    return out, tol


def crop4(ob, src, sb):
    """The box `ob` cut out of the source (a single channel broadcast to four), zero outside it (S:382-416).  tol 0: copies."""
    out = np.zeros((ob[2], ob[3], 4), dtype=np.float64)
    ov = _overlap(ob, sb)
    if ov is not None:
        out[ov[0]] = _rgba(np.asarray(src)[ov[1]], src.shape[2])
    return out, 0


def blend(dst, db, src, sb, mode, k4=None):
    """The other canvas_compose modes on the whole of `dst` with the source zero-extended (S:287-297, S:348-361):
      1 OUT   src (1 - dst_a)                          r = 2 -> 3 u T
      3 ATOP  src dst_a + dst (1 - src_a)              r = 4 -> 5 u T
      4 XOR   src (1 - dst_a) + dst (1 - src_a)        r = 5 -> 6 u T
      5 arithmetic  clip(k1 src dst + k2 src + k3 dst + k4, 0, 1)   r = 7 (4 products, 3 sums) -> 8 u T; the clip moves no
        value further from the exact clipped one.
    T = the sum of the magnitudes of the formula's terms."""
    d = np.asarray(dst).astype(LD)
    s = np.zeros(d.shape, dtype=LD)
    ov = _overlap(db, sb)
    if ov is not None:
        s[ov[0]] = _rgba(np.asarray(src)[ov[1]].astype(LD), src.shape[2])
    da, sa = d[..., 3:], s[..., 3:]
    if mode == COMPOSE_OUT:
        terms, r = [s * (1 - da)], 2
    elif mode == COMPOSE_ATOP:
        terms, r = [s * da, d * (1 - sa)], 4
    elif mode == COMPOSE_XOR:
        terms, r = [s * (1 - da), d * (1 - sa)], 5
    elif mode == COMPOSE_ARITHMETIC:
        k1, k2, k3, k4_ = (LD(v) for v in k4)
        terms, r = [k1 * s * d, k2 * s, k3 * d, np.full(d.shape, k4_, dtype=LD)], 7
    else:
        raise ValueError(mode)
    out = sum(terms[1:], terms[0])
    tol = ((r + 1) * U * sum(np.abs(t) for t in terms)).astype(np.float64)
    if mode == COMPOSE_ARITHMETIC:
        out = np.clip(out, 0, 1)
    return out, tol


# ------------------------------------------------------------------------------------------ Layer.convert (S:129-164, S:471-503)
def convert(img, ops):
    """The four conversions in their order on RGBA pixels: 1 premultiplied -> straight (rgb / a where a > 1e-4, then all four
    clipped to [0, 1], S:471-477), 2 sRGB -> linear (S:496-503), 4 linear -> sRGB (S:486-493), 8 straight -> premultiplied
    (rgb * a, S:480-483).  tol: 1e-14 absolute with a power (values in [0, 1]); else one rounding per arithmetic op:
    (r + 1) u |value|, r = the number of ops 1 and 8 present."""
    v = np.asarray(img).astype(LD).copy()
    if ops & PRE_TO_STRAIGHT:
        a = v[..., 3:]
        rgb = np.where(a > LD(0.0001), v[..., :3] / np.where(a > LD(0.0001), a, 1), v[..., :3])
        v = np.clip(np.concatenate([rgb, a], axis=-1), 0, 1)
    if ops & SRGB_TO_LINEAR:
        c = v[..., :3]
        v[..., :3] = np.where(c <= LD(0.04045), c / LD(12.92), np.power(np.maximum((c + LD(0.055)) / LD(1.055), 0), LD(2.4)))
    if ops & LINEAR_TO_SRGB:
        c = v[..., :3]
        v[..., :3] = np.where(c <= LD(0.0031308), c * LD(12.92), LD(1.055) * np.power(np.maximum(c, 0), 1 / LD(2.4)) - LD(0.055))
    if ops & STRAIGHT_TO_PRE:
        v[..., :3] = v[..., :3] * v[..., 3:]
    if ops & (SRGB_TO_LINEAR | LINEAR_TO_SRGB):
        tol = 1e-14
    else:
        r = bool(ops & PRE_TO_STRAIGHT) + bool(ops & STRAIGHT_TO_PRE)
        tol = ((r + 1) * U * np.abs(v)).astype(np.float64) if r else 0
    return v, tol


def convert_ops(pre_from, lin_from, pre_to, lin_to):
    """The ops Layer.convert needs from one (pre_alpha, linear_rgb) state to another (S:129-164): a change of colour space is
    made on straight alpha."""
    ops, cur = 0, pre_from
    if lin_from != lin_to:
        if cur:
            ops, cur = ops | PRE_TO_STRAIGHT, False
        ops |= SRGB_TO_LINEAR if lin_to else LINEAR_TO_SRGB
    if cur != pre_to:
        ops |= STRAIGHT_TO_PRE if pre_to else PRE_TO_STRAIGHT
    return ops


# ------------------------------------------------------------------------------------------ N layers in one pass
def _union(boxes):
    r0, c0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    return (r0, c0, max(b[0] + b[2] for b in boxes) - r0, max(b[1] + b[3] for b in boxes) - c0)


def _intersection(boxes):
    r0, c0 = max(b[0] for b in boxes), max(b[1] for b in boxes)
    r1, c1 = min(b[0] + b[2] for b in boxes), min(b[1] + b[3] for b in boxes)
    return (r0, c0, r1 - r0, c1 - c0) if r1 > r0 and c1 > c0 else None


def compose_over(layers):
    """Layer.compose(layers, OVER) (S:177-207 -> canvas_merge_union, S:366-379): `layers` = [(image, box, ops), ...]; each
    source converted by its ops first, the union canvas zero, the first layer copied, the others OVER in their order.
    Returns (want, tol, union box).  tol per pixel, carried through the chain: a step's own 4 u T, what the step before left
    times |1 - a| (an error of dst is scaled like dst), and the source's conversion error e_s in src itself and in the factor
    (1 - a): e_s (1 + |dst|)."""
    ub = _union([b for _, b, _ in layers])
    out = np.zeros((ub[2], ub[3], 4), dtype=LD)
    tol = np.zeros(out.shape)
    for i, (img, sb, ops) in enumerate(layers):
        s_all, e_all = convert(img, ops) if ops else (np.asarray(img).astype(LD), 0)
        d_sl, s_sl = _overlap(ub, sb)
        s = _rgba(s_all[s_sl], img.shape[2])
        e = np.broadcast_to(np.asarray(e_all, dtype=np.float64), s_all.shape)[s_sl]
        e = _rgba(e, img.shape[2])
        if i == 0:
            out[d_sl], tol[d_sl] = s, e
            continue
        d, k = out[d_sl], 1 - s[..., 3:]
        tol[d_sl] = tol[d_sl] * np.abs(k).astype(np.float64) + e * (1 + np.abs(d)).astype(np.float64) + (4 * U * (np.abs(s) + np.abs(d * k))).astype(np.float64)
        out[d_sl] = s + d * k
    return out, tol, ub


def compose_in(layers):
    """Layer.compose(layers, IN) (canvas_merge_intersect, S:382-416 + S:290): on the intersection of the boxes, the first
    layer cropped (a single channel broadcast), then out = src * out_alpha for every other layer in order.
    Returns (want, tol, box).  tol carried through the chain: |src| times the error of out_alpha, |out_alpha| times the
    source's conversion error, and the product's own rounding at 2 u."""
    ib = _intersection([b for _, b, _ in layers])
    assert ib is not None
    out = tol = None
    for i, (img, sb, ops) in enumerate(layers):
        s_all, e_all = convert(img, ops) if ops else (np.asarray(img).astype(LD), 0)
        _, s_sl = _overlap(ib, sb)
        s = _rgba(s_all[s_sl], img.shape[2])
        e = _rgba(np.broadcast_to(np.asarray(e_all, dtype=np.float64), s_all.shape)[s_sl], img.shape[2])
        if i == 0:
            out, tol = s.copy(), e.copy()
            continue
        da = out[..., 3:]
        v = s * da
        tol = np.abs(s).astype(np.float64) * tol[..., 3:] + np.abs(da).astype(np.float64) * e + (2 * U * np.abs(v)).astype(np.float64)
        out = v
    return out, tol, ib


# ------------------------------------------------------------------------------------------ per-pixel operations
def color_matrix(img, m):
    """Layer.color_matrix (S:95-104): clip(px @ M[:, :4].T + M[:, 4], 0, 1), M the 4 x 5 matrix.
    tol: r = 8 (4 products, 4 sums; fused forms have fewer) -> 9 u (sum_k |x_k m_qk| + |m_q4|); the clip moves nothing further."""
    x, ml = np.asarray(img).astype(LD), np.asarray(m).astype(LD)
    out = x @ ml[:, :4].T + ml[:, 4]
    tol = (9 * U * (np.abs(x) @ np.abs(ml[:, :4]).T + np.abs(ml[:, 4]))).astype(np.float64)
    return np.clip(out, 0, 1), tol


def morphology(img, ky, kx, is_max):
    """Layer.morphology (S:120-127) = min / max pooling, window ky rows x kx columns, stride 1, no padding (S:419-468), NaNs
    skipped (a window of nothing but NaN gives NaN).  tol 0: every output is one of the inputs."""
    x = np.asarray(img)
    rows, cols = x.shape[:2]
    orows, ocols = rows - ky + 1, cols - kx + 1
    pick = np.fmax if is_max else np.fmin   # (fmax / fmin: the NaN operand loses)
    acc = np.full((orows, ocols, x.shape[2]), np.nan)
    for dy in range(ky):
        for dx in range(kx):
            acc = pick(acc, x[dy:dy + orows, dx:dx + ocols])
    return acc, 0


def luminance(img):
    """The luminance mask (S:735): (rgb @ [0.2125, 0.7154, 0.072]) * alpha of a straight-alpha layer, one channel.
    tol: r = 6 (3 products, 2 sums, the product with alpha) -> 7 u |alpha| sum_k |x_k w_k|."""
    x = np.asarray(img).astype(LD)
    w = np.array([0.2125, 0.7154, 0.072]).astype(LD)
    out = (x[..., :3] @ w) * x[..., 3]
    tol = (7 * U * (np.abs(x[..., :3]) @ np.abs(w)) * np.abs(x[..., 3])).astype(np.float64)
    return out, tol


def background(img, rgba):
    """Layer.background (S:166-169): the image OVER a constant colour, image + colour * (1 - alpha).
    tol: r = 3 -> 4 u (|image| + |colour (1 - alpha)|)."""
    x, c = np.asarray(img).astype(LD), np.asarray(rgba).astype(LD)
    t = c * (1 - x[..., 3:])
    return x + t, (4 * U * (np.abs(x) + np.abs(t))).astype(np.float64)


def clip01(x):
    """ndarray.clip(0, 1) (S:326): below 0 -> 0, above 1 -> 1, everything else -- NaN and -0.0 included -- as it is.  tol 0."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x)), 0


def scale(x, f):
    """Layer.opacity's product (S:171-175): x * f, a single correctly rounded product in double.  tol 0."""
    return np.asarray(x, dtype=np.float64) * np.float64(f), 0


def to_f32(x, clip):
    """double -> float32 (round to nearest even, subnormals kept), behind a clip to [0, 1] when asked.  tol 0."""
    x = np.asarray(x, dtype=np.float64)
    if clip:
        x = clip01(x)[0]
    with np.errstate(over="ignore", under="ignore"):
        return x.astype(np.float32), 0


def to_rgba8(x):
    """The output stage (canvas_to_png, S:262): np.round(x * 255.0) -- one product in double, rounded half to even --, values
    outside [0, 255] saturated, NaN -> 0.  tol 0."""
    r = np.round(np.asarray(x, dtype=np.float64) * 255.0)
    r = np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0))
    return r.astype(np.uint8), 0
