"""The filter primitives beyond the reference at the edges of their values, as data: feTurbulence coordinates at the powers of
two where an integer part stops fitting, feComponentTransfer at the ends of [0, 1] and with NaN or infinite pixels,
feConvolveMatrix with a NaN or infinite pixel under its kernel, the lighting primitives with a NaN surface and degenerate
lights, the parameters every entry refuses, and documents whose numbers are not finite.  Consumed on the CPU by
tests/test_filter_edges_host.py (the host build of csrc/svgr_core.h against the restatements, and alone under the
undefined-behaviour sanitizer) and on the device by tests/test_gpu_filter_edges.py.  Every layer is a few dozen pixels: every
edge here is per pixel.  Each case says which edge it is for (`edge`), and the host test asserts that it reaches it.

DESIGN.md "Filter primitives at the edges of their values" states the rules the cases pin."""
import math

import numpy as np

from tests import filter_ref as F
from tests import lighting_ref as LR

NAN, INF = float("nan"), float("inf")
NON_FINITE = (NAN, INF, -INF)


# ====================================================================================== feTurbulence
# A case is a (rows, cols) layer at `offset` under the transform translate(`translate`): pixel [R, C] is the user point
# (offset + (R, C) + 0.5 - translate), which is what Layer.turbulence evaluates and what fh_turbulence gets as points
# (`turb_points`).  The lattice coordinate of octave k is tx_k = 2^k px fx + 4096.  `at` = the pixel whose coordinate the case
# is about, `edge` = (kind, ...) as `turb_reaches` reads it.
TURB_SHAPE = (3, 5)
TURB_AT = (1, 2)
TURB_TILE = (-2.5, 1.75, 230.3, 310.9)
THRESHOLDS = {"2^31": 2.0 ** 31, "2^52": 2.0 ** 52, "2^53": 2.0 ** 53, "2^62": 2.0 ** 62, "2^63": 2.0 ** 63}
LAST_OCTAVES = 8   # "crossed at the last octave only": tx_7 at the threshold, tx_0 .. tx_6 at most half of it


def turb_transform(case):
    from svgrasterize_amd.geometry import Transform

    return Transform().translate(*case["translate"])


def turb_points(case):
    """(px, py), flat: the user points of the case's pixel centres, by the kernel's plain form of the inverse transform."""
    px, py = F.pixel_user_points(turb_transform(case).invert.m6(), case["offset"], case["shape"])
    return px.ravel(), py.ravel()


def _turb(name, freq, octaves, fractal, stitch, translate=(0.0, 0.0), offset=(0, 0), seed=5, edge=None, shape=TURB_SHAPE,
          tile=TURB_TILE):
    return dict(name=name, freq=(float(freq[0]), float(freq[1])), octaves=octaves, fractal=bool(fractal),
                tile=tuple(tile) if stitch else None, translate=(float(translate[0]), float(translate[1])), offset=tuple(offset),
                shape=tuple(shape), seed=seed, edge=edge)


def _tx_at(case, octave):
    px, _py = turb_points(case)
    at = TURB_AT[0] * case["shape"][1] + TURB_AT[1]
    return F.turbulence_trace(case["seed"], case["freq"], case["octaves"], case["tile"], px[at], 0.0)[octave][0]


def _straddle(make, x, threshold, octave):
    """Neighbouring doubles (lo, hi) of the free parameter (positive, and tx grows with it) around the estimate `x` with
    tx(lo) < threshold <= tx(hi): a bisection over the doubles between x (1 - 1e-6) and x (1 + 1e-6)."""
    def below(bits):
        return _tx_at(make(float(np.int64(bits).view(np.float64))), octave) < threshold

    lo, hi = (int(np.float64(v).view(np.int64)) for v in (x * (1.0 - 1e-6), x * (1.0 + 1e-6)))
    assert below(lo) and not below(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if below(mid) else (lo, mid)
    return tuple(float(np.int64(v).view(np.float64)) for v in (lo, hi))


def _threshold_cases():
    cases = []
    for label, T in THRESHOLDS.items():
        for octaves, where in ((1, "first"), (LAST_OCTAVES, "last")):
            octave = octaves - 1
            for fractal, stitch in ((True, False), (False, False), (True, True), (False, True)):
                if stitch:
                    # the tile fixes the frequency (0.06 adjusted), so the point moves: a translate of about -T / (2^k f)
                    def make(v, fractal=fractal, octaves=octaves):
                        return _turb("", (0.06, 0.045), octaves, fractal, True, translate=(-v, 3.0))

                    f = F.turbulence_params(0.06, 0.045, TURB_TILE, True)[0]
                    start = (T - 4096.0) / (f * 2.0 ** octave) - 1.5
                else:
                    # the point stays (pixel centre 1.5 of the row axis) and the frequency grows to about T / (2^k 1.5)
                    def make(v, fractal=fractal, octaves=octaves):
                        return _turb("", (v, 0.045), octaves, fractal, False)

                    start = (T - 4096.0) / (1.5 * 2.0 ** octave)
                lo, hi = _straddle(make, start, T, octave)
                for side, v in (("under", lo), ("over", hi)):
                    case = make(v)
                    case["name"] = f"tx_{side}_{label}_{where}_octave_{'fractal' if fractal else 'turbulence'}_{'stitch' if stitch else 'nostitch'}"
                    case["edge"] = ("threshold", T, octave, side)
                    cases.append(case)
    return cases


def _turbulence_cases():
    cases = []
    for fractal in (False, True):
        for stitch in (False, True):
            tag = f"{'fractal' if fractal else 'turbulence'}_{'stitch' if stitch else 'nostitch'}"
            for freq in ((0.0, 0.07), (0.07, 0.0), (0.0, 0.0)):
                cases.append(_turb(f"frequency_{freq[0]:g}_{freq[1]:g}_{tag}", freq, 3, fractal, stitch, edge=("frequency_zero",)))
            cases.append(_turb(f"octaves_0_{tag}", (0.06, 0.045), 0, fractal, stitch, edge=("octaves", 0)))
            cases.append(_turb(f"octaves_32_{tag}", (0.06, 0.045), 32, fractal, stitch, edge=("octaves", 32)))
            # user x about -70000: tx = -70000 * 0.06 + 4096 < 0, so the integer part is taken toward zero and the fraction is negative
            cases.append(_turb(f"below_minus_4096_{tag}", (0.06, 0.045), 2, fractal, stitch, translate=(70000.3, 100123.7),
                               edge=("negative",)))
            # pixel centres at integers (translate 0.5) and frequencies 1 and 0.25: tx is an integer at every pixel, ty at some
            cases.append(_turb(f"tx_integer_{tag}", (1.0, 0.25), 2, fractal, stitch, translate=(0.5, 0.5), tile=(0.0, 0.0, 16.0, 8.0),
                               edge=("integer",)))
        # finite numbers whose product is not: 1.5 * 1.7e308 overflows at the first octave, 1.5 * 1e305 * 2^k at the twelfth (k = 11);
        # with a stitch tile the frequency stays small and the point is far: 1e308 * 0.06 * 2^k overflows at k = 5
        cases.append(_turb(f"overflow_first_octave_{fractal}", (1.7e308, 0.045), 2, fractal, False, edge=("overflow", 0)))
        cases.append(_turb(f"overflow_later_octave_{fractal}", (1e305, 1e305), 16, fractal, False, edge=("overflow", 11)))
        cases.append(_turb(f"overflow_stitch_{fractal}", (0.06, 0.045), 8, fractal, True, translate=(-1e308, 3.0), edge=("overflow", 5)))
    for seed in (0, -1, 2 ** 31 - 1, 2 ** 31, -2 ** 40, 3.9):
        cases.append(_turb(f"seed_{seed}", (0.06, 0.045), 2, True, seed != 0, seed=seed, edge=("seed", seed)))
    # the stitch bound from its accepted side (the other side is among the refusals): 32 octaves, width_0 = wrap_0 - 4096 = 2^22 - 1
    cases.append(_turb("stitch_state_at_its_bound", (1.0, 1.0), 32, False, True, tile=(0.0, 0.0, 2.0 ** 22 - 1, 7.0),
                       edge=("stitch_bound",)))
    return cases + _threshold_cases()


# (tile, frequencies, octaves) around the bound  2^(octaves - 1) max(width_0, |wrap_0 - 4096|) + 4096 <= 2^53:  (what, accepted)
STITCH_BOUND = [
    (dict(freq=(1.0, 1.0), octaves=32, tile=(0.0, 0.0, 2.0 ** 22 - 1, 7.0)), True),     # 2^31 (2^22 - 1) + 4096 = 2^53 - 2^31 + 4096
    (dict(freq=(1.0, 1.0), octaves=32, tile=(0.0, 0.0, 2.0 ** 22, 7.0)), False),        # 2^31 2^22 + 4096 > 2^53
    (dict(freq=(1.0, 1.0), octaves=32, tile=(0.0, 0.0, 7.0, 2.0 ** 22)), False),        # the same on the other axis
    (dict(freq=(1.0, 1.0), octaves=1, tile=(2.0 ** 53 - 4104, 0.0, 7.0, 7.0)), True),    # one octave: wrap_0 = x + 4096 + 7 = 2^53 - 1
    (dict(freq=(1.0, 1.0), octaves=1, tile=(2.0 ** 53 - 4102, 0.0, 7.0, 7.0)), False),   # x + 4096 + 7 = 2^53 + 1 is not a double
    (dict(freq=(1.0, 1.0), octaves=32, tile=(2.0 ** 22, 0.0, 7.0, 7.0)), False),        # wrap_0 - 4096 = 2^22 + 7 from the tile's x
    (dict(freq=(1.0, 1.0), octaves=32, tile=(-2.0 ** 22 - 8, 0.0, 7.0, 7.0)), False),   # and from a negative x
    (dict(freq=(1.0, 1.0), octaves=32, tile=(2.0 ** 22 - 8, 0.0, 7.0, 7.0)), True),
    (dict(freq=(0.06, 0.045), octaves=32, tile=TURB_TILE), True),
    (dict(freq=(1e300, 1.0), octaves=1, tile=(0.0, 0.0, 1e300, 7.0)), False),           # tile.w f overflows
]


# ====================================================================================== feComponentTransfer
C_EDGES = [-0.0, 0.0, 2.0 ** -1074, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, NAN, INF, -INF]


def _long_table(n):
    k = np.arange(n, dtype=np.float64)
    return tuple(((k * 37.0) % 101.0) / 80.0 - 0.1)   # values in [-0.1, 1.1625], neighbours far apart


def _transfer_cases():
    cases = []

    def add(name, fn, extra=(), edge=None):
        cases.append(dict(name=name, fn=fn, c=np.array(C_EDGES + list(extra), dtype=np.float64), edge=edge))

    add("identity", None)
    for kind in ("table", "discrete"):
        add(f"{kind}_length_1", (kind, (0.7,)))
        add(f"{kind}_length_2", (kind, (0.2, 0.9)))
        add(f"{kind}_length_4096", (kind, _long_table(4096)), extra=[k / 4095.0 for k in (1, 2047, 4094)] + [0.37, 0.99999],
            edge=("length", 4096))
        add(f"{kind}_outside_0_1", (kind, (-0.5, 1.5, 0.25, 2.0, -3.0)), extra=[0.1, 0.3, 0.5, 0.7, 0.9], edge=("outside",))
    # c m (table, m = n - 1) and c n (discrete) exact integers: c = k / 4 and k / 8, with their neighbours
    knots = [k / 4.0 for k in range(1, 4)]
    near = [float(np.nextafter(c, d)) for c in knots for d in (0.0, 1.0)]
    add("table_on_its_knots", ("table", (0.1, 0.9, 0.3, 0.6, 0.2)), extra=knots + near, edge=("knots", 4))
    add("discrete_on_its_steps", ("discrete", (0.1, 0.9, 0.3, 0.6)), extra=knots + near, edge=("knots", 4))
    add("table_of_huge_values", ("table", (1e308, -1e308, 1e308)), extra=[0.25, 0.5, 0.75], edge=("nan_inside",))
    add("linear_identity", ("linear", 1.0, 0.0))
    add("linear_down", ("linear", -2.0, 1.5), extra=[0.25, 0.5, 0.75])
    add("linear_overflowing", ("linear", 1.7e308, 1.7e308), extra=[0.5], edge=("inf_inside",))
    add("linear_inf_minus_inf", ("linear", 1.7e308, -1.7e308), extra=[0.5])
    for amplitude, exponent in ((0.0, -1.0), (1.0, -1.0), (1.0, 0.0), (0.0, 0.0), (-1.0, 0.5)):
        add(f"gamma_{amplitude:g}_{exponent:g}", ("gamma", amplitude, exponent, 0.25), extra=[0.04, 0.5],
            edge=("nan_inside",) if (amplitude, exponent) == (0.0, -1.0) else None)
    return cases


# ====================================================================================== feConvolveMatrix
CM_SHAPE = (5, 7)
CM_KERNEL = np.array([[1.0, 2.0, 0.75], [0.5, 3.0, 1.0], [0.0, 0.25, 1.5]])   # (one weight is 0: 0 * NaN is still NaN)
CM_AT = (0, 6)   # the odd pixel: a corner, which `duplicate` repeats and `wrap` brings round to the other side


def _cm_image(preserve):
    rng = np.random.default_rng(20240611)
    img = rng.uniform(0.25, 0.75, CM_SHAPE + (4,))
    if not preserve:
        img[..., :3] *= img[..., 3:]
    return img


def _convolve_cases():
    cases = []

    def add(name, image, kernel, divisor, bias, edge_mode, preserve, target=None, edge=None):
        kernel = np.ascontiguousarray(kernel, dtype=np.float64)
        target = (kernel.shape[1] // 2, kernel.shape[0] // 2) if target is None else target
        cases.append(dict(name=name, image=image, kernel=kernel, divisor=float(divisor), bias=float(bias), target=target,
                          edge_mode=edge_mode, preserve=bool(preserve), edge=edge))

    for preserve in (False, True):
        for edge_mode in ("duplicate", "wrap", "none"):
            for label, value in (("nan", NAN), ("plus_inf", INF), ("minus_inf", -INF)):
                img = _cm_image(preserve)
                img[CM_AT][: 3 if preserve else 4] = value   # (preserveAlpha copies alpha: the odd pixel keeps a finite one)
                add(f"{label}_pixel_{edge_mode}_{'preserve' if preserve else 'premultiplied'}", img, CM_KERNEL, 2.0 * CM_KERNEL.sum(),
                    0.0, edge_mode, preserve, edge=("odd_pixel", label))
    img = _cm_image(True)
    img[1:4, 2:5, 3] = 0.0
    add("alpha_0_under_preserve_alpha", img, CM_KERNEL, CM_KERNEL.sum(), 0.0, "duplicate", True, edge=("alpha_zero",))
    half = np.full(CM_SHAPE + (4,), 0.5)
    for bias, what in ((-0.5, 0.0), (0.5, 1.0)):
        # nine weights of 1 over nine pixels of 0.5, divisor 9: 4.5 / 9 = 0.5 exactly, and the bias takes it to exactly 0 or 1
        add(f"bias_to_exactly_{what:g}", half, np.ones((3, 3)), 9.0, bias, "duplicate", False, edge=("exactly", what))
        add(f"bias_to_exactly_{what:g}_preserve", half, np.ones((3, 3)), 9.0, bias, "wrap", True, edge=("exactly", what))
    img = _cm_image(False)
    img[2, 1:6] = 0.0
    add("divisor_2_to_minus_1000", img, np.array([[1.0]]), 2.0 ** -1000, 0.0, "none", False, edge=("huge",))
    add("divisor_2_to_minus_1000_3x3", img, CM_KERNEL, -(2.0 ** -1000), 0.0, "none", True, edge=("huge",))
    return cases


# ====================================================================================== lighting
# A case: the region's alpha A (the source covers exactly the region, at `offset`), the light in the device frame (`params`, what
# the C ABI and the host build take) and as a light source (`light`, what Layer.lighting takes under the identity transform;
# LR.light_frame of it is `params` up to the rounding of the trigonometry), colour, surfaceScale, constant, `se` (None = diffuse).
L_OFFSET = (-2, 3)
L_COLOR = (0.9, 0.6, 1.0)


def _l_alpha(shape=(3, 3)):
    return np.random.default_rng(77).uniform(0.1, 0.9, shape)


def _lights():
    """name -> (kind, light): one of each kind, aimed at the 3 x 3 region at L_OFFSET."""
    return {
        "distant": (LR.DISTANT, (30.0, 50.0)),
        "point": (LR.POINT, (0.25, 5.75, 3.0)),
        "spot": (LR.SPOT, (0.25, 5.75, 3.0, -0.5, 4.5, 0.0, 2.0, 40.0)),
    }


def _identity():
    from svgrasterize_amd.geometry import Transform

    return Transform()


def _lighting_cases():
    cases = []

    def add(name, A, kind, light, ss=2.0, constant=0.9, se=None, params=None, offset=L_OFFSET, edge=None, color=L_COLOR):
        params = LR.light_frame(_identity(), kind, light) if params is None else np.asarray(params, dtype=np.float64)
        cases.append(dict(name=name, A=np.ascontiguousarray(A, dtype=np.float64), kind=kind, light=light, params=params,
                          color=color, ss=float(ss), constant=float(constant), se=se, offset=tuple(offset), edge=edge))

    for lname, (kind, light) in _lights().items():
        for se in (None, 7.0):
            tag = f"{lname}_{'diffuse' if se is None else 'specular'}"
            for label, value in (("nan", NAN), ("inf", INF), ("2", 2.0)):
                for where, at in (("centre", (1, 1)), ("neighbour", (0, 1))):
                    A = _l_alpha()
                    A[at] = value
                    add(f"alpha_{label}_at_the_{where}_{tag}", A, kind, light, se=se, edge=("alpha", at, value))
            for ss in (0.0, -0.0):
                add(f"surface_scale_{ss!r}_{tag}", _l_alpha(), kind, light, ss=ss, se=se, edge=("flat",))
            add(f"region_1x1_{tag}", _l_alpha((1, 1)), kind, light, se=se, edge=("region", (1, 1)))
            add(f"region_2x2_{tag}", _l_alpha((2, 2)), kind, light, se=se, edge=("region", (2, 2)))
    for se in (None, 1.0, 128.0):
        tag = "diffuse" if se is None else f"specular_{se:g}"
        # the light exactly at the surface point of the centre pixel: centre (-0.5, 4.5), height surfaceScale * alpha = 2 * 0.5
        A = _l_alpha()
        A[1, 1] = 0.5
        add(f"point_light_at_the_surface_{tag}", A, LR.POINT, (-0.5, 4.5, 1.0), se=se, edge=("at_surface", (1, 1)))
        # L = (0, 0, -1): the half vector L + (0, 0, 1) is zero.  Layer.lighting reaches it as elevation -90 up to cos(-90 deg) = 6e-17.
        add(f"distant_light_from_below_{tag}", _l_alpha(), LR.DISTANT, (0.0, -90.0), se=se, params=[0, 0, -1, 0, 0, 0, 0, 0],
            edge=("half_vector_zero",))
        # a spot that points at itself: no direction (S = 0), so nothing is lit
        add(f"spot_pointing_at_itself_{tag}", _l_alpha(), LR.SPOT, (0.25, 5.75, 3.0, 0.25, 5.75, 3.0, 2.0, None), se=se,
            edge=("no_direction",))
        for cos, degrees in ((-1.0, 180.0), (0.0, 90.0), (1.0, 0.0)):
            light = (0.25, 5.75, 3.0, -0.5, 4.5, 0.0, 2.0, degrees)
            params = LR.light_frame(_identity(), LR.SPOT, light)
            params[7] = cos
            add(f"spot_cone_cosine_{cos:g}_{tag}", _l_alpha(), LR.SPOT, light, se=se, params=params, edge=("cone", cos))
    # the spot straight above the centre pixel's surface point, looking down: m = -L.S = 1 exactly, which a cone of cosine 1 admits
    A = _l_alpha()
    A[1, 1] = 0.5
    add("spot_cone_cosine_1_on_its_axis", A, LR.SPOT, (-0.5, 4.5, 4.0, -0.5, 4.5, 0.0, 2.0, 0.0), edge=("on_axis", (1, 1)))
    for se in (1.0, 128.0):
        add(f"specular_exponent_{se:g}", _l_alpha(), LR.POINT, (0.25, 5.75, 3.0), se=se, edge=("exponent", se))
    # NaN out of finite parameters: a spot exponent of -1e6 makes pow(m, exponent) infinite for every m < 1, and a colour channel
    # of 0 times that is NaN, which must end as 0 (the other channels end as 1)
    for se in (None, 7.0):
        add(f"spot_exponent_minus_1e6_{'diffuse' if se is None else 'specular'}", _l_alpha(), LR.SPOT,
            (0.25, 5.75, 3.0, -0.5, 4.5, 0.0, -1e6, None), se=se, color=(0.9, 0.0, 1.0), edge=("nan_inside",))
    return cases


# ====================================================================================== refusals
# One ABI call per floating-point parameter, that parameter nan, inf and -inf in turn (`refusals`), everything else valid (`base`).
def refusal_base():
    return dict(
        turbulence=dict(inv=np.array([1.0, 0.0, 0.5, 0.0, 1.0, -0.5]), freq=np.array([0.06, 0.045]), tile=np.array(TURB_TILE), seed=5,
                        octaves=2, fractal=1, stitch=1, shape=(3, 5), offset=(0, 0)),
        transfer=dict(types=np.array([1, 2, 3, 4], dtype=np.int32), params=np.tile(np.array([1.0, 0.0, 1.0, 1.0, 0.0]), (4, 1)),
                      counts=np.array([3, 2, 0, 0], dtype=np.int64), values=np.array([0.1, 0.5, 0.9, 0.2, 0.8]), n_px=6),
        convolve=dict(kernel=CM_KERNEL.copy(), scalars=np.array([CM_KERNEL.sum(), 0.1]), shape=(3, 4)),   # scalars: divisor, bias
        lighting=dict(params=LR.light_frame(_identity(), LR.SPOT, _lights()["spot"][1]), color=np.array(L_COLOR),
                      scalars=np.array([2.0, 0.9, 7.0]), shape=(3, 3), offset=L_OFFSET),   # scalars: surfaceScale, constant, exponent
    )


def refusals():
    """[(primitive, field, index, value)]: set base[primitive][field].flat[index] = value and the entry must refuse the call."""
    base = refusal_base()
    out = []
    for primitive, fields in (("turbulence", ("inv", "freq", "tile")), ("transfer", ("params", "values")),
                              ("convolve", ("kernel", "scalars")), ("lighting", ("params", "color", "scalars"))):
        for field in fields:
            for index in range(base[primitive][field].size):
                out.extend((primitive, field, index, value) for value in NON_FINITE)
    out.extend(("turbulence", "tile", index, value) for index in (2, 3) for value in (0.0, -0.0, -1.0))   # tile sizes 0 and -1
    return out


# ====================================================================================== documents
# Attributes that are not finite, one primitive each, in a 16 x 16 document: (name, the primitive, the attribute the warning names).
_FE = {
    "turbulence_frequency_overflow": ('<feTurbulence baseFrequency="1e400"/>', "baseFrequency"),
    "turbulence_frequency_nan": ('<feTurbulence baseFrequency="0.05 nan"/>', "baseFrequency"),
    "turbulence_octaves_inf": ('<feTurbulence baseFrequency="0.05" numOctaves="inf"/>', "numOctaves"),
    "turbulence_octaves_nan": ('<feTurbulence baseFrequency="0.05" numOctaves="nan"/>', "numOctaves"),
    "turbulence_seed_nan": ('<feTurbulence baseFrequency="0.05" seed="nan"/>', "seed"),
    "transfer_slope_inf": ('<feComponentTransfer><feFuncR type="linear" slope="inf"/></feComponentTransfer>', "feFuncR slope"),
    "transfer_table_nan": ('<feComponentTransfer><feFuncG type="table" tableValues="0 nan 1"/></feComponentTransfer>', "feFuncG tableValues"),
    "convolve_divisor_nan": ('<feConvolveMatrix kernelMatrix="1 0 0 0 1 0 0 0 1" divisor="nan"/>', "divisor"),
    "convolve_kernel_inf": ('<feConvolveMatrix kernelMatrix="1 0 0 0 inf 0 0 0 1"/>', "kernelMatrix"),
    "lighting_surface_scale_inf": ('<feDiffuseLighting surfaceScale="inf"><feDistantLight azimuth="30" elevation="50"/></feDiffuseLighting>',
                                   "surfaceScale"),
    "lighting_point_x_nan": ('<feDiffuseLighting><fePointLight x="nan" y="4" z="5"/></feDiffuseLighting>', "fePointLight x"),
    "lighting_exponent_nan": ('<feSpecularLighting specularExponent="nan"><feDistantLight azimuth="30" elevation="50"/></feSpecularLighting>',
                              "specularExponent"),
    "composite_k1_nan": ('<feComposite in2="SourceAlpha" operator="arithmetic" k1="nan" k2="0.5" k3="0.5"/>', "k1"),
    "displacement_scale_inf": ('<feDisplacementMap in2="SourceGraphic" scale="inf" xChannelSelector="R"/>', "scale"),
    "morphology_radius_nan": ('<feMorphology radius="nan"/>', "radius"),
    "blur_deviation_inf": ('<feGaussianBlur stdDeviation="inf"/>', "stdDeviation"),
    "offset_dx_nan": ('<feOffset dx="nan" dy="1"/>', "dx"),
    "drop_shadow_deviation_inf": ('<feDropShadow stdDeviation="inf"/>', "stdDeviation"),
    "drop_shadow_dx_nan": ('<feDropShadow dx="nan"/>', "dx"),
}


def document(primitive):
    return ('<svg xmlns="http://www.w3.org/2000/svg" width="16" height="16"><defs><filter id="f" x="0" y="0" width="1" height="1">'
            '<feFlood flood-color="#48c" flood-opacity="0.5" result="kept"/>' + primitive +
            '</filter></defs><rect x="2" y="3" width="11" height="9" fill="#c84" filter="url(#f)"/></svg>')


DOCUMENTS = [(name, document(primitive), attribute) for name, (primitive, attribute) in _FE.items()]
# the same primitives with finite numbers: each must survive the check (it drops nothing it should keep)
FINITE_DOCUMENTS = [(name, document(primitive.replace("1e400", "0.05").replace("nan", "2").replace("inf", "2")))
                    for name, (primitive, _attribute) in _FE.items()]

TURBULENCE = _turbulence_cases()
TRANSFER = _transfer_cases()
CONVOLVE = _convolve_cases()
LIGHTING = _lighting_cases()
REFUSALS = refusals()


# ====================================================================================== the case file of the harness program
def _hex(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == INF else ("-inf" if v == -INF else v.hex()))


def _line(kind, *parts):
    out = [kind]
    for p in parts:
        if isinstance(p, (int, np.integer)):
            out.append(str(int(p)))
        elif isinstance(p, (float, np.floating)):
            out.append(_hex(p))
        else:
            out.extend(_hex(v) for v in np.asarray(p, dtype=np.float64).ravel())
    return " ".join(out)


def case_file():
    """(text, number of cases, number the program must report as refused) for tests/filter_harness.cpp's program: every
    turbulence, transfer, convolve and lighting case, and the turbulence parameters of the refusals and of the stitch bound."""
    from svgrasterize_amd.layer import turbulence_seed

    lines, refused = [], 0
    for c in TURBULENCE:
        px, py = turb_points(c)
        lines.append(_line("T", turbulence_seed(c["seed"]), c["freq"][0], c["freq"][1], (0, 0, 0, 0) if c["tile"] is None else c["tile"],
                           c["octaves"], int(c["fractal"]), int(c["tile"] is not None), len(px), np.stack([px, py], axis=1)))
    pts = np.array([[1.5, 2.5], [-70000.25, 1e300]])
    for what, accepted in STITCH_BOUND:
        lines.append(_line("T", 5, what["freq"][0], what["freq"][1], what["tile"], what["octaves"], 0, 1, len(pts), pts))
        refused += not accepted
    base = refusal_base()["turbulence"]
    for primitive, field, index, value in REFUSALS:
        if primitive == "turbulence" and field != "inv":
            p = {k: np.array(base[k], dtype=np.float64) for k in ("freq", "tile")}
            p[field][index] = value
            lines.append(_line("T", 5, p["freq"][0], p["freq"][1], p["tile"], base["octaves"], 1, 1, len(pts), pts))
            refused += 1
    for c in TRANSFER:
        kind, prm, values = F.transfer_abi(c["fn"])
        lines.append(_line("X", kind, prm, len(values), values, len(c["c"]), c["c"]))
    for c in CONVOLVE:
        oy, ox = c["kernel"].shape
        lines.append(_line("C", c["image"].shape[0], c["image"].shape[1], ox, oy, c["target"][0], c["target"][1],
                           F.EDGE_MODES[c["edge_mode"]], int(c["preserve"]), c["divisor"], c["bias"], c["kernel"], c["image"]))
    for c in LIGHTING:
        lines.append(_line("L", c["kind"], c["params"], c["color"], c["ss"], c["constant"], 1.0 if c["se"] is None else c["se"],
                           int(c["se"] is not None), c["offset"][0], c["offset"][1], c["A"].shape[0], c["A"].shape[1], c["A"]))
    return "\n".join(lines) + "\n", len(lines), refused
