"""The filter primitives at the edges of their values, on the CPU: the host build of csrc/svgr_core.h (tests/filter_harness.cpp,
tests/lighting_harness.cpp) against the restatements (tests/filter_ref.py, tests/lighting_ref.py) for every case of
tests/filter_edge_cases.py, each case shown to reach the edge it is for; the parameters turbulence refuses and the stitch bound
from both sides; the loader's handling of numbers that are not finite; and the harness alone as a program under the
undefined-behaviour sanitizer, whose clean run shows that no case reads outside a table, converts out of range or overflows
an integer.  tests/test_gpu_filter_edges.py sends the same cases to the device."""
import math
import os
import subprocess
import warnings
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from tests import filter_edge_cases as E
from tests import filter_ref as F
from tests import lighting_ref as LR
from tests.util import ROOT

GAMMA_TOL, LIGHTING_TOL, TURBULENCE_TOL = 1e-14, 1e-13, 1e-15   # the tolerances of the primitives' own tests


@pytest.fixture(scope="module")
def fh():
    return F.harness()


@pytest.fixture(scope="module")
def lh():
    return LR.harness()


def _unit(values, what):
    assert not np.isnan(values).any() and (values >= 0.0).all() and (values <= 1.0).all(), what


def _names(cases):
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return names


# ====================================================================================== feTurbulence
def turb_reaches(case):
    """Asserts that the case is at the edge it names."""
    px, py = E.turb_points(case)
    at = E.TURB_AT[0] * case["shape"][1] + E.TURB_AT[1]
    trace = [F.turbulence_trace(case["seed"], case["freq"], case["octaves"], case["tile"], x, y) for x, y in zip(px, py)]
    kind = case["edge"][0]
    if kind == "threshold":
        _, T, octave, side = case["edge"]
        tx = trace[at][octave][0]
        assert (tx < T) if side == "under" else (tx >= T), (tx, T)
        assert abs(tx - T) <= 8 * np.spacing(T)
        assert octave == case["octaves"] - 1 and all(row[0] <= T / 2 + 4096.0 for row in trace[at][:octave])   # (crossed there only)
    elif kind == "frequency_zero":
        assert 0.0 in case["freq"]
    elif kind == "octaves":
        assert case["octaves"] == case["edge"][1] and len(trace[at]) == case["edge"][1]
    elif kind == "negative":
        for rows in trace:
            tx, ty = rows[0][0], rows[0][1]
            assert tx < -1.0 and ty < -1.0 and F.turbulence_cell(tx)[1] < 0.0 and F.turbulence_cell(tx)[0] == -math.floor(-tx)
    elif kind == "integer":
        assert all(F.turbulence_cell(row[0])[1] == 0.0 and math.isfinite(row[0]) for rows in trace for row in rows)
        assert any(F.turbulence_cell(row[1])[1] != 0.0 for rows in trace for row in rows)
    elif kind == "overflow":
        first = [k for k, row in enumerate(trace[at]) if math.isinf(row[0])]
        assert first and first[0] == case["edge"][1] and all(math.isfinite(v) for v in (*px, *py))
    elif kind == "seed":
        from svgrasterize_amd.layer import turbulence_seed

        seed = case["edge"][1]
        assert F.setup_seed(turbulence_seed(seed)) == F.setup_seed(math.trunc(seed)) and -2 ** 63 <= turbulence_seed(seed) < 2 ** 63
    elif kind == "stitch_bound":
        _fx, _fy, width, _h, wrap, _wy = F.turbulence_params(*case["freq"], case["tile"], True)
        state = 2 ** (case["octaves"] - 1) * max(width, abs(wrap - F.PERLIN_N)) + F.PERLIN_N
        assert state <= F.STATE_MAX < state + 2 ** (case["octaves"] - 1)   # (one more unit of width would leave the bound)
    else:
        raise AssertionError(f"unknown edge {kind}")


@pytest.mark.parametrize("name", _names(E.TURBULENCE))
def test_turbulence_header_against_restatement(fh, name):
    from svgrasterize_amd.layer import turbulence_seed

    case = next(c for c in E.TURBULENCE if c["name"] == name)
    turb_reaches(case)
    px, py = E.turb_points(case)
    tile4 = np.ascontiguousarray((0, 0, 0, 0) if case["tile"] is None else case["tile"], dtype=np.float64)
    assert F.turbulence_accepts(case["freq"], case["octaves"], case["tile"])
    assert fh.fh_turbulence_valid(*case["freq"], tile4, case["octaves"], int(case["tile"] is not None)) == 1
    host = F.harness_turbulence(fh, turbulence_seed(case["seed"]), case["freq"], case["octaves"], case["fractal"], case["tile"], px, py)
    want = F.turbulence_exact(case["seed"], case["freq"], case["octaves"], case["fractal"], case["tile"], px, py)
    _unit(host, name)
    err = float(np.abs(host - want).max())
    print(f"{name}: max |host - restatement| {err:.3e}, bound {TURBULENCE_TOL}")
    assert err <= TURBULENCE_TOL
    layer = F.harness_turbulence_layer(fh, E.turb_transform(case), case["offset"], case["shape"], case["freq"], case["octaves"],
                                       turbulence_seed(case["seed"]), case["tile"], case["fractal"])
    assert np.array_equal(layer.reshape(-1, 4), host)
    if case["octaves"] == 0:
        assert np.array_equal(host, np.full_like(host, 0.5 if case["fractal"] else 0.0))
    if case["edge"][0] == "overflow":   # an infinite lattice coordinate: no noise there, 0 in every channel
        assert (host[E.TURB_AT[0] * case["shape"][1] + E.TURB_AT[1]] == 0.0).all()


def test_turbulence_state_is_the_restatements(fh):
    for case in E.TURBULENCE:
        if case["tile"] is None:
            continue
        st, f = np.zeros(4, dtype=np.int64), np.zeros(2)
        fh.fh_turbulence_state(*case["freq"], np.ascontiguousarray(case["tile"], dtype=np.float64), case["octaves"], 1, st, f)
        fx, fy, width, height, wrap_x, wrap_y = F.turbulence_params(*case["freq"], case["tile"], True)
        assert (f[0], f[1], *st.tolist()) == (fx, fy, width, height, wrap_x, wrap_y), case["name"]


def test_turbulence_stitch_bound_from_both_sides(fh):
    seen = set()
    for what, accepted in E.STITCH_BOUND:
        tile4 = np.ascontiguousarray(what["tile"], dtype=np.float64)
        assert F.turbulence_accepts(what["freq"], what["octaves"], what["tile"]) is accepted, what
        assert fh.fh_turbulence_valid(*what["freq"], tile4, what["octaves"], 1) == int(accepted), what
        assert fh.fh_turbulence_valid(*what["freq"], tile4, what["octaves"], 0) == 1   # (without stitching the tile does not count)
        seen.add(accepted)
    assert seen == {True, False}


def test_turbulence_refusals_on_the_host(fh):
    from svgrasterize_amd.layer import turbulence_seed

    base = E.refusal_base()["turbulence"]
    n = 0
    for primitive, field, index, value in E.REFUSALS:
        if primitive != "turbulence" or field == "inv":
            continue
        p = {k: np.array(base[k], dtype=np.float64) for k in ("freq", "tile")}
        assert fh.fh_turbulence_valid(*p["freq"], p["tile"], base["octaves"], 1) == 1
        p[field][index] = value
        assert fh.fh_turbulence_valid(*p["freq"], p["tile"], base["octaves"], 1) == 0, (field, index, value)
        assert not F.turbulence_accepts(p["freq"], base["octaves"], p["tile"])
        n += 1
    assert n == 3 * 6 + 6
    for octaves in (-1, 33):
        assert fh.fh_turbulence_valid(*base["freq"], base["tile"], octaves, 1) == 0
    for seed in E.NON_FINITE:
        with pytest.raises(ValueError):
            turbulence_seed(seed)


# ====================================================================================== feComponentTransfer
@pytest.mark.parametrize("name", _names(E.TRANSFER))
def test_transfer_header_against_restatement(fh, name):
    case = next(c for c in E.TRANSFER if c["name"] == name)
    c, fn = case["c"], case["fn"]
    assert np.isnan(c).any() and np.isinf(c).any() and (c == 2.0 ** -1074).any() and (c == 1.0 - 2.0 ** -53).any()
    host = F.harness_transfer(fh, c, fn)
    want = F.transfer(c, fn)
    raw = F.transfer(c, fn, raw=True)
    _unit(host, name)
    if fn is not None and fn[0] == "gamma":
        assert np.abs(host - want).max() <= GAMMA_TOL
    else:
        assert np.array_equal(host, want), (host, want)
    # NaN and everything at or below 0 go the way of 0, everything from 1 up the way of 1
    zero, one = host[list(c).index(0.0)], host[list(c).index(1.0)]
    assert all(host[k] == zero for k, v in enumerate(c) if math.isnan(v) or v <= 0.0)
    assert all(host[k] == one for k, v in enumerate(c) if v >= 1.0)
    edge = case["edge"]
    if edge is None:
        return
    if edge[0] == "nan_inside":     # finite parameters, finite pixel, NaN before the last clamp: it ends as 0
        assert np.isfinite(np.asarray(fn[1:] if fn[0] == "gamma" else fn[1], dtype=np.float64)).all()
        inside = np.isnan(raw) & np.isfinite(c)
        assert inside.any() and (host[inside] == 0.0).all()
    elif edge[0] == "inf_inside":
        assert (np.isinf(raw) & np.isfinite(c)).any()
    elif edge[0] == "knots":
        m = edge[1]
        t = np.clip(c, 0, 1) * m
        on = np.isfinite(c) & (t == np.floor(t)) & (t > 0) & (t < m)
        assert on.sum() >= m - 1
        if fn[0] == "table":
            assert all(host[k] == F.clamp_unit(fn[1][int(t[k])]) for k in np.flatnonzero(on))
        else:
            assert all(host[k] == fn[1][int(t[k])] for k in np.flatnonzero(on))   # (c n = k: the step k begins there)
    elif edge[0] == "length":
        assert len(fn[1]) == edge[1] and abs(host[list(c).index(1.0)] - F.clamp_unit(fn[1][-1])) <= 2.0 ** -52   # (the last entry is read)
    elif edge[0] == "outside":
        assert ((raw < 0.0) | (raw > 1.0)).any() and (min(fn[1]) < 0.0 and max(fn[1]) > 1.0)
    else:
        raise AssertionError(f"unknown edge {edge[0]}")


# ====================================================================================== feConvolveMatrix
def _zero_weight_meets(case, at):
    """Whether some output pixel reads the source pixel `at` through a weight of 0 (edge mode `none`'s view: inside the image)."""
    oy, ox = case["kernel"].shape
    tx, ty = case["target"]
    rows, cols = case["image"].shape[:2]
    for I in range(oy):
        for J in range(ox):
            R, Cc = at[0] + ty - I, at[1] + tx - J
            if case["kernel"][oy - 1 - I, ox - 1 - J] == 0.0 and 0 <= R < rows and 0 <= Cc < cols:
                return True
    return False


@pytest.mark.parametrize("name", _names(E.CONVOLVE))
def test_convolve_matrix_header_against_restatement(fh, name):
    case = next(c for c in E.CONVOLVE if c["name"] == name)
    img, kernel, preserve = case["image"], case["kernel"], case["preserve"]
    args = (img, kernel, case["divisor"], case["bias"], case["target"], case["edge_mode"], preserve)
    host = F.harness_convolve_matrix(fh, *args)
    want = F.convolve_matrix(*args)
    assert np.array_equal(host, want), float(np.nanmax(np.abs(host - want)))
    colours = host[..., :3] if preserve else host
    _unit(colours, name)
    if preserve:
        assert np.array_equal(host[..., 3], img[..., 3])
    else:
        assert (host[..., :3] <= host[..., 3:]).all()
    edge = case["edge"]
    if edge[0] == "odd_pixel":
        foot = F.convolve_footprint(img.shape[:2], kernel.shape, case["target"], case["edge_mode"], E.CM_AT)
        odd = img[E.CM_AT][0]
        assert not np.isfinite(odd) and np.isfinite(np.delete(img.reshape(-1, 4), E.CM_AT[0] * img.shape[1] + E.CM_AT[1], axis=0)).all()
        assert foot[E.CM_AT] and _zero_weight_meets(case, E.CM_AT)
        assert foot.sum() == {"none": 4, "duplicate": 4, "wrap": 9}[case["edge_mode"]]   # (a corner: 2 x 2 inside, all nine by wrap)
        clean = img.copy()
        clean[E.CM_AT] = 0.5
        away = F.convolve_matrix(clean, *args[1:])
        assert np.array_equal(colours[~foot], (away[..., :3] if preserve else away)[~foot])   # nothing else sees the odd pixel
        assert (colours[~foot] > 0.0).all()
        if edge[1] == "nan":          # exactly the footprint is 0, the positions with weight 0 included
            assert (colours[foot] == 0.0).all()
        elif edge[1] == "minus_inf":  # -inf times a positive weight is -inf, times 0 is NaN: 0 either way
            assert (colours[foot] == 0.0).all()
        else:                         # +inf: the top of the clamp, except where it meets the weight 0 (NaN -> 0)
            values = set(np.unique(colours[foot][..., 0]))
            # (`duplicate` repeats the corner into every footprint's outside part, where the weight 0 finds it each time)
            assert values == ({0.0} if case["edge_mode"] == "duplicate" else {0.0, 1.0}), values
    elif edge[0] == "alpha_zero":
        assert (img[..., 3] == 0.0).sum() == 9 and (host[..., 3] == 0.0).sum() == 9
    elif edge[0] == "exactly":
        assert (colours == edge[1]).all()
        assert (4.5 / case["divisor"] + case["bias"]) == edge[1]
    elif edge[0] == "huge":
        assert set(np.unique(colours)) <= {0.0, 1.0} and (colours == 0.0).any()
        assert abs(case["divisor"]) == 2.0 ** -1000
    else:
        raise AssertionError(f"unknown edge {edge[0]}")


# ====================================================================================== lighting
@pytest.mark.parametrize("name", _names(E.LIGHTING))
def test_lighting_header_against_restatement(lh, name):
    case = next(c for c in E.LIGHTING if c["name"] == name)
    A, params, offset = case["A"], case["params"], case["offset"]
    args = (A, offset, case["kind"], params, case["color"], case["ss"], case["constant"], case["se"])
    host = LR.harness_layer(lh, *args)
    want = LR.lighting(*args)
    _unit(host, name)
    _unit(want, name)
    err = float(np.abs(host - want).max())
    assert err <= LIGHTING_TOL, err
    assert np.array_equal(host[..., 3], host[..., :3].max(axis=-1) if case["se"] is not None else np.ones(A.shape))
    from_light = LR.light_frame(E._identity(), case["kind"], case["light"])
    assert np.abs(from_light - params).max() <= 1e-15   # (`light` is `params` up to the rounding of cos(90 degrees))
    edge = case["edge"]
    R, Cc = np.indices(A.shape)
    d0, d1 = offset[0] + R + 0.5, offset[1] + Cc + 0.5
    if edge[0] == "alpha":
        _, at, value = edge
        assert (math.isnan(A[at]) if math.isnan(value) else A[at] == value) and np.isfinite(np.delete(A.ravel(), at[0] * 3 + at[1])).all()
        clean = A.copy()
        clean[at] = 0.5
        assert not np.array_equal(LR.lighting(clean, *args[1:]), want)   # (the odd alpha is seen)
    elif edge[0] == "flat":
        assert case["ss"] == 0.0 and all(np.array_equal(n, np.full(A.shape, v)) for n, v in zip(LR.normals(A, case["ss"]), (0, 0, 1)))
    elif edge[0] == "region":
        assert A.shape == edge[1]
    elif edge[0] == "at_surface":
        at = edge[1]
        assert params[0] - d0[at] == 0.0 and params[1] - d1[at] == 0.0 and params[2] - case["ss"] * A[at] == 0.0
    elif edge[0] == "half_vector_zero":
        assert tuple(params[:3]) == (0.0, 0.0, -1.0)
        if case["se"] is not None:
            assert (host == 0.0).all()
    elif edge[0] == "no_direction":
        assert tuple(params[3:6]) == (0.0, 0.0, 0.0) and (host[..., :3] == 0.0).all()
    elif edge[0] == "cone":
        assert params[7] == edge[1]
        if edge[1] == 1.0:
            assert (host[..., :3] == 0.0).all()     # (no pixel lies exactly on the axis)
        if edge[1] == -1.0 and case["se"] is None:
            assert (host[..., :3] > 0.0).any()
    elif edge[0] == "on_axis":
        at = edge[1]
        assert params[7] == 1.0 and (host[at][:3] > 0.0).all() and (np.delete(host[..., :3].reshape(-1, 3), 4, axis=0) == 0.0).all()
    elif edge[0] == "exponent":
        assert case["se"] == edge[1] and (host[..., :3] > 0.0).any()
    elif edge[0] == "nan_inside":   # finite parameters and pixels, 0 * inf = NaN before the last clamp: it ends as 0, next to channels at 1
        assert np.isfinite(params).all() and np.isfinite(A).all() and case["color"][1] == 0.0
        v = np.stack([params[0] - d0, params[1] - d1, params[2] - case["ss"] * A])
        m = -np.einsum("krc,k->rc", v / np.sqrt((v * v).sum(axis=0)), params[3:6])
        with np.errstate(over="ignore"):
            assert (m > 0.0).all() and np.isinf(np.power(m, params[6])).all()   # every pixel is lit, by an infinite factor
        assert (host[..., 1] == 0.0).all() and (host[..., 0] == 1.0).any()
    else:
        raise AssertionError(f"unknown edge {edge[0]}")


def test_refusals_name_every_parameter():
    """One refusal per floating-point parameter of the four entries and per non-finite value (the device test runs them)."""
    base = E.refusal_base()
    count = {}
    for primitive, field, index, value in E.REFUSALS:
        assert 0 <= index < base[primitive][field].size and np.isfinite(base[primitive][field]).all()
        if not math.isfinite(value):
            count[(primitive, field)] = count.get((primitive, field), 0) + 1
    assert count == {("turbulence", "inv"): 18, ("turbulence", "freq"): 6, ("turbulence", "tile"): 12, ("transfer", "params"): 60,
                     ("transfer", "values"): 15, ("convolve", "kernel"): 27, ("convolve", "scalars"): 6, ("lighting", "params"): 24,
                     ("lighting", "color"): 9, ("lighting", "scalars"): 9}


# ====================================================================================== the loader
def _load_filter(text):
    from svgrasterize_amd import svg

    element = next(e for e in ET.fromstring(text).iter() if e.tag.endswith("}filter"))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        flt = svg._filter(element)
    return flt, [str(w.message) for w in caught]


@pytest.mark.parametrize("name", [d[0] for d in E.DOCUMENTS])
def test_loader_drops_a_primitive_whose_number_is_not_finite(name):
    import svgrasterize_amd as S

    _, text, attribute = next(d for d in E.DOCUMENTS if d[0] == name)
    flt, messages = _load_filter(text)
    assert len(flt.filters) == 1, flt.filters                    # the flood in front of it stays, the primitive is gone
    tag = text.split("result=\"kept\"/><")[1].split(" ")[0].split(">")[0]
    assert any(m.startswith(f"{tag}: {attribute} is not finite") for m in messages), messages
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scene, _ids, _size = S.svg_scene_from_str(text)          # and the document as a whole loads
    assert scene is not None


@pytest.mark.parametrize("name", [d[0] for d in E.FINITE_DOCUMENTS])
def test_loader_keeps_the_primitive_when_its_numbers_are_finite(name):
    _, text = next(d for d in E.FINITE_DOCUMENTS if d[0] == name)
    flt, messages = _load_filter(text)
    assert len(flt.filters) > 1 and not any("not finite" in m for m in messages), messages


def test_loader_leaves_names_alone():
    # `result`, `in` and ids are names, not numbers: "inf" and "nan" there are fine
    text = E.document('<feOffset in="kept" dx="1" dy="1" result="inf"/><feOffset in="inf" dx="1" dy="1" result="nan"/>')
    flt, messages = _load_filter(text)
    assert len(flt.filters) == 3 and not messages


# ====================================================================================== the harness alone, under the sanitizer
def test_harness_alone_under_the_sanitizer(tmp_path):
    # host code only, as a program of its own: nothing of it is loaded into this process
    exe, cases = str(tmp_path / "filter_harness"), str(tmp_path / "cases.txt")
    text, n_cases, n_refused = E.case_file()
    with open(cases, "w") as f:
        f.write(text)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-static-libubsan", "-DFILTER_HARNESS_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "filter_harness.cpp")])
    done = subprocess.run([exe, cases], capture_output=True, text=True)
    assert n_cases >= len(E.TURBULENCE) + len(E.TRANSFER) + len(E.CONVOLVE) + len(E.LIGHTING) + len(E.STITCH_BOUND) and n_refused > 20
    assert done.returncode == 0 and not done.stderr, done.stderr
    assert done.stdout.strip() == f"filter harness: {n_cases} cases, {n_refused} refused", done.stdout
