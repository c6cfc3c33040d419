"""The dasher on the GPU (svgr_path_dash through the C ABI) against the host reference of the same metric
(tests/dash_ref.py), on shapes at the seams of its launch geometry: S = svgr_dash_scan_segments() segments per workgroup of
the scans, 32 lanes per segment, two segments per wave.  The structure of the output is compared exactly, its control
points within dash_ref's derived tolerance; tests/test_dash_host.py checks on the CPU that the inputs meet the conditions."""
import warnings

import numpy as np
import pytest

from tests import dash_cases as cases
from tests import dash_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from svgrasterize_amd import _abi

    _abi.Context.get()
    return _abi


FIXED = cases.fixed_cases()


def check(abi, case, want=None):
    name, path, dashes, offset, plen, exact = case
    detail = {"exact": exact}
    wt, wp, ws = want if want is not None else R.dash(*path, dashes, offset, plen, detail=detail)
    gt, gp, gs = abi.path_dash(*path, dashes, offset, plen)
    assert list(gs) == list(ws), name
    assert list(gt) == list(wt), name
    if exact:
        assert np.array_equal(gp, wp), name
        return 0.0
    tol = R.tolerance(np.asarray(path[1]), len(path[0]), detail["length"], detail["period"])
    err = float(np.abs(gp - wp).max()) if len(wp) else 0.0
    print(f"{name}: max |delta| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (name, err, tol)
    return err


def test_scan_reach_is_what_the_cases_assume(abi):
    assert abi.dash_scan_segments() == cases.S


@pytest.mark.parametrize("case", FIXED, ids=[c[0] for c in FIXED])
def test_fixed_case(abi, case):
    check(abi, case)


def test_fuzz_set(abi):
    ran = 0
    for case in cases.fuzz_cases():
        detail = {}
        want = R.dash(*case[1], case[2], case[3], case[4], detail=detail)
        if detail["clearance"] < 1e-6:
            continue
        name, path, dashes, offset, plen, exact = case
        gt, gp, gs = abi.path_dash(*path, dashes, offset, plen)
        assert list(gs) == list(want[2]) and list(gt) == list(want[0]), name
        tol = R.tolerance(np.asarray(path[1]), len(path[0]), detail["length"], detail["period"])
        assert np.abs(gp - want[1]).max() <= tol, name
        ran += 1
    assert ran >= 190


def test_two_runs_are_byte_identical(abi):
    case = next(c for c in FIXED if c[0] == f"mix{2 * cases.S + 1}")
    a = abi.path_dash(*case[1], case[2], case[3], case[4])
    b = abi.path_dash(*case[1], case[2], case[3], case[4])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_degenerate_input(abi):
    t, p, s = abi.path_dash([], np.zeros((0, 8)), [], [3, 2])
    assert len(t) == 0 and len(p) == 0 and len(s) == 0
    line = R.polyline([(0, 0), (10, 0)])
    for bad in (float("nan"), float("inf"), 1e155):   # (1e155: finite, but its square is not)
        params = np.array(line[1], dtype=np.float64)
        params[0, 2] = bad
        before = abi.Context.get().launches()
        with pytest.raises(ValueError):
            abi.path_dash(line[0], params, line[2], [3, 2])
        assert abi.Context.get().launches() == before   # nothing was launched
    # solid patterns hand the input back
    t, p, s = abi.path_dash(*line, [5, 0])
    assert list(t) == line[0] and np.array_equal(p, np.array(line[1], dtype=np.float64)) and list(s) == line[2]
    with pytest.raises(ValueError):
        abi.path_dash(*line, [1.0] * 65)


HEAD = '<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64">'
RECT = '<rect x="8" y="8" width="40" height="20" fill="none" stroke="#c00" stroke-width="2" stroke-dasharray="6 2" stroke-dashoffset="3"/>'
GROUP = '<g stroke-dasharray="5 3" stroke="#00f" fill="none" stroke-width="3">%s</g>'
LINE = '<path d="M4,58 L60,58" stroke-linecap="round"/>'
CUBIC = '<path d="M4,40 C20,20 40,60 60,40"/>'
SVG_LINES = HEAD + RECT + GROUP % LINE + "</svg>"          # integer lines, integer dashes: the reference's outputs are exact
SVG_CUBIC = HEAD + GROUP % CUBIC + "</svg>"
SVG_ALL = HEAD + RECT + GROUP % (CUBIC + LINE) + "</svg>"   # a dashed rectangle, a dashed cubic, an inherited dasharray

class HostDash:
    """Stands in for Path.dash: dash_ref on the host, in float64; keeps the outlines it made, float64 and long double."""

    def __init__(self):
        self.outlines = []

    def __call__(self, path, dashes, offset=0.0, path_length=None):
        from svgrasterize_amd import geometry

        types, params, sizes = path._segment_arrays()
        t, p, s = R.dash(types, np.array(params), sizes, dashes, offset, path_length or 0.0)
        wide = R.dash(types, np.array(params), sizes, dashes, offset, path_length or 0.0, long_double=True)
        self.outlines.append(((t, p, s), wide))
        return geometry.Path.from_segments(t, p, s)


class DeviceDash:
    """Path.dash as it is, keeping the outlines it made."""

    def __init__(self, real):
        self.real, self.outlines = real, []

    def __call__(self, path, dashes, offset=0.0, path_length=None):
        out = self.real(path, dashes, offset, path_length)
        self.outlines.append(out._segment_arrays())
        return out


def both_ways(monkeypatch, run):
    """run() with the dasher on the device, then with dash_ref in its place: (result, outlines) of each."""
    import svgrasterize_amd as S
    from svgrasterize_amd import geometry

    device, host = DeviceDash(geometry.Path.dash), HostDash()
    monkeypatch.setattr(geometry.Path, "dash", lambda self, *a, **k: device(self, *a, **k))
    S.clear_render_cache()
    got = run()
    monkeypatch.setattr(geometry.Path, "dash", lambda self, *a, **k: host(self, *a, **k))
    S.clear_render_cache()
    want = run()
    S.clear_render_cache()
    assert len(device.outlines) == len(host.outlines) > 0
    return got, device.outlines, want, host.outlines


def render_float(text):
    import svgrasterize_amd as S

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scene, _ids, _size = S.svg_scene_from_str(text)
    out = scene.render(S.Transform(), viewport=[0, 0, 64, 64], linear_rgb=True)
    assert out is not None
    layer = out[0]
    canvas = np.zeros((64, 64, 4))
    img = layer.image
    y, x = layer.offset
    canvas[y:y + img.shape[0], x:x + img.shape[1]] = img
    return canvas


def test_document_through_render_svg(abi, monkeypatch):
    """The whole document -- dashed rectangle, dashed cubic, inherited dasharray -- through render_svg, against the same call
    with dash_ref on the host in the dasher's place (same stroker, same route).  The float renders behind the two files differ
    by a float32 ULP (lines) or by the cubic's outline distance, ~1e-14 pixel: neither moves an 8-bit value by more than one
    level, and only where the value sits on a rounding edge."""
    import io

    import svgrasterize_amd as S

    got, _d, want, _h = both_ways(monkeypatch, lambda: S.read_png(S.render_svg(io.StringIO(SVG_ALL))))
    assert got.shape == want.shape == (64, 64, 4)
    assert got[..., 3].max() > 128 and (got[..., 3] == 0).any()
    # the dashed shapes differ from their solid strokes: along the rectangle's top edge there are dashes and gaps
    assert got[9, 8:48, 3].min() < 3 and got[9, 8:48, 3].max() > 250
    delta = np.abs(got.astype(int) - want.astype(int))
    print(f"render_svg: {int((delta > 0).sum())} values differ, max {int(delta.max())} level(s)")
    assert delta.max() <= 1


def test_line_shapes_render_within_one_ulp(abi, monkeypatch):
    """Integer lines with integer dashes: the device's outlines equal dash_ref's bit for bit, and the renders then differ by
    at most the float32 contract's 1 ULP."""
    got, dev, want, host = both_ways(monkeypatch, lambda: render_float(SVG_LINES))
    for (gt, gp, gs), ((wt, wp, ws), _wide) in zip(dev, host):
        assert list(gt) == list(wt) and list(gs) == list(ws)
        assert np.array_equal(np.asarray(gp, dtype=np.float64).reshape(-1, 8), wp)
    assert got[..., 3].max() > 0.5 and got[9, 8:48, 3].min() < 0.01 < got[9, 8:48, 3].max()
    want32 = np.abs(want.astype(np.float32))
    ulp = np.maximum(np.nextafter(want32, np.float32(np.inf)) - want32, np.float32(2.0 ** -24)).astype(np.float64)
    err = np.abs(got - want)
    print(f"lines: max |delta| {err.max():.3e}")
    assert (err <= ulp).all()


def test_cubic_outline_within_four_times_the_measured_distance(abi, monkeypatch):
    """The dashed cubic: max |delta| between the device's outline and dash_ref's float64 one, against 4 x cases.CUBIC_DISTANCE."""
    got, dev, want, host = both_ways(monkeypatch, lambda: render_float(SVG_CUBIC))
    (gt, gp, gs), ((wt, wp, ws), wide) = dev[0], host[0]
    assert len(dev) == 1 and list(gt) == list(wt) and list(gs) == list(ws)
    measured = float(np.abs(wp - wide[1]).max())
    err = float(np.abs(np.asarray(gp, dtype=np.float64).reshape(-1, 8) - wp).max())
    print(f"cubic: outline max |delta| {err:.3e}, float64 to long double {measured:.3e} (recorded {cases.CUBIC_DISTANCE:.3e}), "
          f"render max |delta| {np.abs(got - want).max():.3e}")
    assert got[..., 3].max() > 0.5
    assert err <= 4 * cases.CUBIC_DISTANCE
