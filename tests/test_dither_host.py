"""Dithering on the CPU: csrc/svgr_dither.h (through tests/dither_harness.cpp) against the numpy restatement of the same
definitions (tests/dither_ref.py), bit for bit; what dithering is for, measured against a known truth; the arguments of the
public route, refused before any device work; the ABI; and the harness alone under the address and undefined-behaviour
sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import svgrasterize_amd as S
from svgrasterize_amd import _abi, quant
from tests import dither_ref as R
from tests import quant_ref as Q
from tests.util import ROOT

MODES = ("ordered", "diffusion")


@pytest.fixture(scope="module")
def lib():
    return R.harness()


def _noise(rows, cols, seed):
    img = np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    img[::3, ::2, 3] = 0          # transparent, with stray colour
    img[1::2, 1::3, 3] = 255      # opaque; the rest is translucent
    return img


def _palette(n, seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    pal[::2, 3] = 255
    if n > 2:
        pal[1] = 0
    return pal


def _ramp(rows=16, cols=256):
    img = np.zeros((rows, cols, 4), dtype=np.uint8)
    img[..., :3] = np.arange(cols, dtype=np.uint8)[None, :, None]
    img[..., 3] = 255
    return img


def _greys(*values):
    return np.array([(v, v, v, 255) for v in values], dtype=np.uint8)


@pytest.mark.parametrize("n_pal", [1, 2, 3, 16, 17, 255, 256])
def test_header_is_the_restatement(lib, n_pal):
    pal = _palette(n_pal, n_pal)
    amp = R.amplitude_ref(pal)
    assert quant.ordered_amplitude(pal) == amp
    for cols in (1, 2, 7, 8, 9, 17):
        for rows in (1, 2, 3, 9):
            img = _noise(rows, cols, 1000 * n_pal + 10 * cols + rows)
            for mode in MODES:
                stream, idx = R.harness_dither(lib, img, pal, mode, amp)
                assert np.array_equal(idx, R.dither_ref(img, pal, mode, amp)), (mode, rows, cols)
                assert np.array_equal(stream, Q.pack_rows(idx, Q.depth_of(n_pal))), (mode, rows, cols)
    big = R.harness_dither(lib, img, pal, "ordered", R.X_MAX)[1]   # (the largest amplitude: every clamp is reached)
    assert np.array_equal(big, R.ordered_ref(img, pal, R.X_MAX))


def test_bayer_matrix(lib):
    B = np.array([[lib.h_bayer(r, c) for c in range(8)] for r in range(8)])
    assert sorted(B.reshape(-1)) == list(range(64))
    assert (B[0, 0], B[0, 1], B[1, 0], B[1, 1]) == (0, 32, 48, 16)
    assert np.array_equal(B, R.bayer())
    assert lib.h_bayer(8 + 3, 16 + 5) == B[3, 5]


def test_ordered_amplitude():
    assert quant.ordered_amplitude(_greys(0, 255)) == 65025 == R.amplitude_ref(_greys(0, 255))
    assert quant.ordered_amplitude(_greys(0, 85, 170, 255)) == 21675 == R.amplitude_ref(_greys(0, 85, 170, 255))
    assert quant.ordered_amplitude(_greys(7)) == 0
    for n in (2, 3, 17, 256):
        assert quant.ordered_amplitude(_palette(n, n)) == R.amplitude_ref(_palette(n, n))


@pytest.mark.parametrize("values", [(0, 255), (0, 85, 170, 255)])
def test_block_means_follow_the_ramp(lib, values):
    # the truth is the ramp itself: dithering exists to keep its local averages, which plain rounding loses in bands
    ramp, pal = _ramp(), _greys(*values)
    plain = R.block_mean_error(Q.harness_index(Q.harness(), ramp, pal)[1], pal, ramp)
    for mode in MODES:
        got = R.block_mean_error(R.harness_dither(lib, ramp, pal, mode, quant.ordered_amplitude(pal))[1], pal, ramp)
        print(len(values), "greys:", mode, got, "against", plain, "undithered")
        assert got <= plain / 5, (mode, got, plain)


def test_palette_colours_keep_their_indices_under_diffusion(lib):
    pal = _palette(17, 3)
    img = pal[np.random.default_rng(5).integers(0, 17, (9, 23))]
    img[img[..., 3] == 0, :3] = (9, 8, 7)
    assert np.array_equal(R.harness_dither(lib, img, pal, "diffusion")[1], Q.harness_index(Q.harness(), img, pal)[1])
    # ordered: the same with nothing to move by (amplitude 0), at any alpha
    assert np.array_equal(R.harness_dither(lib, img, pal, "ordered", 0)[1], Q.harness_index(Q.harness(), img, pal)[1])


def test_transparent_pixels_stop_the_error(lib):
    pal = np.concatenate([_greys(0, 255), np.array([[200, 10, 10, 0]], dtype=np.uint8)])
    solid = _ramp(1, 96)
    solid[..., :3] += 100   # (mid greys: every pixel leaves an error worth passing on)
    ramp = solid.copy()
    ramp[0, 40:43] = (255, 255, 255, 0)
    idx = R.harness_dither(lib, ramp, pal, "diffusion")[1]
    assert (idx[0, 40:43] == 2).all() and (idx[0, :40] < 2).all() and (idx[0, 43:] < 2).all()
    assert np.array_equal(idx[:, 43:], R.harness_dither(lib, np.ascontiguousarray(ramp[:, 43:]), pal, "diffusion")[1])
    assert not np.array_equal(R.harness_dither(lib, solid, pal, "diffusion")[1][:, 43:], idx[:, 43:])   # (the error does get there otherwise)
    # the X = 0 entry is the plain route's choice, also when no entry is transparent
    assert (R.harness_dither(lib, ramp, _greys(255, 0), "diffusion")[1][0, 40:43] == 1).all()


def test_bad_arguments_never_reach_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_abi.Context, "get", classmethod(no_device))
    img = _noise(4, 5, 1)
    layer = S.Layer(np.zeros((2, 2, 4)), (0, 0), pre_alpha=True, linear_rgb=True)
    for bad in ("floyd", "Ordered", "", "fs"):
        for call in (lambda: S.quantize(img, dither=bad), lambda: S.canvas_to_png(img, palette=True, dither=bad),
                     lambda: layer.write_png(palette=16, dither=bad), lambda: S.render_svg("no/such/file.svg", palette=True, dither=bad)):
            with pytest.raises(ValueError, match="none.*ordered.*diffusion"):
                call()
    for bad in (1, True, False, 0.5, ("ordered",), b"ordered"):
        for call in (lambda: S.quantize(img, dither=bad), lambda: S.canvas_to_png(img, palette=True, encoder="device", dither=bad),
                     lambda: layer.write_png(palette=16, dither=bad), lambda: S.render_svg("no/such/file.svg", palette=True, dither=bad)):
            with pytest.raises(TypeError, match="dither"):
                call()
    for mode in MODES:
        for palette in (None, False):
            for call in (lambda: S.canvas_to_png(img, palette=palette, dither=mode), lambda: layer.write_png(palette=palette, dither=mode),
                         lambda: S.render_svg("no/such/file.svg", palette=palette, dither=mode)):
                with pytest.raises(ValueError, match="palette"):
                    call()
    with pytest.raises(ValueError, match="max_colors"):   # (the other arguments are still looked at)
        S.quantize(img, max_colors=1, dither="ordered")
    with pytest.raises(ValueError, match="paeth"):
        S.canvas_to_png(img, palette=True, encoder="device", filter="paeth", dither="diffusion")


def test_no_dither_is_the_plain_file():
    img = np.zeros((3, 4, 4), dtype=np.uint8)
    want = S.canvas_to_png(img).getvalue()
    assert S.canvas_to_png(img, dither=None).getvalue() == want == S.canvas_to_png(img, dither="none").getvalue()


def test_abi_and_exports(lib):
    names = ("svgr_quant_dither", "svgr_dither_tile_rows", "svgr_dither_tile_cols")
    hdr = open(os.path.join(ROOT, "include", "svgr.h")).read()
    so = _abi.load_library()
    assert so.svgr_abi_version() == 6 and "#define SVGR_ABI_VERSION 6" in hdr
    for name in names:
        assert name in _abi.EXPORTS and re.search(rf"\b{name}\s*\(", hdr) and hasattr(so, name)
    rows, cols = _abi.dither_tile()
    assert rows >= 2 and cols > 2 * (rows - 1)   # (what lets a tile's first row depend on two tiles above only)
    assert _abi.DITHER_MODES == {"ordered": lib.h_mode_ordered(), "diffusion": lib.h_mode_diffusion()}
    assert callable(quant.ordered_amplitude) and "quantize" in S.__all__


def test_harness_alone_under_the_sanitizers(tmp_path):
    # host code only, as a program of its own: nothing of it is loaded into this process
    exe = str(tmp_path / "dither_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-DDITHER_HARNESS_MAIN", "-o", exe, os.path.join(ROOT, "tests", "dither_harness.cpp")])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and "dither harness: 1008 runs" in done.stdout and not done.stderr, done.stderr
