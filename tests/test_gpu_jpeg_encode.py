"""JPEG output on the device: svgr_jpeg_encode (k_jpeg_planes + k_jpeg_fdct) against the host build of the same integer
arithmetic (tests/jpeg_enc_harness.cpp) -- bit for bit --, Layer.write_jpeg of a small rendered scene read back with read_jpeg,
and render_svg's format switch."""
import ctypes as C
import io

import numpy as np
import pytest

from tests import jpeg_enc_ref as E
from tests.jpeg_ref import _T

pytestmark = pytest.mark.gpu

SAMPLINGS = [None, "4:4:4", "4:2:2", "4:4:0", "4:2:0"]   # None: grey


@pytest.fixture(scope="module")
def S():
    import svgrasterize_amd as S

    S.Context.get()
    return S


@pytest.fixture(scope="module")
def eh():
    return E.harness()


def _tables(n_comp):
    rng = np.random.default_rng(11)
    return {"ones": np.ones((n_comp, 64), dtype=np.uint16), "max": np.full((n_comp, 64), 255, dtype=np.uint16),
            "mixed": rng.integers(1, 256, (n_comp, 64)).astype(np.uint16)}


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 17), (100, 259), (517, 130)])
def test_encode_equals_host_build(S, eh, size, sampling):
    """sizes whose block counts are no multiple of a workgroup's 32 blocks and whose sides are no multiple of the MCU (odd
    widths take the kernel's unaligned path, even ones its 8-byte loads), every sampling and grey, the extreme images, tables
    of 1, of 255 and mixed"""
    from svgrasterize_amd import _abi

    ctx = _abi.Context.get()
    frame = E.frame_of(*size, sampling)
    tables = _tables(frame.n_comp)
    for k, (name, img) in enumerate(E.images(*size).items()):
        dev = ctx.from_host(img)
        for kind in (("ones", "max", "mixed") if name == "random" else (("ones", "max", "mixed")[k % 3],)):
            got = _abi.jpeg_encode(ctx, frame, dev, tables[kind])
            want = E.harness_coefficients(eh, frame, img, tables[kind])
            assert got.dtype == np.int16 and got.shape == want.shape
            assert np.array_equal(got, want), f"{name}, {kind}: {int((got != want).sum())} coefficients differ"
    # a host array goes the same way (uploaded first), and an even width one wider takes the aligned loads
    img = E.images(size[0], size[1] + 1)["random"]
    frame = E.frame_of(size[0], size[1] + 1, sampling)
    assert np.array_equal(_abi.jpeg_encode(ctx, frame, img, tables["mixed"]), E.harness_coefficients(eh, frame, img, tables["mixed"]))


def _scene_layer(S, w=64, h=48):
    from svgrasterize_amd.geometry import Transform

    body = ('<defs><linearGradient id="g" x1="0" y1="0" x2="1" y2="1"><stop offset="0" stop-color="#e02010"/>'
            '<stop offset="1" stop-color="#1040f0"/></linearGradient></defs>'
            '<rect x="4" y="3" width="50" height="40" fill="url(#g)"/>'
            '<circle cx="40" cy="26" r="17" fill="#20c040" fill-opacity="0.5"/>')
    scene, _, _ = S.svg_scene_from_str(f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}">{body}</svg>')
    return scene.render(Transform().matrix(0, 1, 0, 1, 0, 0), viewport=[0, 0, h, w])[0].on_canvas(h, w)


def _round_trip_bound(quant):
    """The largest |difference| per channel (R, G, B) between a pixel and read_jpeg of its written file at 4:4:4, from the
    tables alone.

    Encoder: each of Y, Cb, Cr is rounded to 8 bits (<= 1/2, plus 3 * 255 * 2^-17 < 0.01 for the matrix's stored factors; the
    clamp only brings a value nearer).  A coefficient is the exact F / q rounded, off by <= 1/2, plus the transform table's
    2^-16 sum |s - 128| <= 2^-16 * 64 * 128 = 1/8, over q; dequantised, that is e(v, u) = q(v, u) / 2 + 1/8.  Decoder: sample
    (y, x) takes sum_vu |T[y][v] T[x][u]| e(v, u) of it (the basis amplitudes), its own table adds 2^-16 sum |F| <= 2^-16 * 8 *
    ||s - 128||_2 <= 2^-16 * 8 * 8 * 128 = 1/8, and the sample is rounded to 8 bits (<= 1/2; again the clamp only helps).  So a
    component is off by E_c = 0.51 + max_yx sum_vu |T T| e + 1/8 + 1/2.  The decoder's matrix is the inverse of the encoder's
    (JFIF's printed factors: to 1e-5 of 255 * 3), its stored factors add < 0.01, and its one rounding 1/2:
    R: E_0 + 1.402 E_2, G: E_0 + 0.344136 E_1 + 0.714136 E_2, B: E_0 + 1.772 E_1, each + 0.53.  Both sides are integers, so
    the difference is at most the floor of that."""
    a = np.abs(_T)   # [x][u]
    e_c = []
    for i in range(3):
        e = quant[i].reshape(8, 8).astype(np.float64) / 2.0 + 0.125
        e_c.append(0.51 + float(np.einsum("yv,vu,xu->yx", a, e, a).max()) + 0.125 + 0.5)
    return np.floor(np.array([e_c[0] + 1.402 * e_c[2], e_c[0] + 0.344136 * e_c[1] + 0.714136 * e_c[2], e_c[0] + 1.772 * e_c[1]]) + 0.53)


def test_layer_write_jpeg_round_trip(S):
    from svgrasterize_amd import jpeg

    layer = _scene_layer(S)
    bg = (0.2, 0.3, 0.1, 1.0)   # (premultiplied linear RGBA, opaque)
    want = layer.background(bg).to_rgba8()
    assert want.shape == (48, 64, 4) and (want[..., 3] == 255).all() and len(np.unique(want[..., 0])) > 20
    best = layer.write_jpeg(None, bg=bg, quality=100, subsampling="4:4:4")
    got = S.read_jpeg(best)
    bound = _round_trip_bound(jpeg.quant_tables(100)[[0, 1, 1]])
    err100 = np.abs(got[..., :3].astype(int) - want[..., :3].astype(int))
    print("quality 100, 4:4:4: max |difference| per channel", err100.max(axis=(0, 1)), "bound", bound)
    assert (err100.max(axis=(0, 1)) <= bound).all()
    # the default background is opaque white, and the module-level entry takes the layer too
    white = layer.write_jpeg(quality=100, subsampling="4:4:4")
    assert white == jpeg.write_jpeg(layer, quality=100, subsampling="4:4:4")
    corner = S.read_jpeg(white)[0, 0, :3].astype(int)
    assert (np.abs(corner - 255) <= bound).all()
    # a lower quality: a smaller file that is further from the pixels
    sink = io.BytesIO()
    small = layer.write_jpeg(sink, bg=bg, quality=50, subsampling="4:4:4")
    assert sink.getvalue() == small and len(small) < len(best)
    err50 = np.abs(S.read_jpeg(small)[..., :3].astype(int) - want[..., :3].astype(int))
    assert err50.mean() > err100.mean()
    # canvas_to_jpeg: the same bytes from the host array
    assert S.canvas_to_jpeg(want, quality=50, subsampling="4:4:4") == small
    # every sampling and grey decode to the layer's size
    for sampling in SAMPLINGS:
        out = S.read_jpeg(layer.write_jpeg(bg=bg, grey=sampling is None, subsampling=sampling or "4:2:0"))
        assert out.shape == (48, 64, 4)
        if sampling is None:
            assert (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()
    with pytest.raises(ValueError, match="quality"):
        layer.write_jpeg(quality=0)
    with pytest.raises(ValueError, match="subsampling"):
        layer.write_jpeg(subsampling="4:1:1")


def test_render_svg_formats(S, tmp_path):
    """The document is built so that two 16 x 16 MCUs are of one colour: (0, 0) lies inside an opaque rectangle whose edges are
    MCU edges, and the last column of MCUs (x >= 48) shows the background alone, padding included (the edge rule repeats it).
    A block of one value has no AC (the table's columns other than the first sum to zero, term against term), its DC comes back
    within q / 2 <= 2 at quality 90 and above, i.e. the sample within 1/4 of an integer: every component of such an MCU decodes
    exactly, and a pixel away from the MCU's edge takes its chroma from that MCU alone.  There the decoded pixel is the colour
    matrix there and back of the PNG route's pixel: each of Y, Cb, Cr rounded (0.51 with the stored factors' share), the inverse
    matrix's stored factors and one rounding (0.53): R 0.51 (1 + 1.402) + 0.53 = 1.76, G 0.51 (1 + 0.344136 + 0.714136) + 0.53
    = 1.58, B 0.51 (1 + 1.772) + 0.53 = 1.94, so integers at most 1 apart; white (Y 255, Cb = Cr = 128) and black are exact."""
    from svgrasterize_amd import jpeg

    doc = tmp_path / "doc.svg"
    doc.write_text('<svg xmlns="http://www.w3.org/2000/svg" width="56" height="30"><rect x="0" y="0" width="16" height="16" fill="#c03020"/>'
                   '<circle cx="30" cy="18" r="9" fill="#2040c0" fill-opacity="0.6"/></svg>')
    png = S.render_svg(str(doc))
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    assert S.render_svg(str(doc), tmp_path / "out.png") == png and (tmp_path / "out.png").read_bytes() == png
    assert S.render_svg(str(doc), format="png") == png and S.render_svg(str(doc), tmp_path / "named.jpg", format="png") == png
    sink = io.BytesIO()
    assert S.render_svg(str(doc), sink) == png and sink.getvalue() == png   # (a file object: PNG unless told otherwise)

    for kw, path in (({"format": "jpeg"}, None), ({}, tmp_path / "Out.JPG"), ({}, str(tmp_path / "out.jpeg")), ({}, tmp_path / "o.jpe")):
        data = S.render_svg(str(doc), path, **kw)
        codes = [c for _o, c, _b in jpeg.markers(data)]
        assert codes[:2] == [0xD8, 0xE0] and codes[-1] == 0xD9
        frame, _coef, quant = jpeg.decode_coefficients(data)
        assert (frame.width, frame.height, frame.n_comp) == (56, 30, 3) and (frame.h[0], frame.v[0]) == (2, 2)
        assert np.array_equal(quant, jpeg.quant_tables(90)[[0, 1, 1]])
        if path is not None:
            assert open(path, "rb").read() == data
    px = S.read_jpeg(data)
    ref = S.read_png(png)
    assert px.shape == ref.shape == (30, 56, 4)
    assert (ref[:16, :16, 3] == 255).all() and abs(int(ref[6, 6, 0]) - 0xc0) <= 1 and ref[4, 52, 3] == 0
    assert (px[2:28, 50:55, :3] == 255).all()                      # (no bg: opaque white where the PNG is transparent)
    assert (np.abs(px[2:14, 2:14, :3].astype(int) - ref[2:14, 2:14, :3].astype(int)) <= 1).all()
    dark = S.read_jpeg(S.render_svg(str(doc), format="jpeg", bg=(0.0, 0.0, 0.0, 1.0), quality=95, subsampling="4:4:4"))
    assert (dark[2:28, 50:55, :3] == 0).all()
    assert (np.abs(dark[2:14, 2:14, :3].astype(int) - ref[2:14, 2:14, :3].astype(int)) <= 1).all()
    frame, _coef, quant = jpeg.decode_coefficients(S.render_svg(str(doc), format="jpeg", quality=60, subsampling="4:2:2"))
    assert (frame.h[0], frame.v[0]) == (2, 1) and np.array_equal(quant[0], jpeg.quant_tables(60)[0])
    with pytest.raises(ValueError, match="format"):
        S.render_svg(str(doc), format="gif")


def test_encode_rejects_nonsense(S):
    from svgrasterize_amd import _abi

    ctx = _abi.Context.get()
    frame = E.frame_of(9, 17, "4:2:0")
    quant = np.ones((3, 64), dtype=np.uint16)
    src = ctx.from_host(np.zeros((9, 17, 4), dtype=np.uint8))
    n = _abi.jpeg_n_coef(frame)
    coef = np.zeros(n + 64, dtype=np.int16)

    def rc(frame=frame, src=src, quant=quant, n=n):
        return ctx.lib.svgr_jpeg_encode(ctx.handle, C.byref(frame), src.handle, _abi.ptr(quant), _abi.ptr(coef), n)

    assert rc() == 0
    rgb = E.frame_of(9, 17, "4:2:0")
    rgb.colour = _abi.JPEG_RGB
    assert rc(frame=rgb) == -1
    grey3 = E.frame_of(9, 17, "4:4:4")
    grey3.colour = _abi.JPEG_GREY
    assert rc(frame=grey3) == -1
    chroma2 = E.frame_of(9, 17, "4:4:4")
    chroma2.h[1] = 2
    assert rc(frame=chroma2, n=_abi.jpeg_n_coef(chroma2)) == -1
    assert rc(src=ctx.alloc(9 * 17 * 4 - 4)) == -1
    assert rc(n=n - 64) == -1 and rc(n=n + 64) == -1
    for bad in (0, 256):
        q = quant.copy()
        q[2, 63] = bad
        assert rc(quant=q) == -1
    with pytest.raises(ValueError, match="table entry"):
        _abi.jpeg_encode(ctx, frame, src, q)
    with pytest.raises(ValueError):
        _abi.jpeg_encode(ctx, frame, np.zeros((9, 16, 4), dtype=np.uint8), quant)
