"""CPU-side checks of SVG <image>: the PNG reader over every colour type, bit depth, filter and Adam7 (against the encoded
arrays, and against PIL where it is installed), malformed input, the preserveAspectRatio placement of Scene.image, the
loader's <image> element and the scene plumbing of ImagePaint.  No GPU needed."""
import base64
import io
import os
import struct
import warnings

import numpy as np
import pytest

from svgrasterize_amd import _abi, read_png
from svgrasterize_amd.geometry import Transform
from svgrasterize_amd.layer import canvas_to_png
from svgrasterize_amd.paint import ImagePaint
from svgrasterize_amd.scene import RENDER_FILL, RENDER_TRANSFORM, Scene, _paint_arrays, image_placement
from svgrasterize_amd.svg import svg_scene_from_filepath, svg_scene_from_str
from tests import image_ref as R

# (colour type, bit depth) of the specification
FORMATS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8),
           (6, 16)]


def _case(color_type, depth, h, w, seed, trns=False):
    """(raw samples, palette, tRNS bytes, expected RGBA) of a seeded image."""
    rng = np.random.default_rng(seed)
    ch = R.CHANNELS[color_type]
    top = (1 << depth) - 1
    palette = trns_bytes = None
    if color_type == 3:
        n_pal = min(top + 1, 5 + seed % 7)
        samples = rng.integers(0, n_pal, (h, w, 1))
        palette = rng.integers(0, 256, (n_pal, 3))
        alpha = rng.integers(0, 256, max(n_pal - 2, 1)) if trns else None
        table = np.full((n_pal, 4), 255, dtype=np.uint8)
        table[:, :3] = palette
        if trns:
            table[:len(alpha), 3] = alpha
            trns_bytes = alpha.astype(np.uint8).tobytes()
        return samples, palette, trns_bytes, table[samples[..., 0]]
    samples = rng.integers(0, top + 1, (h, w, ch))
    want = np.empty((h, w, 4), dtype=np.uint8)
    if color_type in (0, 4):
        want[..., :3] = R.to8(samples[..., :1], depth)
    else:
        want[..., :3] = R.to8(samples[..., :3], depth)
    want[..., 3] = R.to8(samples[..., -1], depth) if color_type in (4, 6) else 255
    if trns and color_type in (0, 2):
        key = samples[h // 2, w // 2, :ch]
        trns_bytes = struct.pack(f">{ch}H", *[int(k) for k in key])
        want[np.all(samples == key, axis=2), 3] = 0
    return samples, palette, trns_bytes, want


def _pil_decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


@pytest.mark.parametrize("color_type, depth", FORMATS)
@pytest.mark.parametrize("width", [1, 7, 33])
@pytest.mark.parametrize("filters", [0, 1, 2, 3, 4, "mixed"])
def test_png_decode_matrix(color_type, depth, width, filters):
    samples, palette, trns, want = _case(color_type, depth, 9, width, seed=width * 31 + depth)
    data = R.encode_png(samples, color_type, depth, palette, trns, filters=filters, seed=width)
    got = read_png(data)
    assert got.dtype == np.uint8 and got.shape == (9, width, 4)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("color_type, depth", FORMATS)
@pytest.mark.parametrize("shape", [(1, 1), (7, 7), (13, 33), (3, 10)])
def test_png_adam7(color_type, depth, shape):
    samples, palette, trns, want = _case(color_type, depth, *shape, seed=shape[1] + depth, trns=True)
    data = R.encode_png(samples, color_type, depth, palette, trns, interlace=True, seed=depth)
    assert np.array_equal(read_png(data), want)


@pytest.mark.parametrize("color_type, depth", [(0, 1), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 2), (3, 8)])
def test_png_transparency_key(color_type, depth):
    samples, palette, trns, want = _case(color_type, depth, 11, 7, seed=5, trns=True)
    got = read_png(R.encode_png(samples, color_type, depth, palette, trns))
    assert np.array_equal(got, want)
    assert (got[..., 3] == 0).any() if color_type != 3 else True


@pytest.mark.parametrize("color_type, depth", [f for f in FORMATS if f[1] <= 8])
@pytest.mark.parametrize("interlace", [False, True])
def test_png_matches_pil(color_type, depth, interlace):
    # (no colour key on gray below 8 bits here: PIL does not apply it to 4-bit gray; test_png_transparency_key covers it)
    key = color_type in (2, 3) or (color_type == 0 and depth == 8)
    samples, palette, trns, want = _case(color_type, depth, 17, 7, seed=depth + color_type, trns=key)
    data = R.encode_png(samples, color_type, depth, palette, trns, interlace=interlace, seed=3)
    got = read_png(data)
    assert np.array_equal(got, want)
    assert np.array_equal(got, _pil_decode(data))


def test_png_ancillary_chunks_ignored():
    samples, _, _, want = _case(6, 8, 5, 6, seed=2)
    extra = [(b"gAMA", struct.pack(">I", 45455)), (b"sRGB", b"\x00"), (b"tEXt", b"Comment\x00hello"),
             (b"cHRM", bytes(32)), (b"iCCP", b"p\x00\x00" + bytes(8))]
    assert np.array_equal(read_png(R.encode_png(samples, 6, 8, extra_chunks=extra)), want)


@pytest.mark.parametrize("threads", [1, 4])
def test_write_png_round_trip(threads):
    rgba = R.random_rgba((37, 53), seed=11)
    buf = canvas_to_png(rgba, None, level=6, threads=threads)
    assert np.array_equal(read_png(buf.getvalue()), rgba)


def _good_png():
    samples, palette, trns, _ = _case(3, 4, 6, 9, seed=1)
    return R.encode_png(samples, 3, 4, palette, trns)


def test_png_malformed():
    good = _good_png()
    read_png(good)
    with pytest.raises(ValueError, match="signature"):
        read_png(b"\x89PNG\r\n\x1b\n" + good[8:])
    bad_crc = bytearray(good)
    bad_crc[8 + 8 + 3] ^= 1   # (a byte of the IHDR body)
    with pytest.raises(ValueError, match="CRC"):
        read_png(bytes(bad_crc))
    idat = good.index(b"IDAT")
    for cut in (idat + 10, len(good) - 20, len(good) - 5, 20):
        with pytest.raises(ValueError):
            read_png(good[:cut])
    with pytest.raises(ValueError, match="IHDR"):   # 16-bit palette: no such combination
        read_png(R.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 16, 3, 0, 0, 0)).join([good[:8], good[33:]]))
    with pytest.raises(ValueError):
        read_png(b"")


def test_png_bad_filter_byte():
    samples = np.random.default_rng(0).integers(0, 256, (4, 5, 4))
    stream = R.filter_rows(R.pack_rows(samples, 8), 4, [0, 1, 2, 3])
    raw = bytearray(stream)
    raw[2 * 21] = 5   # (row 2's filter type)
    data = (b"\x89PNG\r\n\x1a\n" + R.chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 4, 8, 6, 0, 0, 0)) +
            R.chunk(b"IDAT", __import__("zlib").compress(bytes(raw))) + R.chunk(b"IEND", b""))
    with pytest.raises(ValueError):
        read_png(data)
    lib = _abi.load_library()
    src = np.frombuffer(bytes(raw), dtype=np.uint8)
    dst = np.zeros((4, 20), dtype=np.uint8)
    assert lib.svgr_png_unfilter(src.ctypes.data_as(_abi._P), src.size, 4, 20, 4, dst.ctypes.data_as(_abi._P)) == -1
    ok = np.frombuffer(stream, dtype=np.uint8)
    assert lib.svgr_png_unfilter(ok.ctypes.data_as(_abi._P), ok.size, 4, 20, 4, dst.ctypes.data_as(_abi._P)) == 0
    assert np.array_equal(dst, samples.astype(np.uint8).reshape(4, 20))
    # a short source is refused, not read past
    assert lib.svgr_png_unfilter(ok.ctypes.data_as(_abi._P), ok.size - 1, 4, 20, 4, dst.ctypes.data_as(_abi._P)) == -1


def test_png_palette_index_beyond_plte():
    samples = np.array([[[0], [1], [2], [3]]])
    data = R.encode_png(samples, 3, 2, palette=[[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    with pytest.raises(ValueError, match="palette"):
        read_png(data)


# ------------------------------------------------------------------------------------------------------------------------
# placement (SVG 1.1 section 7.8)
# ------------------------------------------------------------------------------------------------------------------------
ALIGNS = [f"x{x}Y{y}" for x in ("Min", "Mid", "Max") for y in ("Min", "Mid", "Max")]


def _expect(size, vp, par):
    """Hand-derived (scale x, scale y, translate x, translate y) and the visible rectangle."""
    h, w = size
    x, y, vw, vh = vp
    if par == "none":
        return (vw / w, vh / h, x, y), (x, y, x + vw, y + vh)
    align, mode = par.split()
    s = min(vw / w, vh / h) if mode == "meet" else max(vw / w, vh / h)
    fx = {"Min": 0.0, "Mid": 0.5, "Max": 1.0}[align[1:4]]
    fy = {"Min": 0.0, "Mid": 0.5, "Max": 1.0}[align[5:8]]
    tx, ty = x + fx * (vw - s * w), y + fy * (vh - s * h)
    if mode == "meet":
        return (s, s, tx, ty), (tx, ty, tx + s * w, ty + s * h)
    return (s, s, tx, ty), (x, y, x + vw, y + vh)


@pytest.mark.parametrize("par", [f"{a} {m}" for a in ALIGNS for m in ("meet", "slice")] + ["none"])
@pytest.mark.parametrize("size", [(40, 10), (10, 40)])          # portrait, landscape image (h, w)
@pytest.mark.parametrize("vp", [(3, 5, 20, 60), (-2, 7, 50, 12)])  # landscape, portrait viewport (x, y, w, h)
def test_placement(par, size, vp):
    tr, visible = image_placement(size, *vp, par)
    (sx, sy, tx, ty), vis = _expect(size, vp, par)
    np.testing.assert_allclose(tr.m, [[sx, 0, tx], [0, sy, ty], [0, 0, 1]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(visible, vis, rtol=0, atol=1e-12)
    # the visible rectangle lies in the viewport and in the image
    x, y, vw, vh = vp
    h, w = size
    corners = tr(np.array([[0, 0], [w, h]], dtype=np.float64))
    assert visible[0] >= max(x, corners[0, 0]) - 1e-12 and visible[2] <= min(x + vw, corners[1, 0]) + 1e-12
    assert visible[1] >= max(y, corners[0, 1]) - 1e-12 and visible[3] <= min(y + vh, corners[1, 1]) + 1e-12


def test_placement_empty_and_invalid():
    assert image_placement((4, 4), 0, 0, 0, 10) is None
    assert image_placement((4, 4), 0, 0, 10, 0) is None
    assert Scene.image(R.random_rgba((4, 4), 0), 0, 0, 0, 5) is None
    with pytest.raises(ValueError):
        image_placement((4, 4), 0, 0, 10, 10, "xMidYMid stretch")
    tr, _ = image_placement((4, 4), 0, 0, 10, 20, "defer xMinYMax meet")
    np.testing.assert_allclose(tr.m[:2], [[2.5, 0, 0], [0, 2.5, 10]])


def test_scene_image_node():
    px = R.random_rgba((6, 8), 1)
    node = Scene.image(px, 1, 2, 16, 30, "xMidYMax slice", smooth=False)
    kind, (path, paint, rule) = node
    assert kind == RENDER_FILL and isinstance(paint, ImagePaint) and not paint.smooth
    assert np.array_equal(paint.pixels, px) and not paint.pixels.flags.writeable
    px[0, 0, 0] ^= 1
    assert not np.array_equal(paint.pixels, px)   # (a copy: editing the caller's array cannot reach the paint)
    np.testing.assert_allclose(paint.transform.m[:2], [[30 / 6, 0, 1 + (16 - 8 * 5) / 2], [0, 5, 2]])


# ------------------------------------------------------------------------------------------------------------------------
# loader
# ------------------------------------------------------------------------------------------------------------------------
def _png(h=5, w=7, seed=0):
    px = R.random_rgba((h, w), seed)
    return px, R.encode_png(px, 6, 8)


def _uri(data):
    return "data:image/png;base64," + base64.b64encode(data).decode()


def _doc(body, extra=""):
    return (f'<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" width="64" height="48" {extra}>'
            f"{body}</svg>")


def _leaves(scene):
    """(path, paint) of every FILL under the scene, with the node kinds passed on the way."""
    out = []

    def walk(s, kinds):
        kind, args = s
        if kind == RENDER_FILL:
            out.append((args[0], args[1], tuple(kinds)))
        elif kind == 2:
            for c in args:
                walk(c, kinds + [kind])
        else:
            walk(args[0], kinds + [kind])

    walk(scene, [])
    return out


@pytest.mark.parametrize("attr", ["href", "xlink:href"])
def test_loader_image_element(attr):
    px, data = _png()
    doc = _doc(f'<defs><clipPath id="c"><circle cx="10" cy="10" r="8"/></clipPath></defs>'
               f'<image id="im" {attr}="{_uri(data)}" x="3" y="4" width="21" height="10" opacity="0.5" '
               f'transform="rotate(10)" clip-path="url(#c)" preserveAspectRatio="xMaxYMin slice"/>'
               f'<rect id="r" x="3" y="4" width="21" height="10" opacity="0.5" transform="rotate(10)" clip-path="url(#c)"/>')
    scene, ids, size = svg_scene_from_str(doc)
    (img_path, paint, img_kinds), (rect_path, _, rect_kinds) = _leaves(scene)
    assert isinstance(paint, ImagePaint) and paint.smooth and np.array_equal(paint.pixels, px)
    assert img_kinds == rect_kinds and RENDER_TRANSFORM in img_kinds
    want_tr, _ = image_placement((5, 7), 3, 4, 21, 10, "xMaxYMin slice")
    np.testing.assert_allclose(paint.transform.m, want_tr.m)
    # slice: the visible rectangle is the viewport, the <rect>'s outline
    pts = lambda p: p.packed()[0][:, :4].reshape(-1, 2)
    np.testing.assert_allclose([pts(img_path).min(0), pts(img_path).max(0)], [pts(rect_path).min(0), pts(rect_path).max(0)])
    assert "im" in ids


def test_loader_image_sizes_and_rendering():
    px, data = _png(5, 10)
    uri = _uri(data)
    body = (f'<g style="image-rendering: pixelated"><image href="{uri}"/></g>'
            f'<image href="{uri}" width="30"/><image href="{uri}" height="15"/>'
            f'<image href="{uri}" width="10" height="10" preserveAspectRatio="bogus"/>')
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        scene, _, _ = svg_scene_from_str(_doc(body))
    assert any("preserveAspectRatio" in str(w.message) for w in rec)
    (p0, a, _), (p1, b, _), (p2, c, _), (p3, d, _) = _leaves(scene)
    assert not a.smooth and b.smooth and c.smooth
    np.testing.assert_allclose(a.transform.m[:2], [[1, 0, 0], [0, 1, 0]])        # intrinsic size
    np.testing.assert_allclose(b.transform.m[:2], [[3, 0, 0], [0, 3, 0]])        # height from the aspect ratio
    np.testing.assert_allclose(c.transform.m[:2], [[3, 0, 0], [0, 3, 0]])
    np.testing.assert_allclose(d.transform.m[:2], [[1, 0, 0], [0, 1, 2.5]])      # fell back to xMidYMid meet


def test_loader_relative_path(tmp_path):
    px, data = _png(4, 3, seed=9)
    (tmp_path / "pics").mkdir()
    (tmp_path / "pics" / "a.png").write_bytes(data)
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc('<image href="pics/a.png" width="6" height="8"/>'))
    scene, _, _ = svg_scene_from_filepath(str(doc))
    ((_, paint, _),) = _leaves(scene)
    assert np.array_equal(paint.pixels, px)
    # from a string there is no document directory: warn, skip
    with pytest.warns(UserWarning, match="not from a file"):
        assert svg_scene_from_str(_doc('<image href="pics/a.png" width="6" height="8"/>'))[0] is None


@pytest.mark.parametrize("href, why", [
    ("data:image/jpeg;base64,/9j/4AAQSkZJRgABAQ==", "unsupported image data"),
    ("http://example.com/a.png", "only data URIs"),
    ("https://example.com/a.png", "only data URIs"),
    ("missing.png", "not readable"),
    ("data:image/png;base64,iVBORw0KGgoAAAAN", "undecodable"),
])
def test_loader_skips_unusable_images(tmp_path, href, why):
    doc = tmp_path / "doc.svg"
    doc.write_text(_doc(f'<image href="{href}" width="6" height="8"/>'))
    with pytest.warns(UserWarning, match=why):
        scene, _, _ = svg_scene_from_filepath(str(doc))
    assert scene is None


def test_loader_zero_size_image():
    _px, data = _png()
    with pytest.warns(UserWarning, match="empty"):
        scene, _, _ = svg_scene_from_str(_doc(f'<image href="{_uri(data)}" width="0" height="8"/>'))
    assert scene is None


def test_loader_base64_whitespace():
    px, data = _png(3, 3)
    b64 = base64.b64encode(data).decode()
    spaced = "\n  ".join(b64[i:i + 16] for i in range(0, len(b64), 16))
    scene, _, _ = svg_scene_from_str(_doc(f'<image href="data:image/png;base64,{spaced}" width="6" height="6"/>'))
    ((_, paint, _),) = _leaves(scene)
    assert np.array_equal(paint.pixels, px)


# ------------------------------------------------------------------------------------------------------------------------
# scene plumbing
# ------------------------------------------------------------------------------------------------------------------------
def test_repr_is_short():
    node = Scene.image(R.random_rgba((300, 400), 2), 0, 0, 40, 30)
    text = repr(Scene.group([node, node.opacity(0.5)]))
    assert "ImagePaint(400x300, smooth)" in text and len(text) < 2000
    assert repr(ImagePaint(R.random_rgba((2, 3), 0), Transform(), False)) == "ImagePaint(3x2, nearest)"


def test_paint_arrays_include_pixels():
    node = Scene.image(R.random_rgba((5, 6), 3), 0, 0, 12, 10)
    arrays = []
    _paint_arrays(Scene.group([node, Scene.fill(node[1][0], np.array([1.0, 0, 0, 1]))]), arrays, set())
    assert any(a is node[1][1].pixels for a in arrays)


def test_scenedump_round_trip(tmp_path):
    from svgrasterize_amd import scenedump

    a = Scene.image(R.random_rgba((5, 6), 4), 1, 2, 12, 10, "xMinYMid slice")
    b = Scene.image(R.random_rgba((3, 2), 5), 0, 0, 4, 4, smooth=False).transform(Transform().rotate(0.3))
    scene = Scene.group([a, b])
    tree, arrays = scenedump.dump_scene(scene)
    path = os.path.join(tmp_path, "s.npz")
    np.savez(path, tree=__import__("json").dumps(tree), info="{}", **arrays)
    back, _info, _z = scenedump.load_scene(path)
    tree2, arrays2 = scenedump.dump_scene(back)
    assert scenedump.compare_dumps(tree, arrays, tree2, arrays2) == []
    for (_, p, _), (_, q, _) in zip(_leaves(scene), _leaves(back)):
        assert np.array_equal(p.pixels, q.pixels) and p.smooth == q.smooth
        np.testing.assert_array_equal(p.transform.m, q.transform.m)


def test_image_levels_layout():
    levels = _abi.image_levels(37, 53)
    assert levels[0] == (0, 37, 53) and levels[-1][1:] == (1, 1)
    assert [lv[1:] for lv in levels] == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
    assert all(levels[k + 1][0] == levels[k][0] + levels[k][1] * levels[k][2] for k in range(len(levels) - 1))
