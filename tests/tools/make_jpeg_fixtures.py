#!/usr/bin/env python3
"""Writes the JPEG fixtures of tests/golden/jpeg: small files that cover the reader's matrix, each beside the pixels Pillow
(libjpeg-turbo) decodes from it, as NAME.jpg + NAME.npy ((h, w) uint8 for grey, (h, w, 3) for colour).  The tests read the
committed files only; this script needs Pillow and is run by hand when the matrix changes:
    python tests/tools/make_jpeg_fixtures.py
The source images are synthetic (seeded gradients, shapes and noise); nothing is copied from anywhere."""
import io
import os
import struct

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "jpeg")


def picture(h, w, seed, noise=6.0):
    """Gradients, a disc, a few hard edges and some noise: smooth areas, sharp chroma edges and texture in one image."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    img = np.stack([255 * u, 255 * v, 255 * (1 - 0.5 * u - 0.5 * v)], axis=-1)
    disc = (x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2 < (0.25 * min(h, w)) ** 2
    img[disc] = (230, 40, 60)
    img[(x > 0.15 * w) & (x < 0.3 * w) & (y > 0.55 * h)] = (20, 200, 240)
    img[(y > 0.8 * h) & (x > 0.5 * w)] = (250, 250, 250)
    img[(y < 0.12 * h) & (x < 0.2 * w)] = (0, 0, 0)
    img += rng.normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(rgb, grey=False, **options):
    im = Image.fromarray(rgb)
    if grey:
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **options)
    return buf.getvalue()


def segments(data):
    """[(marker code, start, end)] of the segments in front of the first scan"""
    out, pos = [], 2
    while data[pos + 1] != 0xDA:
        (length,) = struct.unpack(">H", data[pos + 2:pos + 4])
        out.append((data[pos + 1], pos, pos + 2 + length))
        pos += 2 + length
    out.append((0xDA, pos, pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]))
    return out


def without_jfif(data):
    for code, start, end in segments(data):
        if code == 0xE0:
            return data[:start] + data[end:]
    return data


def with_adobe(data, transform):
    """An APP14 Adobe segment with the given transform byte in place of the JFIF one (decoders give JFIF precedence)."""
    data = without_jfif(data)
    body = b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform)
    return data[:2] + b"\xff\xee" + struct.pack(">H", 2 + len(body)) + body + data[2:]


def with_component_ids(data, ids):
    """The component identifiers of the frame and scan headers replaced (a baseline file with one interleaved scan)."""
    data = bytearray(without_jfif(data))
    for code, start, _end in segments(bytes(data)):
        if code in (0xC0, 0xC1, 0xC2):
            for i, cid in enumerate(ids):
                data[start + 10 + 3 * i] = cid
        if code == 0xDA:
            for i, cid in enumerate(ids):
                data[start + 5 + 2 * i] = cid
    return bytes(data)


def as_440(data):
    """Pillow writes no 4:4:0.  A 4:2:2 file of w x h has the same blocks per MCU (two of luma, one of each chroma) and as
    many MCUs (ceil(w / 16) ceil(h / 8)) as a 4:4:0 file of h x w, so swapping the luma sampling factors and the size in
    the frame header turns it into a valid 4:4:0 stream (of a scrambled picture, which does not matter here)."""
    data = bytearray(data)
    for code, start, _end in segments(bytes(data)):
        if code == 0xC0:
            height, width = struct.unpack(">HH", data[start + 5:start + 9])
            assert data[start + 11] == 0x21
            data[start + 5:start + 9] = struct.pack(">HH", width, height)
            data[start + 11] = 0x12
    return bytes(data)


def main():
    os.makedirs(OUT, exist_ok=True)
    small = picture(40, 50, 1)
    coarse = [[min(16 + 40 * (i // 8 + i % 8), 1200) for i in range(64)], [min(30 + 70 * (i // 8 + i % 8), 2000) for i in range(64)]]
    files = {
        "grey_baseline": encode(small, grey=True, quality=90),
        "grey_progressive": encode(small, grey=True, quality=85, progressive=True),
        "ycc444_baseline": encode(small, quality=90, subsampling=0),
        "ycc422_baseline": encode(small, quality=90, subsampling=1),
        "ycc420_baseline": encode(small, quality=90, subsampling=2),
        "ycc444_progressive": encode(small, quality=85, subsampling=0, progressive=True),
        "ycc422_progressive": encode(small, quality=85, subsampling=1, progressive=True),
        "ycc420_progressive": encode(small, quality=85, subsampling=2, progressive=True),
        "ycc420_optimised": encode(small, quality=75, subsampling=2, optimize=True),
        "ycc420_restart": encode(small, quality=90, subsampling=2, restart_marker_blocks=2),
        "ycc444_restart_rows": encode(small, quality=90, subsampling=0, restart_marker_rows=1),
        "ycc420_progressive_restart": encode(small, quality=85, subsampling=2, progressive=True, restart_marker_blocks=3),
        "ycc420_33x17": encode(picture(17, 33, 2), quality=90, subsampling=2),
        "ycc422_progressive_31x23": encode(picture(23, 31, 3), quality=90, subsampling=1, progressive=True),
        "ycc420_1x1": encode(picture(1, 1, 4), quality=90, subsampling=2),
        "ycc420_7x5": encode(picture(5, 7, 5), quality=90, subsampling=2),
        "grey_3x8": encode(picture(8, 3, 6), grey=True, quality=90),
        "ycc444_low_quality": encode(small, quality=12, subsampling=0),
        "ycc420_photo": encode(picture(192, 256, 7, noise=14.0), quality=85, subsampling=2),
    }
    files["ycc440_from_422"] = as_440(encode(small, quality=90, subsampling=1))
    try:   # entries above 255 make the encoder write a 16-bit DQT and, with it, an extended sequential frame (SOF1)
        files["ycc420_dqt16_sof1"] = encode(small, subsampling=2, qtables=coarse)
    except (TypeError, ValueError, OSError) as e:
        print("no 16-bit DQT from this Pillow:", e)
    files["rgb_adobe"] = with_adobe(encode(small, quality=90, subsampling=0), 0)
    files["rgb_component_ids"] = with_component_ids(encode(small, quality=90, subsampling=0), b"RGB")
    files["ycc444_adobe_transform1"] = with_adobe(encode(small, quality=90, subsampling=0), 1)

    for name, data in sorted(files.items()):
        im = Image.open(io.BytesIO(data))
        im.load()
        pixels = np.asarray(im)
        assert pixels.dtype == np.uint8 and im.mode in ("L", "RGB")
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        np.save(os.path.join(OUT, name + ".npy"), pixels)
        sof = [f"SOF{c - 0xC0}" for c, _s, _e in segments(data) if 0xC0 <= c <= 0xC2]
        dqt16 = any(c == 0xDB and data[s + 4] >> 4 for c, s, _e in segments(data))
        print(f"{name}: {len(data)} bytes, {im.size[0]} x {im.size[1]} {im.mode} {sof[0]}{' 16-bit DQT' if dqt16 else ''}")


if __name__ == "__main__":
    main()
