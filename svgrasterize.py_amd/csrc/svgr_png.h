// svgr_png.h -- PNG scanline filters for writing (PNG 1.2 section 6), 8-bit RGBA: four bytes per pixel, one lane per pixel.
//
// Everything a lane does is integer arithmetic on one pixel and its three neighbours, compilable for the host (the CPU harness
// of tests/png_enc_harness.cpp) and for the device (k_png_filter of svgr_hip.hip).  DESIGN.md 7n has the definitions;
// tests/png_enc_ref.py restates them in numpy.
//
//   pixel      a little-endian uint32 as svgr_layer_to_rgba8 writes it: byte k of the pixel is bits 8k .. 8k + 7
//   neighbours a = the pixel to the left, b = the pixel above, c = the pixel above a.  The row above row 0 and the pixel left
//              of column 0 are zero
//   filters    0 None  x;  1 Sub  x - a;  2 Up  x - b;  3 Average  x - floor((a + b) / 2);  4 Paeth  x - paeth(a, b, c), all
//              modulo 256 per byte.  paeth: p = a + b - c, the nearest of a, b, c to p, ties in the order a, b, c
//   adaptive   libpng's heuristic: per row and filter type the sum over the filtered bytes (the type byte not among them) of
//              min(v, 256 - v); the smallest sum wins, a tie goes to the lower type number
//   stream     row r of the filtered stream F is its type byte and 4 * cols filtered bytes: rows * (1 + 4 * cols) bytes
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

constexpr int PNG_FILTER_NONE = 0, PNG_FILTER_SUB = 1, PNG_FILTER_UP = 2, PNG_FILTER_AVERAGE = 3, PNG_FILTER_PAETH = 4;
constexpr int PNG_FILTER_ADAPTIVE = 5;   // (no type of the format: the caller's request for the per-row choice)
constexpr int PNG_FILTER_TYPES = 5;

// The Paeth predictor of one byte.
PNG_HD int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// One byte x under filter `type` with the neighbours' bytes a, b, c.
PNG_HD int png_filter_byte(int type, int x, int a, int b, int c) {
    const int pred = type == PNG_FILTER_SUB ? a : type == PNG_FILTER_UP ? b : type == PNG_FILTER_AVERAGE ? (a + b) >> 1
                   : type == PNG_FILTER_PAETH ? png_paeth(a, b, c) : 0;
    return (x - pred) & 255;
}

// One pixel (four bytes) under filter `type`.
PNG_HD uint32_t png_filter_px(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t f = 0;
    for (int k = 0; k < 32; k += 8)
        f |= (uint32_t)png_filter_byte(type, (x >> k) & 255, (a >> k) & 255, (b >> k) & 255, (c >> k) & 255) << k;
    return f;
}

// What a filtered byte adds to its row's sum.
PNG_HD uint32_t png_cost_byte(int v) { return (uint32_t)(v < 256 - v ? v : 256 - v); }
PNG_HD uint32_t png_cost_px(uint32_t f) {
    return png_cost_byte(f & 255) + png_cost_byte((f >> 8) & 255) + png_cost_byte((f >> 16) & 255) + png_cost_byte(f >> 24);
}

// The adaptive choice from a row's five sums.
PNG_HD int png_pick(const uint32_t* sums) {
    int best = 0;
    for (int t = 1; t < PNG_FILTER_TYPES; ++t)
        if (sums[t] < sums[best]) best = t;
    return best;
}

// Pixel x of row `row`: its neighbours out of the image (src: rows * cols pixels).
PNG_HD void png_neighbours(const uint32_t* src, int64_t row, int64_t cols, int64_t x, uint32_t& px, uint32_t& a, uint32_t& b, uint32_t& c) {
    const uint32_t* cur = src + row * cols;
    px = cur[x];
    a = x ? cur[x - 1] : 0u;
    b = row ? cur[x - cols] : 0u;
    c = x && row ? cur[x - cols - 1] : 0u;
}

// The filtered pixel's four bytes at their place in the stream (byte stores: a row of F begins at an odd offset).
PNG_HD void png_store_px(uint8_t* out_row, int64_t x, uint32_t f) {
    uint8_t* o = out_row + 1 + 4 * x;
    o[0] = (uint8_t)f; o[1] = (uint8_t)(f >> 8); o[2] = (uint8_t)(f >> 16); o[3] = (uint8_t)(f >> 24);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Sample formats beyond 8-bit RGBA (svgr_png_samples, svgr_png_filter_bytes; DESIGN.md 7v has the definitions,
// tests/png_fmt_ref.py restates them in numpy, tests/png_fmt_harness.cpp drives them on the host).
//
//   colour   the PNG colour types 0 grey, 2 RGB, 4 grey + alpha, 6 RGBA, at depth 8 or 16: bpp = channels * depth / 8 bytes a
//            pixel, one of 1, 2, 3, 4, 6, 8
//   source   a straight-alpha sRGB-encoded RGBA pixel in doubles (a converted layer), a one-channel mask value, or four bytes
//            (each v / 255.0)
//   sample   rint(v * M) saturated to [0, M], NaN giving 0, M = 255 or 65535; a 16-bit sample is stored most significant byte
//            first.  At M = 255 this is k_to_rgba8's rule
//   grey     y = (0.2126 * r + 0.7152 * g) + 0.0722 * b, every product and sum rounded on its own (no fused multiply-add), then
//            quantised like any sample.  The three weights sum to 1 in double and r = g = b = k / M comes back as k
//   filters  as above, with bytes in place of pixels: byte i of a row has a = row[i - bpp], b = above[i], c = above[i - bpp],
//            zero outside the image
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int PNG_COLOR_GREY = 0, PNG_COLOR_RGB = 2, PNG_COLOR_GREY_ALPHA = 4, PNG_COLOR_RGBA = 6;
constexpr int PNG_SRC_RGBA_F64 = 0, PNG_SRC_MASK_F64 = 1, PNG_SRC_RGBA_U8 = 2;

// Samples per pixel of a colour type; 0 for a number that is none of the four.
PNG_HD int png_channels(int color) {
    return color == PNG_COLOR_GREY ? 1 : color == PNG_COLOR_RGB ? 3 : color == PNG_COLOR_GREY_ALPHA ? 2 : color == PNG_COLOR_RGBA ? 4 : 0;
}
// Bytes per pixel; 0 for an unknown colour type or a depth that is neither 8 nor 16.
PNG_HD int png_bpp(int color, int depth) { return depth == 8 || depth == 16 ? png_channels(color) * (depth >> 3) : 0; }
PNG_HD bool png_bpp_ok(int bpp) { return bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8; }

// One sample: rint(v * max) saturated to [0, max]; NaN gives 0.
PNG_HD uint32_t png_quant(double v, int max) {
    const double r = rint(v * (double)max);
    return r > 0.0 ? (r < (double)max ? (uint32_t)r : (uint32_t)max) : 0u;   // (NaN fails r > 0)
}

// Rec. 709 luma of straight sRGB-encoded values: two sums and three products, each rounded once.  (clang honours the pragma on
// the host and the device; a GCC host build takes -ffp-contract=off, as every host build of these headers does.)
PNG_HD double png_luma(double r, double g, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double pr = 0.2126 * r, pg = 0.7152 * g, pb = 0.0722 * b;
    const double s = pr + pg;
    return s + pb;
}

// `n` samples (n <= 4) in file order as one word: byte k of the pixel in the file is bits 8k .. 8k + 7.
PNG_HD uint64_t png_pack_samples(const uint32_t* q, int n, int depth) {
    uint64_t s = 0;
    for (int j = 0; j < n; ++j)
        s |= depth == 16 ? (uint64_t)(((q[j] >> 8) & 255u) | ((q[j] & 255u) << 8)) << (16 * j) : (uint64_t)q[j] << (8 * j);
    return s;
}

// The sample bytes of one straight-alpha RGBA pixel (the caller has put a layer without alpha in the file over its background).
PNG_HD uint64_t png_samples_px(double r, double g, double b, double a, int color, int depth) {
    const int M = depth == 16 ? 65535 : 255;
    uint32_t q[4];
    int n = 0;
    if (color == PNG_COLOR_RGB || color == PNG_COLOR_RGBA) {
        q[0] = png_quant(r, M); q[1] = png_quant(g, M); q[2] = png_quant(b, M);
        n = 3;
    } else {
        q[0] = png_quant(png_luma(r, g, b), M);
        n = 1;
    }
    if (color == PNG_COLOR_GREY_ALPHA || color == PNG_COLOR_RGBA) q[n++] = png_quant(a, M);
    return png_pack_samples(q, n, depth);
}
// ... of one mask value (colour type 0 only).
PNG_HD uint64_t png_samples_px(double m, int depth) {
    const uint32_t q = png_quant(m, depth == 16 ? 65535 : 255);
    return png_pack_samples(&q, 1, depth);
}
// ... of four bytes R, G, B, A (a little-endian uint32): each v / 255.0.
PNG_HD uint64_t png_samples_px(uint32_t rgba, int color, int depth) {
    return png_samples_px((double)(rgba & 255u) / 255.0, (double)((rgba >> 8) & 255u) / 255.0, (double)((rgba >> 16) & 255u) / 255.0,
                          (double)(rgba >> 24) / 255.0, color, depth);
}

// Byte i of row `row` and its neighbours out of an image of rows * row_bytes bytes.
PNG_HD void png_neighbours_byte(const uint8_t* src, int64_t row, int64_t row_bytes, int bpp, int64_t i, int& x, int& a, int& b, int& c) {
    const uint8_t* cur = src + row * row_bytes;
    x = cur[i];
    a = i >= bpp ? cur[i - bpp] : 0;
    b = row ? cur[i - row_bytes] : 0;
    c = i >= bpp && row ? cur[i - row_bytes - bpp] : 0;
}

// A row's five sums (the adaptive choice is png_pick of them) and the row under one type, a byte at a time: the serial form of
// k_png_filter_bytes, which the host harness runs.
PNG_HD void png_row_sums_bytes(const uint8_t* src, int64_t row, int64_t row_bytes, int bpp, uint32_t* sums) {
    for (int t = 0; t < PNG_FILTER_TYPES; ++t) sums[t] = 0;
    for (int64_t i = 0; i < row_bytes; ++i) {
        int x, a, b, c;
        png_neighbours_byte(src, row, row_bytes, bpp, i, x, a, b, c);
        for (int t = 0; t < PNG_FILTER_TYPES; ++t) sums[t] += png_cost_byte(png_filter_byte(t, x, a, b, c));
    }
}
PNG_HD void png_filter_row_bytes(const uint8_t* src, int64_t row, int64_t row_bytes, int bpp, int type, uint8_t* out_row) {
    out_row[0] = (uint8_t)type;
    for (int64_t i = 0; i < row_bytes; ++i) {
        int x, a, b, c;
        png_neighbours_byte(src, row, row_bytes, bpp, i, x, a, b, c);
        out_row[1 + i] = (uint8_t)png_filter_byte(type, x, a, b, c);
    }
}
