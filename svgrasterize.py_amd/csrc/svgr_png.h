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
