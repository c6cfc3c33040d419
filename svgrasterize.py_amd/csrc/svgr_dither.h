// svgr_dither.h -- dithering for indexed PNG output: the target a pixel is matched at under ordered dithering and under
// Floyd-Steinberg error diffusion, and the sequential form of both.
//
// Like svgr_quant.h, which it builds on: integer arithmetic on one pixel, compilable for the host (tests/dither_harness.cpp) and
// for the device (k_quant_dither_* of svgr_hip.hip), so every result is defined to the bit.  DESIGN.md 7u has the definitions;
// tests/dither_ref.py restates them in numpy.
//
//   coordinates  both modes work on X(p) = (r a, g a, b a, 255 a) of the canonical pixel; a target t is X moved and clamped to
//                0 .. 65025 per coordinate, so quant_dist's 32-bit squares still hold; the pixel takes quant_nearest(t)
//   ordered      B = the 8 x 8 Bayer matrix (0 .. 63) at (row & 7, col & 7); h = amp * a / 255; off = (((2 B + 1) h) >> 7) -
//                (h >> 1); t = (clamp(x0 + off), clamp(x1 + off), clamp(x2 + off), x3).  amp belongs to the palette
//                (quant.ordered_amplitude); a == 0 gives h = 0
//   diffusion    every row left to right; acc = 7 e(r, c-1) + 3 e(r-1, c+1) + 5 e(r-1, c) + e(r-1, c-1), int32, errors from
//                outside the image being 0; t = clamp(x + floor((acc + 8) / 16)) in all four coordinates; e = t - X(entry).  A
//                pixel with a == 0 takes the entry nearest to X = 0 and passes on e = 0
#pragma once
#include "svgr_quant.h"

constexpr int DITHER_ORDERED = 1, DITHER_DIFFUSION = 2;
constexpr int32_t DITHER_X_MAX = 65025;   // 255 * 255: the largest coordinate, and the largest amplitude

// B[row & 7][col & 7]: the recursion M -> [[4 M, 4 M + 2], [4 M + 3, 4 M + 1]] from [[0]], three times.  The cell of a 2 x 2 step is
// T(y, x) = 2 (y ^ x) + y; the lowest bits of (row, col) choose the cell of the first step, which the later ones multiply by 4.
QUANT_HD int dither_bayer(int64_t row, int64_t col) {
    int v = 0;
    for (int k = 0; k < 3; ++k) {
        const int y = (int)(row >> k) & 1, x = (int)(col >> k) & 1;
        v = 4 * v + 2 * (y ^ x) + y;
    }
    return v;
}

QUANT_HD uint32_t dither_clamp(int32_t v) { return v < 0 ? 0u : v > DITHER_X_MAX ? (uint32_t)DITHER_X_MAX : (uint32_t)v; }

// floor(v / 16) of a signed value (an arithmetic shift, spelled out)
QUANT_HD int32_t dither_floor16(int32_t v) { return v >= 0 ? v / 16 : -((15 - v) / 16); }

// ordered: the target of the pixel with the coordinates x and the alpha a at (row, col)
QUANT_HD void dither_ordered_target(const uint32_t* x, uint32_t a, uint32_t amp, int64_t row, int64_t col, uint32_t* t) {
    const int32_t h = (int32_t)(amp * a / 255u);   // (amp <= 65025, a <= 255: below 2^24)
    const int32_t off = (((2 * dither_bayer(row, col) + 1) * h) >> 7) - (h >> 1);
    for (int k = 0; k < 3; ++k) t[k] = dither_clamp((int32_t)x[k] + off);
    t[3] = x[3];
}

// diffusion: the target of the pixel with the coordinates x and the accumulated weighted errors acc (|acc| <= 16 * 65025)
QUANT_HD void dither_diffusion_target(const uint32_t* x, const int32_t* acc, uint32_t* t) {
    for (int k = 0; k < 4; ++k) t[k] = dither_clamp((int32_t)x[k] + dither_floor16(acc[k] + 8));
}

// One row of indices into the stream and / or the plain indices, as quant_index_rows stores them.
inline void dither_store_row(const uint8_t* idx_row, int64_t r, int64_t cols, int depth, uint8_t* stream, uint8_t* indices) {
    const int64_t rb = quant_row_bytes(cols, depth);
    if (indices)
        for (int64_t c = 0; c < cols; ++c) indices[r * cols + c] = idx_row[c];
    if (!stream) return;
    stream[r * rb] = 0;
    for (int64_t c0 = 0; c0 < cols; c0 += QUANT_RUN) {
        uint8_t bytes[8];
        const int n = (int)(cols - c0 < QUANT_RUN ? cols - c0 : QUANT_RUN);
        quant_pack_run(idx_row + c0, n, depth, bytes);
        const int nb = (n * depth + 7) / 8;
        for (int j = 0; j < nb; ++j) stream[r * rb + 1 + c0 * depth / 8 + j] = bytes[j];
    }
}

// Sequential form of svgr_quant_dither (the host side of the parity tests; the kernels compute the same).  `work` has room for
// cols bytes and, for diffusion, `acc` for 2 * 4 * (cols + 2) values.
inline void dither_rows(const uint32_t* src, int64_t rows, int64_t cols, const uint32_t* pal, int n_pal, int mode, uint32_t amp, uint8_t* stream,
                        uint8_t* indices, uint8_t* work, int32_t* acc) {
    uint32_t pal_x[4 * QUANT_MAX_COLORS];
    for (int i = 0; i < n_pal; ++i) quant_x(quant_canon(pal[i]), pal_x + 4 * i);
    const int depth = quant_depth(n_pal);
    const uint32_t zero[4] = {0, 0, 0, 0};
    const int clear = quant_nearest(pal_x, n_pal, zero);
    const int64_t stride = 4 * (cols + 2);   // a row of accumulators: columns -1 .. cols, what falls on the two ends is dropped
    if (mode == DITHER_DIFFUSION)
        for (int64_t i = 0; i < 2 * stride; ++i) acc[i] = 0;
    for (int64_t r = 0; r < rows; ++r) {
        int32_t* cur = acc + (r & 1) * stride + 4;
        int32_t* next = acc + ((r + 1) & 1) * stride + 4;
        for (int64_t c = 0; c < cols; ++c) {
            const uint32_t px = quant_canon(src[r * cols + c]);
            uint32_t x[4], t[4];
            quant_x(px, x);
            if (mode == DITHER_ORDERED) {
                dither_ordered_target(x, px >> 24, amp, r, c, t);
                work[c] = (uint8_t)quant_nearest(pal_x, n_pal, t);
                continue;
            }
            if (!px) {
                work[c] = (uint8_t)clear;
                continue;
            }
            dither_diffusion_target(x, cur + 4 * c, t);
            const int k = quant_nearest(pal_x, n_pal, t);
            work[c] = (uint8_t)k;
            for (int j = 0; j < 4; ++j) {
                const int32_t e = (int32_t)t[j] - (int32_t)pal_x[4 * k + j];
                cur[4 * (c + 1) + j] += 7 * e;
                next[4 * (c - 1) + j] += 3 * e;
                next[4 * c + j] += 5 * e;
                next[4 * (c + 1) + j] += e;
            }
        }
        if (mode == DITHER_DIFFUSION)
            for (int64_t i = -4; i < stride - 4; ++i) cur[i] = 0;   // (this row's becomes the row after next's)
        dither_store_row(work, r, cols, depth, stream, indices);
    }
}
