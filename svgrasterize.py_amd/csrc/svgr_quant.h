// svgr_quant.h -- colour quantisation for indexed PNG output: the canonical pixel, the metric, the nearest palette entry, the bin
// key, the hash of the distinct-colour set and the packing of index rows.
//
// Everything a lane does is integer arithmetic on one pixel, compilable for the host (the CPU harness of
// tests/quant_harness.cpp) and for the device (k_quant_* of svgr_hip.hip).  DESIGN.md 7t has the definitions;
// tests/quant_ref.py restates them in numpy.
//
//   pixel      a little-endian uint32 as svgr_layer_to_rgba8 writes it: r = bits 0-7, g = 8-15, b = 16-23, a = 24-31, straight
//              alpha.  Canonical: a pixel with a == 0 is 0 (its colour cannot be seen)
//   metric     X(p) = (r * a, g * a, b * a, 255 * a), each 0 .. 65025; D(p, q) = the sum of the four squared differences.  One
//              square fits 32 bits (65025^2 < 2^32), their sum does not: D is unsigned 64-bit
//   nearest    the palette entry with the smallest D; a tie goes to the lowest index
//   bin        (r >> 3, g >> 3, b >> 3, a >> 3) of the canonical pixel, r in the highest bits: 20 bits
//   rows       depth = the smallest of 1, 2, 4, 8 with 2^depth >= the palette's length; a row of the stream is the filter byte 0
//              and ceil(cols * depth / 8) bytes, the indices MSB first, the last byte's unused low bits zero
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define QUANT_HD __host__ __device__ inline
#else
#define QUANT_HD inline
#endif

constexpr int QUANT_MAX_COLORS = 256;
constexpr int QUANT_BIN_BITS = 20;
constexpr uint32_t QUANT_BINS = 1u << QUANT_BIN_BITS;
constexpr int QUANT_HASH_BITS = 10;                       // the distinct-colour set: 1024 slots for at most 256 colours
constexpr uint32_t QUANT_SLOTS = 1u << QUANT_HASH_BITS;
constexpr uint32_t QUANT_EMPTY = 1u;                      // r = 1 with a = 0: no canonical pixel has this value
constexpr int QUANT_RUN = 8;                              // consecutive pixels of one lane: whole bytes at every depth

struct QuantBin { uint64_t n, s[4]; };                    // pixels of the bin, and the four sums of X over them

QUANT_HD uint32_t quant_canon(uint32_t px) { return (px >> 24) ? px : 0u; }

QUANT_HD void quant_x(uint32_t px, uint32_t* x) {
    const uint32_t a = px >> 24;
    x[0] = (px & 255u) * a;
    x[1] = ((px >> 8) & 255u) * a;
    x[2] = ((px >> 16) & 255u) * a;
    x[3] = 255u * a;
}

QUANT_HD uint64_t quant_dist(const uint32_t* x, const uint32_t* y) {
    uint64_t d = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t e = x[k] > y[k] ? x[k] - y[k] : y[k] - x[k];
        d += (uint64_t)(e * e);   // (e <= 65025: the product fits 32 bits)
    }
    return d;
}

// The nearest of the n entries whose coordinates are pal_x[4 * i .. 4 * i + 3] to the pixel with the coordinates x.
QUANT_HD int quant_nearest(const uint32_t* pal_x, int n, const uint32_t* x) {
    int best = 0;
    uint64_t best_d = quant_dist(x, pal_x);
    for (int i = 1; i < n; ++i) {
        const uint64_t d = quant_dist(x, pal_x + 4 * i);
        if (d < best_d) { best_d = d; best = i; }
    }
    return best;
}

QUANT_HD uint32_t quant_bin_key(uint32_t px) {
    const uint32_t c = quant_canon(px);
    return ((c & 255u) >> 3) << 15 | (((c >> 8) & 255u) >> 3) << 10 | (((c >> 16) & 255u) >> 3) << 5 | (c >> 27);
}

// Where a canonical pixel begins its probe of the distinct-colour set (it goes on to slot + 1, + 2, ... modulo QUANT_SLOTS).
QUANT_HD uint32_t quant_slot(uint32_t canon) { return (canon * 2654435761u) >> (32 - QUANT_HASH_BITS); }

QUANT_HD int quant_depth(int n_colors) { return n_colors <= 2 ? 1 : n_colors <= 4 ? 2 : n_colors <= 16 ? 4 : 8; }
QUANT_HD int64_t quant_row_bytes(int64_t cols, int depth) { return 1 + (cols * depth + 7) / 8; }

// The bytes of QUANT_RUN consecutive pixels' indices (the first `n` of idx count, the others pack as zero) at `depth`: depth
// bytes, out[0] first in the row.
QUANT_HD void quant_pack_run(const uint8_t* idx, int n, int depth, uint8_t* out) {
    const int per = 8 / depth;
    for (int j = 0; j < depth; ++j) {
        uint32_t v = 0;
        for (int k = 0; k < per; ++k) {
            const int i = j * per + k;
            v = (v << depth) | (i < n ? (uint32_t)idx[i] : 0u);
        }
        out[j] = (uint8_t)v;
    }
}

// Sequential forms of the three stages over n pixels (the host side of the parity tests; the kernels compute the same).
inline void quant_index_rows(const uint32_t* src, int64_t rows, int64_t cols, const uint32_t* pal, int n_pal, uint8_t* stream, uint8_t* indices) {
    uint32_t pal_x[4 * QUANT_MAX_COLORS];
    for (int i = 0; i < n_pal; ++i) quant_x(quant_canon(pal[i]), pal_x + 4 * i);
    const int depth = quant_depth(n_pal);
    const int64_t rb = quant_row_bytes(cols, depth);
    for (int64_t r = 0; r < rows; ++r) {
        if (stream) stream[r * rb] = 0;
        for (int64_t c0 = 0; c0 < cols; c0 += QUANT_RUN) {
            uint8_t idx[QUANT_RUN], bytes[8];
            const int n = (int)(cols - c0 < QUANT_RUN ? cols - c0 : QUANT_RUN);
            for (int k = 0; k < n; ++k) {
                uint32_t x[4];
                quant_x(quant_canon(src[r * cols + c0 + k]), x);
                idx[k] = (uint8_t)quant_nearest(pal_x, n_pal, x);
                if (indices) indices[r * cols + c0 + k] = idx[k];
            }
            quant_pack_run(idx, n, depth, bytes);
            const int nb = (n * depth + 7) / 8;
            if (stream)
                for (int j = 0; j < nb; ++j) stream[r * rb + 1 + c0 * depth / 8 + j] = bytes[j];
        }
    }
}
