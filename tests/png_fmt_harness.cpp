// CPU harness for the PNG sample formats: the second part of csrc/svgr_png.h driven serially on the host -- one loop iteration
// where k_png_samples has one lane, one byte where k_png_filter_bytes has a quarter of a lane.  The arithmetic is the header's
// own, so the bytes this writes are the device's.  tests/test_png_formats_host.py holds it against tests/png_fmt_ref.py; with
// -DPNG_FMT_HARNESS_MAIN it is a stand-alone program (for a run under a sanitizer).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_png.h"

extern "C" {

void h_quant(const double* v, int64_t n, int max, uint32_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = png_quant(v[i], max);
}
void h_luma(const double* rgb, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = png_luma(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}
int h_bpp(int color, int depth) { return png_bpp(color, depth); }

// svgr_png_samples, serially: n_px pixels of `src` (what `kind` says) to n_px * bpp bytes.  Returns 0, or -1 for arguments the
// entry refuses.
int h_samples(const void* src, int kind, int64_t n_px, int color, int depth, uint8_t* dst) {
    const int bpp = png_bpp(color, depth);
    if (!bpp || kind < PNG_SRC_RGBA_F64 || kind > PNG_SRC_RGBA_U8 || (kind == PNG_SRC_MASK_F64 && color != PNG_COLOR_GREY)) return -1;
    for (int64_t i = 0; i < n_px; ++i) {
        uint64_t s;
        if (kind == PNG_SRC_RGBA_F64) {
            const double* p = (const double*)src + 4 * i;
            s = png_samples_px(p[0], p[1], p[2], p[3], color, depth);
        } else if (kind == PNG_SRC_MASK_F64) {
            s = png_samples_px(((const double*)src)[i], depth);
        } else {
            uint32_t px;
            memcpy(&px, (const uint8_t*)src + 4 * i, 4);
            s = png_samples_px(px, color, depth);
        }
        for (int k = 0; k < bpp; ++k) dst[i * bpp + k] = (uint8_t)(s >> (8 * k));
    }
    return 0;
}

// svgr_png_filter_bytes, serially
int h_filter_bytes(const uint8_t* src, int64_t rows, int64_t row_bytes, int bpp, int mode, uint8_t* out) {
    if (!png_bpp_ok(bpp) || row_bytes <= 0 || row_bytes % bpp || mode < 0 || mode > PNG_FILTER_ADAPTIVE) return -1;
    for (int64_t r = 0; r < rows; ++r) {
        int type = mode;
        if (mode == PNG_FILTER_ADAPTIVE) {
            uint32_t sums[PNG_FILTER_TYPES];
            png_row_sums_bytes(src, r, row_bytes, bpp, sums);
            type = png_pick(sums);
        }
        png_filter_row_bytes(src, r, row_bytes, bpp, type, out + r * (1 + row_bytes));
    }
    return 0;
}

}  // extern "C"

#ifdef PNG_FMT_HARNESS_MAIN
// Every format over a few pixels and every filter at every pixel size, for a run under a sanitizer: prints a checksum.
int main() {
    const int colors[] = {PNG_COLOR_GREY, PNG_COLOR_RGB, PNG_COLOR_GREY_ALPHA, PNG_COLOR_RGBA}, bpps[] = {1, 2, 3, 4, 6, 8};
    const int64_t n = 301;
    std::vector<double> f64((size_t)n * 4);
    std::vector<uint8_t> u8((size_t)n * 4);
    for (size_t i = 0; i < f64.size(); ++i) {
        f64[i] = (double)((i * 37) % 1031) / 1000.0 - 0.01;
        u8[i] = (uint8_t)(i * 29 >> 2);
    }
    uint64_t sum = 0;
    for (int color : colors)
        for (int depth = 8; depth <= 16; depth += 8)
            for (int kind = 0; kind < 3; ++kind) {
                std::vector<uint8_t> dst((size_t)(n * png_bpp(color, depth)));
                const void* src = kind == PNG_SRC_RGBA_U8 ? (const void*)u8.data() : (const void*)f64.data();
                if (h_samples(src, kind, n, color, depth, dst.data()) != (kind == PNG_SRC_MASK_F64 && color != PNG_COLOR_GREY ? -1 : 0)) return 1;
                for (uint8_t b : dst) sum = sum * 31 + b;
            }
    for (int bpp : bpps) {
        const int64_t rows = 5, row_bytes = 67 * bpp;
        std::vector<uint8_t> img((size_t)(rows * row_bytes)), out((size_t)(rows * (1 + row_bytes)));
        for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)(i * 31 >> 4);
        for (int mode = 0; mode <= PNG_FILTER_ADAPTIVE; ++mode) {
            if (h_filter_bytes(img.data(), rows, row_bytes, bpp, mode, out.data())) return 1;
            for (uint8_t b : out) sum = sum * 31 + b;
        }
    }
    printf("formats ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
