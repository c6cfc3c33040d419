// svgr_png.cpp -- the scanline filters of a PNG image reversed on the host (png.py reads the chunks and inflates).
//
// Each filtered byte depends on the reconstructed byte to its left and the one above it (PNG spec, section 9), so the
// work is a sequential walk over the bytes: native, like the stroker, and linked into the same library.  Interlaced
// images call this once per Adam7 pass.
#include <cstdint>
#include <cstdlib>

#include "../../include/svgr.h"

namespace {

inline uint8_t paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    if (pa <= pb && pa <= pc) return (uint8_t)a;
    return (uint8_t)(pb <= pc ? b : c);
}

}  // namespace

extern "C" {

int svgr_png_unfilter(const uint8_t* src, int64_t src_bytes, int64_t rows, int64_t row_bytes, int64_t bytes_per_pixel,
                      uint8_t* dst) {
    if (!src || !dst || rows < 0 || row_bytes < 0 || bytes_per_pixel < 1 || bytes_per_pixel > 8 ||
        row_bytes > ((int64_t)1 << 40) || rows > ((int64_t)1 << 40))
        return SVGR_E_INVALID;
    if (src_bytes < 0 || src_bytes / (row_bytes + 1) < rows) return SVGR_E_INVALID;   // (never reads past src)
    const int64_t bpp = bytes_per_pixel;
    for (int64_t r = 0; r < rows; ++r) {
        const uint8_t f = src[r * (row_bytes + 1)];
        const uint8_t* in = src + r * (row_bytes + 1) + 1;
        uint8_t* out = dst + r * row_bytes;
        const uint8_t* up = r > 0 ? out - row_bytes : nullptr;   // (the first row's "above" is all zeros)
        switch (f) {
        case 0:
            for (int64_t i = 0; i < row_bytes; ++i) out[i] = in[i];
            break;
        case 1:
            for (int64_t i = 0; i < row_bytes; ++i) out[i] = (uint8_t)(in[i] + (i >= bpp ? out[i - bpp] : 0));
            break;
        case 2:
            for (int64_t i = 0; i < row_bytes; ++i) out[i] = (uint8_t)(in[i] + (up ? up[i] : 0));
            break;
        case 3:
            for (int64_t i = 0; i < row_bytes; ++i) {
                const int a = i >= bpp ? out[i - bpp] : 0, b = up ? up[i] : 0;
                out[i] = (uint8_t)(in[i] + ((a + b) >> 1));
            }
            break;
        case 4:
            for (int64_t i = 0; i < row_bytes; ++i) {
                const int a = i >= bpp ? out[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
                out[i] = (uint8_t)(in[i] + paeth(a, b, c));
            }
            break;
        default:
            return SVGR_E_INVALID;
        }
    }
    return SVGR_OK;
}

}  // extern "C"
