// CPU harness for dithering: csrc/svgr_dither.h driven serially on the host.  The arithmetic is the header's own, so what this
// computes is the device's bit for bit.  tests/test_dither_host.py holds it against tests/dither_ref.py; with
// -DDITHER_HARNESS_MAIN it is a stand-alone program (for a run under a sanitizer) over the same palettes and shapes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_dither.h"

extern "C" {
int h_bayer(int row, int col) { return dither_bayer(row, col); }
int h_mode_ordered() { return DITHER_ORDERED; }
int h_mode_diffusion() { return DITHER_DIFFUSION; }
int h_depth(int n) { return quant_depth(n); }
int64_t h_row_bytes(int64_t cols, int depth) { return quant_row_bytes(cols, depth); }

// svgr_quant_dither: the row stream and / or the plain indices (either may be null)
void h_dither(const uint32_t* src, int64_t rows, int64_t cols, const uint32_t* pal, int n_pal, int mode, uint32_t amp, uint8_t* stream, uint8_t* indices) {
    std::vector<uint8_t> work((size_t)cols);
    std::vector<int32_t> acc(mode == DITHER_DIFFUSION ? (size_t)(2 * 4 * (cols + 2)) : 0);
    dither_rows(src, rows, cols, pal, n_pal, mode, amp, stream, indices, work.data(), acc.data());
}
}  // extern "C"

#ifdef DITHER_HARNESS_MAIN
int main() {
    uint32_t v = 2463534242u;
    auto next = [&]() { return v = v * 1664525u + 1013904223u; };
    unsigned long long sum = 0;
    int runs = 0;
    for (int n_pal : {1, 2, 3, 16, 17, 255, 256})
        for (int64_t cols : {1, 2, 7, 8, 9, 17})
            for (int64_t rows : {1, 2, 3, 9}) {
                std::vector<uint32_t> src((size_t)(rows * cols)), pal((size_t)n_pal);
                for (auto& p : src) {
                    p = next();
                    if ((p & 7u) == 0) p &= 0x00FFFFFFu;        // transparent, with stray colour
                    else if ((p & 7u) == 1) p |= 0xFF000000u;   // opaque
                }
                for (auto& p : pal) p = next() | ((next() & 1u) ? 0xFF000000u : 0u);
                std::vector<uint8_t> stream((size_t)(rows * quant_row_bytes(cols, quant_depth(n_pal)))), idx((size_t)(rows * cols));
                for (int mode : {DITHER_ORDERED, DITHER_DIFFUSION})
                    for (uint32_t amp : {0u, 5000u, 65025u}) {
                        h_dither(src.data(), rows, cols, pal.data(), n_pal, mode, amp, stream.data(), idx.data());
                        for (uint8_t b : stream) sum += b;
                        for (uint8_t b : idx) sum += b;
                        ++runs;
                    }
            }
    std::printf("dither harness: %d runs, checksum %llu\n", runs, sum);
    return 0;
}
#endif
