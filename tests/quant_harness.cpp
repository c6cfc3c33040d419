// CPU harness for the colour quantiser: csrc/svgr_quant.h driven serially on the host -- one loop iteration where the kernels of
// svgr_hip.hip have one lane.  The arithmetic is the header's own, so what this computes is the device's bit for bit: the set of
// distinct colours, the bins and the index rows.  tests/test_quant_host.py holds it against tests/quant_ref.py; with
// -DQUANT_HARNESS_MAIN it is a stand-alone program (for a run under a sanitizer).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_quant.h"

extern "C" {
int h_run() { return QUANT_RUN; }
int h_slots() { return (int)QUANT_SLOTS; }
uint32_t h_empty() { return QUANT_EMPTY; }
uint32_t h_canon(uint32_t px) { return quant_canon(px); }
void h_x(uint32_t px, uint32_t* x) { quant_x(px, x); }
uint64_t h_dist(uint32_t p, uint32_t q) {
    uint32_t x[4], y[4];
    quant_x(p, x);
    quant_x(q, y);
    return quant_dist(x, y);
}
int h_nearest(const uint32_t* pal, int n, uint32_t px) {
    std::vector<uint32_t> pal_x(4 * (size_t)n);
    uint32_t x[4];
    for (int i = 0; i < n; ++i) quant_x(quant_canon(pal[i]), pal_x.data() + 4 * i);
    quant_x(quant_canon(px), x);
    return quant_nearest(pal_x.data(), n, x);
}
uint32_t h_bin_key(uint32_t px) { return quant_bin_key(px); }
uint32_t h_slot(uint32_t px) { return quant_slot(quant_canon(px)); }
int h_depth(int n) { return quant_depth(n); }
int64_t h_row_bytes(int64_t cols, int depth) { return quant_row_bytes(cols, depth); }
void h_pack_run(const uint8_t* idx, int n, int depth, uint8_t* out) { quant_pack_run(idx, n, depth, out); }

// svgr_quant_index: the row stream and / or the plain indices (either may be null)
void h_index(const uint32_t* src, int64_t rows, int64_t cols, const uint32_t* pal, int n_pal, uint8_t* stream, uint8_t* indices) {
    quant_index_rows(src, rows, cols, pal, n_pal, stream, indices);
}

// svgr_quant_distinct: the distinct canonical pixels, ascending, if there are at most max_colors; -1 otherwise
int64_t h_distinct(const uint32_t* src, int64_t n, int max_colors, uint32_t* colors) {
    std::set<uint32_t> seen;
    for (int64_t i = 0; i < n; ++i) {
        seen.insert(quant_canon(src[i]));
        if ((int64_t)seen.size() > max_colors) return -1;
    }
    std::copy(seen.begin(), seen.end(), colors);
    return (int64_t)seen.size();
}

// svgr_quant_bins: the non-empty bins in key order (keys and bins have room for min(n, 2^20) entries); their number
int64_t h_bins(const uint32_t* src, int64_t n, uint32_t* keys, uint64_t* bins) {
    std::map<uint32_t, QuantBin> hist;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t c = quant_canon(src[i]);
        uint32_t x[4];
        quant_x(c, x);
        QuantBin& b = hist[quant_bin_key(c)];
        b.n += 1;
        for (int k = 0; k < 4; ++k) b.s[k] += x[k];
    }
    int64_t i = 0;
    for (const auto& kv : hist) {
        keys[i] = kv.first;
        bins[5 * i] = kv.second.n;
        for (int k = 0; k < 4; ++k) bins[5 * i + 1 + k] = kv.second.s[k];
        ++i;
    }
    return i;
}
}  // extern "C"

#ifdef QUANT_HARNESS_MAIN
int main() {
    const int64_t rows = 5, cols = 19;
    std::vector<uint32_t> src((size_t)(rows * cols));
    uint32_t v = 12345u;
    for (auto& p : src) {
        v = v * 1664525u + 1013904223u;
        p = v & 0xFF0F0F0Fu;
    }
    for (int n_pal : {1, 2, 3, 16, 17, 256}) {
        std::vector<uint32_t> pal((size_t)n_pal);
        for (int i = 0; i < n_pal; ++i) pal[(size_t)i] = src[(size_t)i % src.size()];
        std::vector<uint8_t> stream((size_t)(rows * quant_row_bytes(cols, quant_depth(n_pal)))), idx((size_t)(rows * cols));
        h_index(src.data(), rows, cols, pal.data(), n_pal, stream.data(), idx.data());
    }
    std::vector<uint32_t> keys(src.size()), colors(256);
    std::vector<uint64_t> bins(5 * src.size());
    const int64_t nb = h_bins(src.data(), (int64_t)src.size(), keys.data(), bins.data());
    const int64_t nd = h_distinct(src.data(), (int64_t)src.size(), 256, colors.data());
    std::printf("quant harness: %lld bins, %lld distinct\n", (long long)nb, (long long)nd);
    return 0;
}
#endif
