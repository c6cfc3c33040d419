// cover_harness.cpp -- the differentiable-coverage header (csrc/svgr_cover.h) compiled for the host, for tests/test_cover_host.py
// (g++ -ffp-contract=off): what the lanes of k_cover_accumulate, k_cover_resolve, k_cover_vjp and k_cover_vjp_m6 do, one segment
// (one row, one path) after the other.
#include <cstdint>
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_cover.h"

using namespace svgr;

namespace {
// the path whose range holds `seg`, as the kernels find it
int path_of(const int32_t* off, int n_paths, int seg) {
    int lo = 0, hi = n_paths;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= seg) lo = mid; else hi = mid;
    }
    return off[lo] <= seg && seg < off[lo + 1] ? lo : -1;
}
}  // namespace

extern "C" {

int ch_slope(double A, int rule) { return cover_slope(A, rule); }
double ch_fill(double A, int rule) { return fill_rule(A, rule); }

// the edges of the segments in the viewport's coordinates, 6 doubles each: p0r, p0c, p1r, p1c, t0, t1; edge_seg: their segment.
// Returns their number (whatever `cap`; only the first `cap` are stored).
long long ch_edges(const double* segs, const uint8_t* kind, const int32_t* off, const double* m6, int n_segs, int n_paths, const int64_t* vp,
                   double flatness, double* edges, int32_t* edge_seg, long long cap) {
    const double thr = (flatness * flatness) * 16.0;
    long long n = 0;
    for (int s = 0; s < n_segs; ++s) {
        const int p = path_of(off, n_paths, s);
        if (p < 0) continue;
        double c[8];
        const int cubic = kind[s] != 0;
        if (!cover_seg_points(segs + 8 * (size_t)s, cubic ? 4 : 2, m6 + 6 * (size_t)p, c)) continue;
        bool overflow = false;
        cover_seg_edges(c, cubic, thr, (double)vp[0], (double)vp[1], [&](double a, double b, double cc, double d, double t0, double t1) {
            if (n < cap) {
                double* e = edges + 6 * n;
                e[0] = a; e[1] = b; e[2] = cc; e[3] = d; e[4] = t0; e[5] = t1;
                edge_seg[n] = s;
            }
            ++n;
        }, overflow);
    }
    return n;
}

// svgr_cover_forward: acc (n_paths x rows x cols, may be NULL) receives the accumulation plane before the row sums.  Returns the
// status bits.
int ch_forward(const double* segs, const uint8_t* kind, const int32_t* off, const double* m6, const uint8_t* rule, int n_segs, int n_paths,
               const int64_t* vp, double flatness, double* cover, int8_t* slope, double* acc_out) {
    const int rows = (int)vp[2], cols = (int)vp[3];
    const double thr = (flatness * flatness) * 16.0;
    const size_t plane = (size_t)rows * (size_t)cols;
    std::vector<double> acc((size_t)n_paths * plane, 0.0);
    int status = 0;
    for (int s = 0; s < n_segs; ++s) {
        const int p = path_of(off, n_paths, s);
        if (p < 0) continue;
        double* a = acc.data() + (size_t)p * plane;
        status |= cover_seg_accumulate(segs + 8 * (size_t)s, kind[s] != 0, m6 + 6 * (size_t)p, (double)vp[0], (double)vp[1], rows, cols, thr,
                                       [&](int r, int c, double v) { a[(size_t)r * cols + c] += v; });
    }
    for (size_t i = 0; acc_out && i < acc.size(); ++i) acc_out[i] = acc[i];
    for (int p = 0; p < n_paths; ++p)
        for (int r = 0; r < rows; ++r) {
            double A = 0.0;
            for (int c = 0; c < cols; ++c) {
                const size_t i = (size_t)p * plane + (size_t)r * cols + c;
                A = A + acc[i];
                cover[i] = fill_rule(A, rule[p] & 1);
                slope[i] = (int8_t)cover_slope(A, rule[p] & 1);
            }
        }
    return status;
}

// svgr_cover_backward from a slope plane and grad_out (doubles: a float plane widens exactly).  Returns the status bits.
int ch_backward(const double* segs, const uint8_t* kind, const int32_t* off, const double* m6, int n_segs, int n_paths, const int64_t* vp,
                double flatness, const int8_t* slope, const double* grad_out, double* grad_segs, double* grad_m6) {
    const int rows = (int)vp[2], cols = (int)vp[3];
    const double thr = (flatness * flatness) * 16.0;
    const size_t plane = (size_t)rows * (size_t)cols;
    std::vector<double> part((size_t)n_segs * 6, 0.0);
    int status = 0;
    for (int s = 0; s < n_segs; ++s) {
        const int p = path_of(off, n_paths, s);
        double* gs = grad_segs + 8 * (size_t)s;
        for (int i = 0; i < 8; ++i) gs[i] = 0.0;
        if (p < 0) continue;
        const size_t base = (size_t)p * plane;
        status |= cover_seg_vjp(segs + 8 * (size_t)s, kind[s] != 0, m6 + 6 * (size_t)p, (double)vp[0], (double)vp[1], rows, cols, thr,
                                [&](int r, int c) {
                                    const size_t i = base + (size_t)r * cols + c;
                                    return cover_weight(grad_out[i], slope[i]);
                                }, gs, part.data() + 6 * (size_t)s);
    }
    for (int p = 0; p < n_paths; ++p) {
        double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int s = off[p]; s < off[p + 1]; ++s)
            for (int k = 0; k < 6; ++k) m[k] = m[k] + part[6 * (size_t)s + k];
        for (int k = 0; k < 6; ++k) grad_m6[6 * (size_t)p + k] = m[k];
    }
    return status;
}

}  // extern "C"
