// gradpaint_harness.cpp -- the gradient-paint header (csrc/svgr_gradpaint.h) compiled for the host, for
// tests/test_gradpaint_host.py (g++ -ffp-contract=off): what the lanes of k_compose_over_painted and k_compose_vjp_painted do,
// one pixel after the other.  Planes, images and gradients are doubles: a float plane widens exactly, and the device rounds once
// at its stores.  desc is n_paths x 4 ints {kind, spread, first stop, end stop}; view is {row0, col0, cols}.
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../svgrasterize.py_amd/csrc/svgr_gradpaint.h"

using namespace svgr;

extern "C" {

// svgr_compose_painted_forward: cover n_paths x n_px, paints n_paths x 4, m6 n_paths x 6, geom n_paths x 4, image n_px x 4
void gph_forward(const double* cover, const double* paints, const int* desc, const double* m6, const double* geom, const double* pos,
                 const double* rgba, const double* bg, const long long* view, int n_paths, long long n_px, double* image) {
    for (long long i = 0; i < n_px; ++i) {
        const long long row = i / view[2], colj = i % view[2];
        double C[4] = {bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0};
        for (int p = 0; p < n_paths; ++p) {
            const int* d = desc + 4 * (size_t)p;
            const double m = cover[(size_t)p * n_px + i];
            if (d[0] == 0) {
                compose_step(C, m, paints + 4 * (size_t)p);
            } else {
                double col[4];
                GradPaintPx e;
                gradpaint_colour(d[0], d[1], m6 + 6 * (size_t)p, geom + 4 * (size_t)p, d[3] - d[2], pos + d[2], rgba + 4 * (size_t)d[2], row, colj, view[0],
                                 view[1], col, e);
                gradpaint_step(C, m, col, paints + 4 * (size_t)p);
            }
        }
        for (int k = 0; k < 4; ++k) image[4 * (size_t)i + k] = C[k];
    }
}

// svgr_compose_painted_backward: grad_cover n_paths x n_px (it holds T_p between the two walks, as on the device); every summed
// output gets its terms in pixel order.  used, if given, is n_px x n_paths x 2: the stops each pixel used (of the path's own list).
void gph_backward(const double* cover, const double* paints, const int* desc, const double* m6, const double* geom, const double* pos,
                  const double* rgba, const double* bg, const long long* view, const double* grad_image, int n_paths, int n_stops, long long n_px,
                  double* grad_cover, double* grad_paints, double* grad_m6, double* grad_geom, double* grad_pos, double* grad_rgba, int* used) {
    for (int j = 0; j < 4 * n_paths; ++j) grad_paints[j] = grad_geom[j] = 0.0;
    for (int j = 0; j < 6 * n_paths; ++j) grad_m6[j] = 0.0;
    for (int j = 0; j < n_stops; ++j) grad_pos[j] = 0.0;
    for (int j = 0; j < 4 * n_stops; ++j) grad_rgba[j] = 0.0;
    for (long long i = 0; i < n_px; ++i) {
        const long long row = i / view[2], colj = i % view[2];
        double above = 1.0;
        for (int p = n_paths - 1; p >= 0; --p) {
            const int* d = desc + 4 * (size_t)p;
            const size_t at = (size_t)p * n_px + i;
            double u;
            if (d[0] == 0) {
                u = compose_through(cover[at], paints[4 * (size_t)p + 3]);
            } else {
                double col[4];
                GradPaintPx e;
                gradpaint_colour(d[0], d[1], m6 + 6 * (size_t)p, geom + 4 * (size_t)p, d[3] - d[2], pos + d[2], rgba + 4 * (size_t)d[2], row, colj, view[0],
                                 view[1], col, e);
                u = gradpaint_through(cover[at], col, paints + 4 * (size_t)p);
            }
            grad_cover[at] = above;
            above = above * u;
        }
        double C[4] = {bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0};
        for (int p = 0; p < n_paths; ++p) {
            const int* d = desc + 4 * (size_t)p;
            const size_t at = (size_t)p * n_px + i;
            const double* paint = paints + 4 * (size_t)p;
            double* gp = grad_paints + 4 * (size_t)p;
            if (d[0] == 0) {
                double t[4];
                grad_cover[at] = compose_vjp_step(C, grad_cover[at], grad_image + 4 * (size_t)i, cover[at], paint, t);
                compose_step(C, cover[at], paint);
                for (int k = 0; k < 4; ++k) gp[k] = gp[k] + t[k];
                if (used) used[2 * ((size_t)i * n_paths + p)] = used[2 * ((size_t)i * n_paths + p) + 1] = -1;
                continue;
            }
            double col[4], P[4], t[4], dense[GRADPAINT_DENSE], lo[GRADPAINT_STOP], hi[GRADPAINT_STOP];
            GradPaintPx e;
            gradpaint_colour(d[0], d[1], m6 + 6 * (size_t)p, geom + 4 * (size_t)p, d[3] - d[2], pos + d[2], rgba + 4 * (size_t)d[2], row, colj, view[0], view[1],
                             col, e);
            gradpaint_effective(col, paint, P);
            grad_cover[at] = compose_vjp_step(C, grad_cover[at], grad_image + 4 * (size_t)i, cover[at], P, t);
            gradpaint_vjp(d[0], geom + 4 * (size_t)p, pos + d[2], rgba + 4 * (size_t)d[2], col, paint, e, t, dense, lo, hi);
            gradpaint_step(C, cover[at], col, paint);
            for (int k = 0; k < 4; ++k) gp[k] = gp[k] + dense[k];
            for (int k = 0; k < 6; ++k) grad_m6[6 * (size_t)p + k] = grad_m6[6 * (size_t)p + k] + dense[4 + k];
            for (int k = 0; k < 4; ++k) grad_geom[4 * (size_t)p + k] = grad_geom[4 * (size_t)p + k] + dense[10 + k];
            if (used) {
                used[2 * ((size_t)i * n_paths + p)] = e.lo;
                used[2 * ((size_t)i * n_paths + p) + 1] = e.hi;
            }
            if (e.lo < 0) continue;
            grad_pos[d[2] + e.lo] = grad_pos[d[2] + e.lo] + lo[0];
            for (int k = 0; k < 4; ++k) grad_rgba[4 * (size_t)(d[2] + e.lo) + k] = grad_rgba[4 * (size_t)(d[2] + e.lo) + k] + lo[1 + k];
            if (e.hi == e.lo) continue;
            grad_pos[d[2] + e.hi] = grad_pos[d[2] + e.hi] + hi[0];
            for (int k = 0; k < 4; ++k) grad_rgba[4 * (size_t)(d[2] + e.hi) + k] = grad_rgba[4 * (size_t)(d[2] + e.hi) + k] + hi[1 + k];
        }
    }
}

}  // extern "C"
