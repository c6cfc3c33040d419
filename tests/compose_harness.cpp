// compose_harness.cpp -- the differentiable-compositing header (csrc/svgr_compose.h) compiled for the host, for
// tests/test_compose_host.py (g++ -ffp-contract=off): what the lanes of k_compose_over and k_compose_vjp do, one pixel after the
// other.  Planes, images and gradients are doubles: a float plane widens exactly, and the device rounds once at its stores.
#include <cstddef>
#include <cstdint>

#include "../svgrasterize.py_amd/csrc/svgr_compose.h"

using namespace svgr;

extern "C" {

// svgr_compose_forward: cover n_paths x n_px, paints n_paths x 4, bg 4 doubles or NULL, image n_px x 4
void cmh_forward(const double* cover, const double* paints, const double* bg, int n_paths, long long n_px, double* image) {
    for (long long i = 0; i < n_px; ++i) {
        double C[4] = {bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0};
        for (int p = 0; p < n_paths; ++p) compose_step(C, cover[(size_t)p * n_px + i], paints + 4 * (size_t)p);
        for (int k = 0; k < 4; ++k) image[4 * (size_t)i + k] = C[k];
    }
}

// svgr_compose_backward: grad_cover n_paths x n_px (it holds T_p between the two walks, as on the device), grad_paints
// n_paths x 4: every path's terms added in pixel order
void cmh_backward(const double* cover, const double* paints, const double* bg, const double* grad_image, int n_paths, long long n_px,
                  double* grad_cover, double* grad_paints) {
    for (int j = 0; j < 4 * n_paths; ++j) grad_paints[j] = 0.0;
    for (long long i = 0; i < n_px; ++i) {
        double above = 1.0;
        for (int p = n_paths - 1; p >= 0; --p) {
            const size_t at = (size_t)p * n_px + i;
            grad_cover[at] = above;
            above = above * compose_through(cover[at], paints[4 * (size_t)p + 3]);
        }
        double C[4] = {bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0};
        for (int p = 0; p < n_paths; ++p) {
            const size_t at = (size_t)p * n_px + i;
            const double* paint = paints + 4 * (size_t)p;
            double t[4];
            grad_cover[at] = compose_vjp_step(C, grad_cover[at], grad_image + 4 * (size_t)i, cover[at], paint, t);
            compose_step(C, cover[at], paint);
            for (int k = 0; k < 4; ++k) grad_paints[4 * (size_t)p + k] = grad_paints[4 * (size_t)p + k] + t[k];
        }
    }
}

}  // extern "C"
