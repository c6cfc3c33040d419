// Host build of the <image> index rule in svgrasterize.py_amd/csrc/svgr_core.h (image_corner, image_nearest) over arrays of
// coordinates and level sizes, for CPU-side unit tests only (tests/test_image_cases_host.py).  NOT a CPU fallback of the
// product: the package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_core.h"

using namespace svgr;

extern "C" {

// idx[4 i ..] = {c0, c1, r0, r1}, frac[2 i ..] = {fx, fy} of the level-space point (x[i], y[i]) in a (h[i], w[i]) level
void ih_corner(const double* x, const double* y, const int* w, const int* h, long n, int* idx, double* frac) {
    for (long i = 0; i < n; ++i) {
        const ImageCorner k = image_corner(x[i], y[i], w[i], h[i]);
        idx[4 * i] = k.c0; idx[4 * i + 1] = k.c1; idx[4 * i + 2] = k.r0; idx[4 * i + 3] = k.r1;
        frac[2 * i] = k.fx; frac[2 * i + 1] = k.fy;
    }
}

// idx[2 i ..] = {(int)xf, (int)yf}, the casts k_image_fill makes of image_nearest's clamped doubles
void ih_nearest(const double* u, const double* v, const int* w, const int* h, long n, int* idx) {
    for (long i = 0; i < n; ++i) {
        double xf, yf;
        image_nearest(u[i], v[i], w[i], h[i], xf, yf);
        idx[2 * i] = (int)xf; idx[2 * i + 1] = (int)yf;
    }
}

}  // extern "C"
