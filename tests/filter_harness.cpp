// Host build of the filter-primitive arithmetic in svgrasterize.py_amd/csrc/svgr_core.h (turb_init, turb_params, turb_point),
// and a restatement of the displacement map's source-index guard, for CPU-side unit tests only
// (tests/test_filter_primitives_host.py, tests/test_gpu_filter_primitives.py, tests/test_image_cases_host.py).  NOT a CPU
// fallback of the product: the package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_core.h"

using namespace svgr;

extern "C" {

void fh_lattice(int64_t seed, int* sel, double* grad) { turb_init(seed, sel, grad); }

// out[4 i ..] = the four channels at user point (pts[2 i], pts[2 i + 1])
void fh_turbulence(int64_t seed, double fx, double fy, const double* tile, int octaves, int fractal, int stitch, const double* pts,
                   long n, double* out) {
    int sel[kTurbLattice];
    double grad[kTurbLattice * 8];
    turb_init(seed, sel, grad);
    const TurbParams p = turb_params(fx, fy, tile, octaves, fractal, stitch);
    for (long i = 0; i < n; ++i) turb_point(sel, grad, p, pts[2 * i], pts[2 * i + 1], out + 4 * i);
}

// the layer k_layer_turbulence writes: pixel [R, C] at device point (o0 + R + 0.5, o1 + C + 0.5), user point by inv (plain form)
void fh_turbulence_layer(int64_t seed, double fx, double fy, const double* tile, int octaves, int fractal, int stitch,
                         const double* inv, long o0, long o1, long rows, long cols, double* out) {
    int sel[kTurbLattice];
    double grad[kTurbLattice * 8];
    turb_init(seed, sel, grad);
    const TurbParams p = turb_params(fx, fy, tile, octaves, fractal, stitch);
    for (long R = 0; R < rows; ++R) {
        for (long C = 0; C < cols; ++C) {
            const double d0 = (double)(o0 + R) + 0.5, d1 = (double)(o1 + C) + 0.5;
            const double px = inv[0] * d0 + inv[1] * d1 + inv[2];
            const double py = inv[3] * d0 + inv[4] * d1 + inv[5];
            turb_point(sel, grad, p, px, py, out + 4 * (R * cols + C));
        }
    }
}

// k_layer_displacement_map's guard, restated: the displaced point (p0[i], p1[i]) against a source box (s0, s1, srows, scols),
// compared as doubles and cast only behind the comparison.  out[i] = the flat pixel index the kernel would read, -1 where it
// writes a transparent pixel.
void fh_dm_index(const double* p0, const double* p1, long n, int s0, int s1, int srows, int scols, int64_t* out) {
    for (long i = 0; i < n; ++i) {
        const double r = floor(p0[i]) - s0, c = floor(p1[i]) - s1;
        out[i] = -1;
        if (r >= 0.0 && r < (double)srows && c >= 0.0 && c < (double)scols) out[i] = (int64_t)((size_t)r * scols + (size_t)c);
    }
}

}  // extern "C"
