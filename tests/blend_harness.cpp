// Host build of the mix-blend-mode arithmetic in svgrasterize.py_amd/csrc/svgr_core.h (mix_blend_px, blend_sep, blend_nonsep),
// for CPU-side unit tests only (tests/test_blend_host.py, tests/test_gpu_blend.py).  NOT a CPU fallback of the product: the
// package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_core.h"

using namespace svgr;

extern "C" {

// n premultiplied pixels: out[4 k ..] = mix_blend_px(mode, backdrop[4 k ..], src[4 k ..])
void bh_px(int mode, long n, const double* backdrop, const double* src, double* out) {
    for (long k = 0; k < n; ++k) {
        double d[4] = {backdrop[4 * k], backdrop[4 * k + 1], backdrop[4 * k + 2], backdrop[4 * k + 3]};
        mix_blend_px(mode, d, src + 4 * k);
        for (int c = 0; c < 4; ++c) out[4 * k + c] = d[c];
    }
}

// B(Cb, Cs) on n straight colours (3 channels each), separable or not
void bh_b(int mode, long n, const double* cb, const double* cs, double* out) {
    for (long k = 0; k < n; ++k) {
        if (mode >= kBlendHue) {
            blend_nonsep(mode, cb + 3 * k, cs + 3 * k, out + 3 * k);
        } else {
            for (int c = 0; c < 3; ++c) out[3 * k + c] = blend_sep(mode, cb[3 * k + c], cs[3 * k + c]);
        }
    }
}

}  // extern "C"
