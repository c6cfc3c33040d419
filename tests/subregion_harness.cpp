// Host build of feTile's index arithmetic in svgrasterize.py_amd/csrc/svgr_core.h (tile_wrap, tile_next, tile_source), for
// CPU-side unit tests only (tests/test_subregion_host.py).  NOT a CPU fallback of the product: the package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_core.h"

using namespace svgr;

extern "C" {

// One axis, the way k_layer_tile walks it: out[k] = the source index of output coordinate o0 + k (k = 0 .. n - 1) for the tile
// [t0, t0 + tn) of a source layer [s0, s0 + sn), -1 where the tile lies outside the layer.  `walk` != 0: one modulo at the
// start and tile_next from then on (the kernel's rows); 0: a modulo per coordinate (the kernel's columns).
void sh_axis(int o0, long n, int t0, int tn, int s0, int sn, int walk, int* out) {
    int t = tile_wrap(o0 - t0, tn);
    for (long k = 0; k < n; ++k) {
        if (!walk) t = tile_wrap(o0 - t0 + (int)k, tn);
        out[k] = tile_source(t, t0, s0, sn);
        if (walk) t = tile_next(t, tn);
    }
}

}  // extern "C"
