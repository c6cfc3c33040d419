// Host build of the path bbox rule in svgrasterize.py_amd/csrc/svgr_core.h (path_box, path_box_is): what k_path_bbox places a path
// by and what a replay that keeps the plan's slab table checks the plan's records against (k_path_build<1>).  For CPU-side unit
// tests only (tests/test_path_box_host.py).  NOT a CPU fallback of the product: the package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_core.h"

using namespace svgr;

extern "C" {

// n paths: ext[4 i ..] = {min row, min column, max row, max column} as k_flatten folds them into keys (made here the same way);
// has_edge[i] == 0: a path without an edge (all four keys 0).  vp = {r0, c0, rows, cols}, used when has_vp.
// out[8 i ..] = {r0, c0, rows, cols, b0, nb, nct, refused}
void pbx_path_box(long n, const double* ext, const unsigned char* has_edge, int has_vp, const int* vp, int tr, int tc, int* out) {
    for (long i = 0; i < n; ++i) {
        uint64_t k[4] = {0, 0, 0, 0};
        if (has_edge[i]) {
            k[0] = ~f64_key(ext[4 * i]); k[1] = ~f64_key(ext[4 * i + 1]);
            k[2] = f64_key(ext[4 * i + 2]); k[3] = f64_key(ext[4 * i + 3]);
        }
        const PathBox o = path_box(k[0], k[1], k[2], k[3], has_vp, vp[0], vp[1], vp[2], vp[3], tr, tc);
        int* q = out + 8 * i;
        q[0] = o.r0; q[1] = o.c0; q[2] = o.rows; q[3] = o.cols; q[4] = o.b0; q[5] = o.nb; q[6] = o.nct; q[7] = o.refused;
    }
}

// the guard's comparison: does the record {r0, c0, rows, cols, nb} state what the rule gives for the extent?
int pbx_guard_ok(const double* ext, int has_vp, const int* vp, int tr, int tc, const int* rec) {
    const PathBox o = path_box(~f64_key(ext[0]), ~f64_key(ext[1]), f64_key(ext[2]), f64_key(ext[3]), has_vp, vp[0], vp[1], vp[2], vp[3], tr, tc);
    return path_box_is(o, rec[0], rec[1], rec[2], rec[3], rec[4]) ? 1 : 0;
}

}  // extern "C"
