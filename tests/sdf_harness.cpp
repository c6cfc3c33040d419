// sdf_harness.cpp -- the distance-field header (csrc/svgr_sdf.h) compiled for the host, for tests/test_sdf_host.py
// (g++ -ffp-contract=off): what a lane of k_sdf_distance does, one point after the other, without its cull,
// and the cull's predicate by itself.
#include <cstdint>

#include "../svgrasterize.py_amd/csrc/svgr_sdf.h"

extern "C" {

int sh_edge_doubles() { return SDF_EDGE_DOUBLES; }
int sh_elem_bytes(int enc) { return sdf_elem_bytes(enc); }

// one prepared edge: out[0 .. 6) = a0, b0, x, y, inv, b1
void sh_prepare(const double* e4, double* out) { sdf_edge_prepare(e4[0], e4[1], e4[2], e4[3], out); }

// the winding term from the shared differences, and svgr_hit.h's own: they must be the same number
int sh_terms(const double* e4, double pa, double pb, int* hit_term) {
    double q[SDF_EDGE_DOUBLES];
    sdf_edge_prepare(e4[0], e4[1], e4[2], e4[3], q);
    *hit_term = hit_edge_term(e4[0], e4[1], e4[2], e4[3], pa, pb);
    return sdf_edge_term(q[1], q[5], q[2], q[3], pb, pa - q[0], pb - q[1]);
}

// clamped distances of n_points points to n_paths paths (path p: the edges off[p] .. off[p + 1]): out[i * n_paths + p]
void sh_distance(const double* edges, const int32_t* off, const uint8_t* rule, long long n_paths, const double* points, long long n_points,
                 double spread, int is_signed, double* out) {
    for (long long i = 0; i < n_points; ++i)
        for (long long p = 0; p < n_paths; ++p)
            out[i * n_paths + p] = sdf_path_distance(edges + 4 * (long long)off[p], off[p + 1] - off[p], rule[p] & 1, is_signed, spread,
                                                     points[2 * i], points[2 * i + 1]);
}

// the kernels' cull, case by case: ext[4 * i ..] = min a, min b, max a, max b; box[5 * i ..] = lo_a, hi_a, lo_b, hi_b, min |pb|
void sh_out_of_reach(const double* ext, const double* box, const double* cull_spread, long long n, uint8_t* out) {
    for (long long i = 0; i < n; ++i) {
        const double* k = box + 5 * i;
        out[i] = sdf_out_of_reach(ext + 4 * i, HitBox{k[0], k[1], k[2], k[3], k[4]}, cull_spread[i]) ? 1 : 0;
    }
}

// the union of rows of clamped distances, as the kernel folds it: from +spread, fmin path after path
void sh_union(const double* d, long long n_points, long long n_paths, double spread, double* out) {
    for (long long i = 0; i < n_points; ++i) {
        double best = spread;
        for (long long p = 0; p < n_paths; ++p) best = fmin(best, d[i * n_paths + p]);
        out[i] = best;
    }
}

double sh_clamp(double d, double spread) { return sdf_clamp(d, spread); }
void sh_encode(const double* d, long long n, double spread, float* f32, uint8_t* u8) {
    for (long long i = 0; i < n; ++i) {
        f32[i] = sdf_encode_f32(d[i], spread);
        u8[i] = sdf_encode_u8(d[i], spread);
    }
}

}  // extern "C"
