// hit_harness.cpp -- the hit-testing header (csrc/svgr_hit.h) compiled for the host, for tests/test_hit_host.py
// (g++ -ffp-contract=off): what a lane of k_hit_winding and of k_hit_resolve does, one point after the other.
#include <cstdint>

#include "../svgrasterize.py_amd/csrc/svgr_hit.h"

extern "C" {

int hh_block() { return HIT_BLOCK; }
int hh_chunk() { return HIT_CHUNK; }

int hh_edge_term(const double* e4, double pa, double pb) { return hit_finite(pa, pb) ? hit_edge_term(e4[0], e4[1], e4[2], e4[3], pa, pb) : 0; }

// winding numbers of n_points points against n_paths paths (path p: the edges off[p] .. off[p + 1]): out[i * n_paths + p]
void hh_winding(const double* edges, const int32_t* off, long long n_paths, const double* points, long long n_points, int32_t* out) {
    for (long long i = 0; i < n_points; ++i)
        for (long long p = 0; p < n_paths; ++p)
            out[i * n_paths + p] = hit_winding(edges + 4 * (long long)off[p], off[p + 1] - off[p], points[2 * i], points[2 * i + 1]);
}

// inside bits from winding numbers: bits[i * words + p / 32]
void hh_inside_bits(const int32_t* winding, const uint8_t* rule, long long n_paths, long long n_points, uint32_t* bits) {
    const long long words = (n_paths + 31) / 32;
    for (long long i = 0; i < n_points; ++i)
        for (long long p = 0; p < n_paths; ++p)
            if (hit_inside(winding[i * n_paths + p], rule[p] & 1)) bits[i * words + p / 32] |= 1u << (p & 31);
}

long long hh_check_tables(long long n_paths, const int32_t* clip_off, const int32_t* clip_group, const int32_t* group_off, const int32_t* group_src,
                          long long n_groups) {
    return hit_check_tables(n_paths, clip_off, clip_group, group_off, group_src, n_groups);
}

// the resolve of every point's row, in place; top[i]
void hh_resolve(uint32_t* bits, long long n_points, int n_paths, const uint8_t* pickable, const int32_t* clip_off, const int32_t* clip_group,
                const int32_t* group_off, const int32_t* group_src, int32_t* top) {
    const long long words = (n_paths + 31) / 32;
    for (long long i = 0; i < n_points; ++i) top[i] = hit_resolve(bits + i * words, n_paths, pickable, clip_off, clip_group, group_off, group_src);
}

}  // extern "C"
