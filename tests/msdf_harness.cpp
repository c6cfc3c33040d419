// msdf_harness.cpp -- the multi-channel distance-field header (csrc/svgr_msdf.h) compiled for the host, for tests/test_msdf_host.py
// and tests/test_gpu_msdf.py (g++ -ffp-contract=off): what a lane of k_msdf_distance does, one point after the other, without its
// cull.
#include <cstdint>

#include "../svgrasterize.py_amd/csrc/svgr_msdf.h"

extern "C" {

int mh_edge_doubles() { return MSDF_EDGE_DOUBLES; }
int mh_sdf_edge_doubles() { return SDF_EDGE_DOUBLES; }

// one prepared edge: out[0 .. 8) = a0, b0, x, y, inv, a1, b1, rl
void mh_prepare(const double* e4, double* out) { msdf_edge_prepare(e4[0], e4[1], e4[2], e4[3], out); }

// R, G, B, A of n_points points over the groups: out[4 * i + c]
void mh_msdf(const double* edges, const int32_t* off, const uint8_t* rule, const uint8_t* colour, const int32_t* group_off, const int8_t* orient,
             long long n_groups, const double* points, long long n_points, double spread, double* out) {
    for (long long i = 0; i < n_points; ++i)
        msdf_point(edges, off, rule, colour, group_off, orient, n_groups, spread, points[2 * i], points[2 * i + 1], out + 4 * i);
}

double mh_median(double r, double g, double b) { return msdf_median(r, g, b); }

void mh_encode(const double* d, long long n, double spread, float* f32, uint8_t* u8) {
    for (long long i = 0; i < n; ++i) {
        f32[i] = sdf_encode_f32(d[i], spread);
        u8[i] = sdf_encode_u8(d[i], spread);
    }
}

}  // extern "C"
