// glyf_harness.cpp -- the TrueType outline per-lane header (csrc/svgr_glyf.h) compiled for the host, for
// tests/test_truetype_host.py (g++ -ffp-contract=off): the library's validation walk with its tables, then the lanes of
// k_glyf_emit one after the other.  With GLYF_HARNESS_MAIN it is a program of its own (a sanitizer build runs that).
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_glyf.h"

extern "C" {

// The validation of svgr_glyf_outline: its status, and the counts of lanes, segments and subpaths.
int gh_validate(const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off, int64_t n_contours, const int32_t* glyph_contour_off,
                int64_t n_glyphs, const int32_t* part_glyph, const double* part_m, const double* part_pen, const double* part_sx,
                const double* part_sy, int64_t n_parts, int64_t* counts3) {
    GlyfTables t;
    const int rc = glyf_tables(pt_on, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen, part_sx,
                               part_sy, n_parts, t);
    counts3[0] = counts3[1] = counts3[2] = 0;
    if (rc) return rc;
    counts3[0] = t.part_lane_off[(size_t)n_parts];
    counts3[1] = t.part_seg_off[(size_t)n_parts];
    counts3[2] = (int64_t)t.sizes.size();
    return 0;
}

// svgr_glyf_outline into arrays of gh_validate's counts: types, params (8 per segment), sizes.  SVGR_E_STATE when a lane met a
// slot outside the result.
int gh_outline(const int16_t* pt_xy, const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
               const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m, const double* part_pen,
               const double* part_sx, const double* part_sy, int64_t n_parts, int32_t* types, double* params, int32_t* sizes) {
    GlyfTables t;
    if (int rc = glyf_tables(pt_on, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen, part_sx,
                             part_sy, n_parts, t))
        return rc;
    const int n_lanes = t.part_lane_off[(size_t)n_parts], n_out = t.part_seg_off[(size_t)n_parts];
    const GlyfView v{pt_xy, pt_on, t.pt_slot.data(), contour_off, glyph_contour_off, part_glyph, t.part_lane_off.data(), t.part_seg_off.data(),
                     part_m, part_pen, part_sx, part_sy, (int)n_contours, (int)n_parts, (int)n_points, n_out};
    bool ok = true;
    if (n_out > 0)
        for (int j = 0; j < n_lanes; ++j) ok = glyf_emit(v, j, types, params) && ok;
    for (size_t s = 0; s < t.sizes.size(); ++s) sizes[s] = t.sizes[s];
    return ok ? 0 : SVGR_E_STATE;
}

}  // extern "C"

#if defined(GLYF_HARNESS_MAIN)
#include <cstdio>
int main() {
    // glyph 0: a square of on-curve points and a circle-like contour of alternating points; glyph 1: empty; glyph 2: one point
    const int16_t xy[] = {0, 0, 100, 0, 100, 100, 0, 100, 50, 20, 80, 20, 80, 50, 80, 80, 50, 80, 20, 80, 20, 50, 20, 20, 7, 7};
    const uint8_t on[] = {1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 0};
    const int32_t c_off[] = {0, 4, 12, 13}, g_off[] = {0, 2, 2, 3}, glyph[] = {1, 0, 2, 0};
    const double m[] = {1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0.5, 0.25, -0.25, 0.5, 10, -10};
    const double pen[] = {0, 10, 200, 300}, sx[] = {0.01, 0.01, 0.01, 0.01}, sy[] = {-0.01, -0.01, -0.01, 0.01};
    int64_t counts[3];
    int rc = gh_validate(on, 13, c_off, 3, g_off, 3, glyph, m, pen, sx, sy, 4, counts);
    if (rc) return 1;
    std::vector<int32_t> types((size_t)counts[1]), sizes((size_t)counts[2]);
    std::vector<double> params((size_t)counts[1] * 8);
    rc = gh_outline(xy, on, 13, c_off, 3, g_off, 3, glyph, m, pen, sx, sy, 4, types.data(), params.data(), sizes.data());
    std::printf("%d %lld %lld %lld %.17g\n", rc, (long long)counts[0], (long long)counts[1], (long long)counts[2], params[params.size() - 8]);
    return rc;
}
#endif
