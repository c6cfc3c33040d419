// gvar_harness.cpp -- the variable-font per-lane header (csrc/svgr_gvar.h) compiled for the host, for
// tests/test_truetype_var_host.py (g++ -ffp-contract=off): the library's validation walk, then the lanes of k_gvar_delta one
// after the other, and the lanes of k_glyf_emit over the varied points.  With GVAR_HARNESS_MAIN it is a program of its own (a
// sanitizer build runs that).
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_glyf.h"
#include "../svgrasterize.py_amd/csrc/svgr_gvar.h"

extern "C" {

// svgr_gvar_deltas: the validation, then every lane.  A refusal leaves `pt_dxy` untouched.  SVGR_E_STATE when a lane met a
// point outside its tables.
int gv_deltas(const int16_t* pt_xy, int64_t n_points, const int32_t* contour_off, int64_t n_contours, const int32_t* glyph_contour_off,
              int64_t n_glyphs, const int32_t* glyph_tuple_off, const double* tuple_scalar, int64_t n_tuples, const int32_t* tuple_pt_off,
              const int32_t* tp_index, const int16_t* tp_dxy, int64_t n_entries, double* pt_dxy) {
    const char* why = "";
    if (int rc = gvar_tables(n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, glyph_tuple_off, tuple_scalar, n_tuples,
                             tuple_pt_off, tp_index, tp_dxy, n_entries, why))
        return rc;
    const GvarView v{pt_xy, contour_off, glyph_contour_off, glyph_tuple_off, tuple_scalar, tuple_pt_off, tp_index, tp_dxy,
                     (int)n_contours, (int)n_glyphs, (int)n_points, (int)n_tuples};
    bool ok = true;
    for (int a = 0; a < (int)n_points; ++a) ok = gvar_delta(v, a, pt_dxy[2 * (size_t)a], pt_dxy[2 * (size_t)a + 1]) && ok;
    return ok ? 0 : SVGR_E_STATE;
}

// svgr_glyf_outline_var into arrays of the glyf harness' counts (gh_validate): types, params (8 per segment), sizes.  A
// refusal of either walk leaves them untouched.
int gv_outline_var(const int16_t* pt_xy, const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
                   const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m, const double* part_pen,
                   const double* part_sx, const double* part_sy, int64_t n_parts, const int32_t* glyph_tuple_off, const double* tuple_scalar,
                   int64_t n_tuples, const int32_t* tuple_pt_off, const int32_t* tp_index, const int16_t* tp_dxy, int64_t n_entries,
                   int32_t* types, double* params, int32_t* sizes) {
    GlyfTables t;
    if (int rc = glyf_tables(pt_on, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen, part_sx,
                             part_sy, n_parts, t))
        return rc;
    std::vector<double> dxy((size_t)n_points * 2 + 2, 0.0);
    if (int rc = gv_deltas(pt_xy, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, glyph_tuple_off, tuple_scalar, n_tuples,
                           tuple_pt_off, tp_index, tp_dxy, n_entries, dxy.data()))
        return rc;
    const int n_lanes = t.part_lane_off[(size_t)n_parts], n_out = t.part_seg_off[(size_t)n_parts];
    GlyfView v{pt_xy, pt_on, t.pt_slot.data(), contour_off, glyph_contour_off, part_glyph, t.part_lane_off.data(), t.part_seg_off.data(),
               part_m, part_pen, part_sx, part_sy, (int)n_contours, (int)n_parts, (int)n_points, n_out};
    v.pt_dxy = n_tuples > 0 ? dxy.data() : nullptr;
    bool ok = true;
    if (n_out > 0)
        for (int j = 0; j < n_lanes; ++j) ok = glyf_emit(v, j, types, params) && ok;
    for (size_t s = 0; s < t.sizes.size(); ++s) sizes[s] = t.sizes[s];
    return ok ? 0 : SVGR_E_STATE;
}

}  // extern "C"

#if defined(GVAR_HARNESS_MAIN)
#include <cstdio>
int main() {
    // glyph 0: a square and a triangle; glyph 1: empty; glyph 2: one point.  Two tuples on glyph 0, one on glyph 2.
    const int16_t xy[] = {0, 0, 100, 0, 100, 100, 0, 100, 50, 20, 80, 20, 65, 60, 7, 7};
    const uint8_t on[] = {1, 1, 1, 1, 1, 0, 1, 1};
    const int32_t c_off[] = {0, 4, 7, 8}, g_off[] = {0, 2, 2, 3}, glyph[] = {0, 2, 0};
    const double m[] = {1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0.5, 0.25, -0.25, 0.5, 10, -10};
    const double pen[] = {0, 200, 300}, sx[] = {0.01, 0.01, 0.01}, sy[] = {-0.01, -0.01, 0.01};
    const int32_t t_off[] = {0, 2, 2, 3}, p_off[] = {0, 2, 3, 4}, index[] = {1, 3, 5, 0};
    const double scalar[] = {0.5, -1.0, 1.0 / 3};
    const int16_t dxy[] = {10, -10, -20, 30, 7, 9, 1, 2};
    double d[16];
    int rc = gv_deltas(xy, 8, c_off, 3, g_off, 3, t_off, scalar, 3, p_off, index, dxy, 4, d);
    if (rc) return 1;
    std::vector<int32_t> types(64), sizes(8);
    std::vector<double> params(64 * 8);
    rc = gv_outline_var(xy, on, 8, c_off, 3, g_off, 3, glyph, m, pen, sx, sy, 3, t_off, scalar, 3, p_off, index, dxy, 4, types.data(),
                        params.data(), sizes.data());
    std::printf("%d %.17g %.17g %.17g %.17g\n", rc, d[0], d[5], d[12], params[0]);
    return rc;
}
#endif
