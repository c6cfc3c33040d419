// cff_harness.cpp -- the CFF outline per-lane header (csrc/svgr_cff.h) compiled for the host, for tests/test_cff_host.py
// (g++ -ffp-contract=off): the library's validation walk with its tables, then the lanes of k_cff_emit one after the other.
// With CFF_HARNESS_MAIN it is a program of its own (a sanitizer build runs that).
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_cff.h"

extern "C" {

// The validation of svgr_cff_outline: its status, and the counts of segments (= lanes) and subpaths.
int ch_validate(const double* pt_xy, const uint8_t* pt_kind, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
                const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m, const double* part_pen,
                const double* part_sx, const double* part_sy, int64_t n_parts, int64_t* counts2) {
    CffTables t;
    const int rc = cff_tables(pt_xy, pt_kind, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen,
                              part_sx, part_sy, n_parts, t);
    counts2[0] = counts2[1] = 0;
    if (rc) return rc;
    counts2[0] = t.part_seg_off[(size_t)n_parts];
    counts2[1] = (int64_t)t.sizes.size();
    return 0;
}

// svgr_cff_outline into arrays of ch_validate's counts: types, params (8 per segment), sizes.  SVGR_E_STATE when a lane met an
// index outside its tables.
int ch_outline(const double* pt_xy, const uint8_t* pt_kind, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
               const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m, const double* part_pen,
               const double* part_sx, const double* part_sy, int64_t n_parts, int32_t* types, double* params, int32_t* sizes) {
    CffTables t;
    if (int rc = cff_tables(pt_xy, pt_kind, n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen,
                            part_sx, part_sy, n_parts, t))
        return rc;
    const int n_out = t.part_seg_off[(size_t)n_parts];
    const CffView v{pt_xy, pt_kind, t.seg_ref.data(), t.glyph_seg_off.data(), contour_off, part_glyph, t.part_seg_off.data(), part_m, part_pen,
                    part_sx, part_sy, (int)n_contours, (int)n_parts, (int)n_points, (int)t.seg_ref.size(), n_out};
    bool ok = true;
    for (int j = 0; j < n_out; ++j) ok = cff_emit(v, j, types, params) && ok;
    for (size_t s = 0; s < t.sizes.size(); ++s) sizes[s] = t.sizes[s];
    return ok ? 0 : SVGR_E_STATE;
}

}  // extern "C"

#if defined(CFF_HARNESS_MAIN)
#include <cstdio>
int main() {
    // glyph 0: a triangle of lines that returns to its start, and a contour of one cubic; glyph 1: empty; glyph 2: a lone MOVE
    const double xy[] = {0, 0, 100, 0, 50, 80.5, 0, 0, 10, 10, 20, 30, 40, 30, 50, 10, 7, 7};
    const uint8_t kind[] = {0, 1, 1, 1, 0, 2, 3, 4, 0};
    const int32_t c_off[] = {0, 4, 8, 9}, g_off[] = {0, 2, 2, 3}, glyph[] = {1, 0, 2, 0};
    const double m[] = {1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0.5, 0.25, -0.25, 0.5, 10, -10};
    const double pen[] = {0, 10, 200, 300}, sx[] = {0.01, 0.01, 0.01, 0.01}, sy[] = {-0.01, -0.01, -0.01, 0.01};
    int64_t counts[2];
    int rc = ch_validate(xy, kind, 9, c_off, 3, g_off, 3, glyph, m, pen, sx, sy, 4, counts);
    if (rc) return 1;
    std::vector<int32_t> types((size_t)counts[0]), sizes((size_t)counts[1]);
    std::vector<double> params((size_t)counts[0] * 8);
    rc = ch_outline(xy, kind, 9, c_off, 3, g_off, 3, glyph, m, pen, sx, sy, 4, types.data(), params.data(), sizes.data());
    std::printf("%d %lld %lld %.17g\n", rc, (long long)counts[0], (long long)counts[1], params[params.size() - 8]);
    return rc;
}
#endif
