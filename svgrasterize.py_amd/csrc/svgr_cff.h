// svgr_cff.h -- OpenType / CFF outlines: the contours a Type 2 charstring draws -- absolute points in double with a kind each
// -- become the lines and cubics of a path, one lane per OUTPUT segment.
//
// Everything a lane does is plain double arithmetic without a data-dependent loop bound, compilable for the host (the CPU
// harness of tests/cff_harness.cpp) and for the device (k_cff_emit of svgr_hip.hip); the search is svgr_textpath.h's
// (textpath_owner), the point transform svgr_glyf.h's (glyf_transform).  cff_tables, the validation walk that also makes the
// segment tables, is host code and shared by the library and the harness.  DESIGN.md 7m has the definitions;
// tests/cff_ref.py restates them in elementwise numpy.
//
//   atlas     every distinct glyph once: pt_xy (double, 2 per point, font units), pt_kind (uint8: 0 MOVE, 1 LINE, 2 C1, 3 C2,
//             4 CURVE, a cubic's end point), contour_off (n_contours + 1, in points), glyph_contour_off (n_glyphs + 1, in
//             contours).  A contour begins with its only MOVE; C1, C2 and CURVE come as that triple
//   part      svgr_glyf.h's: part_glyph, the matrix, pen, sx, sy
//   outline   within a contour a LINE point a gives PATH_LINE p[a-1] -> p[a], a CURVE point a gives PATH_CUBIC p[a-3], p[a-2],
//             p[a-1], p[a]; MOVE, C1 and C2 give nothing.  After the last segment of a contour with at least 2 points comes one
//             PATH_CLOSED line from the contour's last point to its first (of length 0 when the charstring returned to the start
//             itself).  A contour of a lone MOVE gives nothing
//   segments  which points emit is a matter of the kinds alone: seg_ref[s], per atlas segment the index of its end point or,
//             for a closing line, ~contour (negative), and glyph_seg_off are glyph constants, made by cff_tables on the host
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "svgr_glyf.h"

constexpr int CFF_MOVE = 0, CFF_LINE = 1, CFF_C1 = 2, CFF_C2 = 3, CFF_CURVE = 4;

// What an emitting lane reads.
struct CffView {
    const double* pt_xy;             // 2 per atlas point
    const uint8_t* pt_kind;
    const int* seg_ref;              // per atlas segment: its end point, or ~contour for a closing line (cff_tables)
    const int* glyph_seg_off;        // n_glyphs + 1: prefix sums of the glyphs' segment counts (cff_tables)
    const int* contour_off;          // n_contours + 1
    const int* part_glyph;
    const int* part_seg_off;         // n_parts + 1: prefix sums of the parts' segment counts (host-built)
    const double* part_m;            // 6 per part: m00, m01, m10, m11, dx, dy
    const double* part_pen;
    const double* part_sx;
    const double* part_sy;
    int n_contours, n_parts, n_points, n_segs, n_out;
};

// Atlas point a under part p.
GLYF_HD void cff_point(const CffView& v, const GlyfPart& p, int a, double& X, double& Y) {
    double x, y;
    marker_load2(v.pt_xy + 2 * (size_t)a, x, y);
    glyf_transform(p, x, y, X, Y);
}

// Lane j = output segment j: its part, its atlas segment, the 2 or 4 points it reads, one type and one row of 8 doubles.
// false when the tables disagree: an index outside its table (nothing is written then).
GLYF_HD bool cff_emit(const CffView& v, int j, int* types, double* params) {
    if (j < 0 || j >= v.n_out) return false;
    const int k = textpath_owner(v.part_seg_off, v.n_parts, j);
    const int g = v.part_glyph[k];
    const long long s = (long long)v.glyph_seg_off[g] + ((long long)j - v.part_seg_off[k]);
    if (j < v.part_seg_off[k] || j >= v.part_seg_off[k + 1] || s < v.glyph_seg_off[g] || s >= v.glyph_seg_off[g + 1] || s >= v.n_segs)
        return false;
    const int r = v.seg_ref[s];
    int first, last, type;   // the points [first, last] the segment reads
    if (r >= 0) {
        if (r >= v.n_points) return false;
        const int kind = v.pt_kind[r];
        if (kind != CFF_LINE && kind != CFF_CURVE) return false;
        type = kind == CFF_LINE ? SVGR_PATH_LINE : SVGR_PATH_CUBIC;
        first = r - (kind == CFF_LINE ? 1 : 3);
        last = r;
        if (first < 0) return false;
    } else {
        const int c = ~r;
        if (c >= v.n_contours) return false;
        type = SVGR_PATH_CLOSED;
        first = v.contour_off[c];
        last = v.contour_off[c + 1] - 1;
        if (first < 0 || last <= first || last >= v.n_points) return false;
    }
    GlyfPart p;
    {
        const double* m = v.part_m + (size_t)k * 6;
        marker_load2(m, p.m00, p.m01);
        marker_load2(m + 2, p.m10, p.m11);
        marker_load2(m + 4, p.dx, p.dy);
        p.pen = v.part_pen[k];
        p.sx = v.part_sx[k];
        p.sy = v.part_sy[k];
    }
    double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (type == SVGR_PATH_CUBIC) {
        cff_point(v, p, first, o[0], o[1]);
        cff_point(v, p, first + 1, o[2], o[3]);
        cff_point(v, p, first + 2, o[4], o[5]);
        cff_point(v, p, last, o[6], o[7]);
    } else if (type == SVGR_PATH_LINE) {
        cff_point(v, p, first, o[0], o[1]);
        cff_point(v, p, last, o[2], o[3]);
    } else {   // the closing line: from the contour's last point to its first
        cff_point(v, p, last, o[0], o[1]);
        cff_point(v, p, first, o[2], o[3]);
    }
    glyf_store(types, params, j, type, o);
    return true;
}

// The host's side: what svgr_cff_outline checks before anything is launched, and the tables it makes on the way.
struct CffTables {
    std::vector<int32_t> seg_ref;         // n_segs
    std::vector<int32_t> contour_segs;    // n_contours: segments of the contour with its closing line; 0 for a lone MOVE
    std::vector<int32_t> glyph_seg_off;   // n_glyphs + 1
    std::vector<int32_t> part_seg_off;    // n_parts + 1
    std::vector<int32_t> sizes;           // one per contour with segments, in part order then contour order
    const char* why = "";
};

// SVGR_OK, SVGR_E_INVALID or SVGR_E_OVERFLOW (t.why says which).  No array is read beyond the counts given, and none is
// indexed by a value that has not been checked.  The offsets and the parts are glyf_check's to check (svgr_glyf.h).
inline int cff_tables(const double* pt_xy, const uint8_t* pt_kind, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
                      const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m,
                      const double* part_pen, const double* part_sx, const double* part_sy, int64_t n_parts, CffTables& t) {
    if (n_points > 0 && (!pt_xy || !pt_kind)) { t.why = "bad arguments"; return SVGR_E_INVALID; }
    if (int rc = glyf_check(n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen, part_sx, part_sy,
                            n_parts, t.why))
        return rc;
    for (int64_t a = 0; a < n_points; ++a) {
        if (pt_kind[a] > CFF_CURVE) { t.why = "a point kind above 4"; return SVGR_E_INVALID; }
        if (!(std::fabs(pt_xy[2 * a]) <= GLYF_VALUE_MAX) || !(std::fabs(pt_xy[2 * a + 1]) <= GLYF_VALUE_MAX)) {
            t.why = "a coordinate that is not finite or beyond 1e150";
            return SVGR_E_INVALID;
        }
    }
    t.seg_ref.clear();
    t.contour_segs.assign((size_t)n_contours, 0);
    t.glyph_seg_off.assign((size_t)n_glyphs + 1, 0);
    for (int64_t g = 0; g < n_glyphs; ++g) {
        for (int64_t c = glyph_contour_off[g]; c < glyph_contour_off[g + 1]; ++c) {
            const int32_t first = contour_off[c], n = contour_off[c + 1] - first;
            int32_t segs = 0;
            for (int32_t i = 0; i < n; ++i) {
                const int32_t a = first + i;
                const int kind = pt_kind[a];
                if ((i == 0) != (kind == CFF_MOVE)) { t.why = "a contour that does not begin with its only MOVE"; return SVGR_E_INVALID; }
                if (kind == CFF_C1 && !(i + 2 < n && pt_kind[a + 1] == CFF_C2 && pt_kind[a + 2] == CFF_CURVE)) {
                    t.why = "a C1 that C2 and CURVE do not follow";
                    return SVGR_E_INVALID;
                }
                if (kind == CFF_C2 && !(i >= 2 && pt_kind[a - 1] == CFF_C1)) { t.why = "a C2 without its C1"; return SVGR_E_INVALID; }
                if (kind == CFF_CURVE && !(i >= 3 && pt_kind[a - 1] == CFF_C2)) { t.why = "a CURVE without its C1 and C2"; return SVGR_E_INVALID; }
                if (kind == CFF_LINE || kind == CFF_CURVE) {
                    t.seg_ref.push_back(a);
                    ++segs;
                }
            }
            if (n >= 2) {
                t.seg_ref.push_back(~(int32_t)c);
                ++segs;
            }
            t.contour_segs[(size_t)c] = segs;
        }
        t.glyph_seg_off[(size_t)g + 1] = (int32_t)t.seg_ref.size();   // (at most n_points + n_contours <= 2 GLYF_COUNT_MAX)
    }
    t.part_seg_off.assign((size_t)n_parts + 1, 0);
    t.sizes.clear();
    int64_t segs = 0;
    for (int64_t k = 0; k < n_parts; ++k) {
        const int32_t g = part_glyph[k];
        segs += t.glyph_seg_off[(size_t)g + 1] - t.glyph_seg_off[(size_t)g];
        if (segs > GLYF_COUNT_MAX) { t.why = "the segments do not fit a 32-bit count"; return SVGR_E_OVERFLOW; }
        t.part_seg_off[(size_t)k + 1] = (int32_t)segs;
        for (int32_t c = glyph_contour_off[g]; c < glyph_contour_off[g + 1]; ++c)
            if (t.contour_segs[(size_t)c] > 0) t.sizes.push_back(t.contour_segs[(size_t)c]);
    }
    return SVGR_OK;
}
