// svgr_glyf.h -- TrueType (`glyf`) outlines: the contours of simple glyphs -- int16 points with an on-curve flag each -- become
// the lines and cubics of a path, one lane per (part, point) pair.
//
// Everything a lane does is plain double arithmetic without a data-dependent loop bound, compilable for the host (the CPU
// harness of tests/glyf_harness.cpp) and for the device (k_glyf_emit of svgr_hip.hip); the searches are svgr_textpath.h's
// (textpath_owner).  glyf_tables, the validation walk that also makes the slot tables, is host code and shared by the library
// and the harness.  DESIGN.md, "TrueType fonts", has the definitions; tests/ttf_ref.py restates them in elementwise numpy.
//
//   atlas     every distinct simple glyph once: pt_xy (int16, 2 per point), pt_on (uint8, non-zero: on the curve),
//             contour_off (n_contours + 1, in points), glyph_contour_off (n_glyphs + 1, in contours)
//   part      one placed simple glyph: part_glyph, the matrix (m00, m01, m10, m11, dx, dy) in font units, pen, sx, sy.  A point
//             (x, y) goes to x' = (m00 x + m10 y) + dx, y' = (m01 x + m11 y) + dy, then X = (x' + pen) sx, Y = y' sy
//   outline   contour p[0..n-1], prev / next cyclic; n < 2 gives nothing.  An off-curve p[i] emits the quadratic from (prev if
//             on, else the midpoint of prev and p[i]) over p[i] to (next if on, else the midpoint of p[i] and next); an on-curve
//             p[i] with an on-curve next emits the line p[i] -> next; an on-curve p[i] with an off-curve next emits nothing.
//             After the contour's last segment comes one PATH_CLOSED line of length 0 at the chain's start: p[0] if on, else
//             p[n-1] if on, else their midpoint.  Midpoints are (a + b) * 0.5 in font units (exact in double for the int16
//             points; with the deltas of a variable font's instance, pt_dxy, one rounded sum and an exact halving); a quadratic
//             P0 Q P1 is stored as the cubic P0, (1/3) P0 + (2/3) Q, (2/3) Q + (1/3) P1, P1 made from the transformed points
//   slots     whether a point emits is a matter of the flags alone: pt_slot[a], the place of point a's segment among the
//             segments of its glyph, and contour_segs[c] are glyph constants, made by glyf_tables on the host
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "svgr_textpath.h"

#if defined(__HIPCC__)
#define GLYF_HD __host__ __device__ inline
#else
#define GLYF_HD inline
#endif

constexpr double GLYF_VALUE_MAX = 1e150;   // a matrix entry, pen or scale beyond it is refused (the products stay finite)
constexpr int64_t GLYF_COUNT_MAX = INT32_MAX / 2;

// What an emitting lane reads.
struct GlyfView {
    const int16_t* pt_xy;            // 2 per atlas point
    const uint8_t* pt_on;
    const int* pt_slot;              // per atlas point: segments of its glyph in front of its own (glyf_tables)
    const int* contour_off;          // n_contours + 1
    const int* glyph_contour_off;    // n_glyphs + 1
    const int* part_glyph;
    const int* part_lane_off;        // n_parts + 1: prefix sums of the parts' point counts (host-built)
    const int* part_seg_off;         // n_parts + 1: prefix sums of the parts' segment counts (host-built)
    const double* part_m;            // 6 per part: m00, m01, m10, m11, dx, dy
    const double* part_pen;
    const double* part_sx;
    const double* part_sy;
    int n_contours, n_parts, n_points, n_out;
    const double* pt_dxy;            // 2 per atlas point, or null: the deltas of a variable font's instance (svgr_gvar.h)
};

struct GlyfPart { double m00, m01, m10, m11, dx, dy, pen, sx, sy; };

GLYF_HD void glyf_transform(const GlyfPart& p, double x, double y, double& X, double& Y) {
    const double xp = (p.m00 * x + p.m10 * y) + p.dx;
    const double yp = (p.m01 * x + p.m11 * y) + p.dy;
    X = (xp + p.pen) * p.sx;
    Y = yp * p.sy;
}

// Atlas point a in font units: the int16 point, plus its delta at an instance of a variable font.
GLYF_HD void glyf_point(const GlyfView& v, int a, double& x, double& y) {
    x = (double)v.pt_xy[2 * (size_t)a];
    y = (double)v.pt_xy[2 * (size_t)a + 1];
    if (v.pt_dxy) {
        double dx, dy;
        marker_load2(v.pt_dxy + 2 * (size_t)a, dx, dy);
        x = x + dx;
        y = y + dy;
    }
}

GLYF_HD void glyf_store(int* types, double* params, long long slot, int type, const double* o) {
    types[slot] = type;
    double* at = params + (size_t)slot * 8;
    for (int e = 0; e < 8; e += 2) marker_store2(at + e, o[e], o[e + 1]);
}

// Lane j: its part, its atlas point, the segment that point emits (none, or one) and, for the last point of a contour, the
// closing line.  false when the tables disagree: a lane or a slot outside its range (nothing is written there).
GLYF_HD bool glyf_emit(const GlyfView& v, int j, int* types, double* params) {
    const int k = textpath_owner(v.part_lane_off, v.n_parts, j);
    const int c0 = v.glyph_contour_off[v.part_glyph[k]];
    const long long q = (long long)j - v.part_lane_off[k];
    const long long al = (long long)v.contour_off[c0] + q;
    if (q < 0 || j >= v.part_lane_off[k + 1] || al < 0 || al >= v.n_points) return false;
    const int a = (int)al;
    const int c = textpath_owner(v.contour_off, v.n_contours, a);
    const int first = v.contour_off[c], n = v.contour_off[c + 1] - first;
    if (a < first || a >= first + n) return false;
    if (n < 2) return true;
    const int i = a - first;
    const bool last = i == n - 1;
    const int ap = i == 0 ? first + n - 1 : a - 1, an = last ? first : a + 1;
    const bool on = v.pt_on[a] != 0, on_p = v.pt_on[ap] != 0, on_n = v.pt_on[an] != 0;
    const bool emits = !on || on_n;
    if (!emits && !last) return true;
    double x, y, xn, yn;
    glyf_point(v, a, x, y);
    glyf_point(v, an, xn, yn);
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
    const long long slot = (long long)v.part_seg_off[k] + v.pt_slot[a];
    if (emits) {
        if (slot < v.part_seg_off[k] || slot >= v.part_seg_off[k + 1] || slot >= v.n_out) return false;
        double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (on) {   // the line p[i] -> next
            glyf_transform(p, x, y, o[0], o[1]);
            glyf_transform(p, xn, yn, o[2], o[3]);
            glyf_store(types, params, slot, SVGR_PATH_LINE, o);
        } else {    // the quadratic over p[i]
            double xp, yp;
            glyf_point(v, ap, xp, yp);
            const double sx = on_p ? xp : (xp + x) * 0.5, sy = on_p ? yp : (yp + y) * 0.5;
            const double ex = on_n ? xn : (x + xn) * 0.5, ey = on_n ? yn : (y + yn) * 0.5;
            double qx, qy;
            glyf_transform(p, sx, sy, o[0], o[1]);
            glyf_transform(p, x, y, qx, qy);
            glyf_transform(p, ex, ey, o[6], o[7]);
            o[2] = (1.0 / 3) * o[0] + (2.0 / 3) * qx;
            o[3] = (1.0 / 3) * o[1] + (2.0 / 3) * qy;
            o[4] = (2.0 / 3) * qx + (1.0 / 3) * o[6];
            o[5] = (2.0 / 3) * qy + (1.0 / 3) * o[7];
            glyf_store(types, params, slot, SVGR_PATH_CUBIC, o);
        }
    }
    if (last) {   // (next is p[0] here) the closing line, of length 0, at the chain's start
        const long long cs = slot + (emits ? 1 : 0);
        if (cs < v.part_seg_off[k] || cs >= v.part_seg_off[k + 1] || cs >= v.n_out) return false;
        const double sx = on_n ? xn : (on ? x : (x + xn) * 0.5), sy = on_n ? yn : (on ? y : (y + yn) * 0.5);
        double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        glyf_transform(p, sx, sy, o[0], o[1]);
        o[2] = o[0];
        o[3] = o[1];
        glyf_store(types, params, cs, SVGR_PATH_CLOSED, o);
    }
    return true;
}

// The host's side: what svgr_glyf_outline checks before anything is launched, and the tables it makes on the way.
struct GlyfTables {
    std::vector<int32_t> pt_slot;         // n_points
    std::vector<int32_t> contour_segs;    // n_contours: segments of the contour with its closing line; 0 for n < 2
    std::vector<int32_t> glyph_segs;      // n_glyphs
    std::vector<int32_t> part_lane_off;   // n_parts + 1
    std::vector<int32_t> part_seg_off;    // n_parts + 1
    std::vector<int32_t> sizes;           // one per contour with n >= 2, in part order then contour order
    const char* why = "";
};

// What the outline passes of both formats (svgr_cff.h too) check of the offsets and the parts: SVGR_OK, SVGR_E_INVALID or
// SVGR_E_OVERFLOW (why says which).  No array is read beyond the counts given.
inline int glyf_check(int64_t n_points, const int32_t* contour_off, int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs,
                      const int32_t* part_glyph, const double* part_m, const double* part_pen, const double* part_sx, const double* part_sy,
                      int64_t n_parts, const char*& why) {
    if (n_points < 0 || n_contours < 0 || n_glyphs < 0 || n_parts < 0 || !contour_off || !glyph_contour_off ||
        (n_parts > 0 && (!part_glyph || !part_m || !part_pen || !part_sx || !part_sy))) {
        why = "bad arguments";
        return SVGR_E_INVALID;
    }
    if (n_points > GLYF_COUNT_MAX || n_contours > GLYF_COUNT_MAX || n_glyphs > GLYF_COUNT_MAX || n_parts > GLYF_COUNT_MAX) {
        why = "a count does not fit 32 bits";
        return SVGR_E_OVERFLOW;
    }
    if (contour_off[0] != 0 || glyph_contour_off[0] != 0) { why = "offsets that do not begin at 0"; return SVGR_E_INVALID; }
    for (int64_t c = 0; c < n_contours; ++c)
        if (contour_off[c + 1] < contour_off[c]) { why = "contour offsets that decrease"; return SVGR_E_INVALID; }
    if (contour_off[n_contours] != n_points) { why = "contour offsets that do not end at the point count"; return SVGR_E_INVALID; }
    for (int64_t g = 0; g < n_glyphs; ++g)
        if (glyph_contour_off[g + 1] < glyph_contour_off[g]) { why = "glyph offsets that decrease"; return SVGR_E_INVALID; }
    if (glyph_contour_off[n_glyphs] != n_contours) { why = "glyph offsets that do not end at the contour count"; return SVGR_E_INVALID; }
    for (int64_t k = 0; k < n_parts; ++k) {
        if (part_glyph[k] < 0 || part_glyph[k] >= n_glyphs) { why = "a part's glyph id out of range"; return SVGR_E_INVALID; }
        bool ok = std::fabs(part_pen[k]) <= GLYF_VALUE_MAX && std::fabs(part_sx[k]) <= GLYF_VALUE_MAX && std::fabs(part_sy[k]) <= GLYF_VALUE_MAX;
        for (int e = 0; e < 6; ++e) ok = ok && std::fabs(part_m[6 * k + e]) <= GLYF_VALUE_MAX;
        if (!ok) { why = "a matrix, pen or scale that is not finite or beyond 1e150"; return SVGR_E_INVALID; }
    }
    return SVGR_OK;
}

// SVGR_OK, SVGR_E_INVALID or SVGR_E_OVERFLOW (t.why says which).  No array is read beyond the counts given, and none is
// indexed by a value that has not been checked.
inline int glyf_tables(const uint8_t* pt_on, int64_t n_points, const int32_t* contour_off, int64_t n_contours,
                       const int32_t* glyph_contour_off, int64_t n_glyphs, const int32_t* part_glyph, const double* part_m,
                       const double* part_pen, const double* part_sx, const double* part_sy, int64_t n_parts, GlyfTables& t) {
    if (n_points > 0 && !pt_on) { t.why = "bad arguments"; return SVGR_E_INVALID; }
    if (int rc = glyf_check(n_points, contour_off, n_contours, glyph_contour_off, n_glyphs, part_glyph, part_m, part_pen, part_sx, part_sy,
                            n_parts, t.why))
        return rc;
    // the slot of every point and the segment count of every contour: the flags alone decide
    t.pt_slot.assign((size_t)n_points, 0);
    t.contour_segs.assign((size_t)n_contours, 0);
    t.glyph_segs.assign((size_t)n_glyphs, 0);
    for (int64_t g = 0; g < n_glyphs; ++g) {
        int32_t s = 0;
        for (int64_t c = glyph_contour_off[g]; c < glyph_contour_off[g + 1]; ++c) {
            const int32_t first = contour_off[c], n = contour_off[c + 1] - first, s0 = s;
            for (int32_t i = 0; i < n; ++i) {
                const int32_t a = first + i, an = i == n - 1 ? first : a + 1;
                t.pt_slot[(size_t)a] = s;
                if (n >= 2 && (pt_on[a] == 0 || pt_on[an] != 0)) ++s;
            }
            if (n >= 2) ++s;
            t.contour_segs[(size_t)c] = s - s0;
        }
        t.glyph_segs[(size_t)g] = s;
    }
    t.part_lane_off.assign((size_t)n_parts + 1, 0);
    t.part_seg_off.assign((size_t)n_parts + 1, 0);
    t.sizes.clear();
    int64_t lanes = 0, segs = 0;
    for (int64_t k = 0; k < n_parts; ++k) {
        const int32_t g = part_glyph[k], c0 = glyph_contour_off[g], c1 = glyph_contour_off[g + 1];
        lanes += contour_off[c1] - contour_off[c0];
        segs += t.glyph_segs[(size_t)g];
        if (lanes > GLYF_COUNT_MAX || segs > GLYF_COUNT_MAX) { t.why = "the lanes or the segments do not fit a 32-bit count"; return SVGR_E_OVERFLOW; }
        t.part_lane_off[(size_t)k + 1] = (int32_t)lanes;
        t.part_seg_off[(size_t)k + 1] = (int32_t)segs;
        for (int32_t c = c0; c < c1; ++c)
            if (t.contour_segs[(size_t)c] > 0) t.sizes.push_back(t.contour_segs[(size_t)c]);
    }
    return SVGR_OK;
}
