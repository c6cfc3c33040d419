// svgr_gvar.h -- variable fonts (`gvar`): the delta of every atlas point at one instance of the font, one lane per point.
//
// Everything a lane does is plain double arithmetic; the only loop whose length depends on the data is the one over the
// glyph's tuples, every search is a binary search of at most 31 steps.  Compilable for the host (tests/gvar_harness.cpp) and
// for the device (k_gvar_delta of svgr_hip.hip).  gvar_tables, the validation walk, is host code and shared by the library
// and the harness.  DESIGN.md, "Variable fonts", has the definitions; tests/gvar_ref.py restates them in elementwise numpy.
//
//   atlas     svgr_glyf.h's: pt_xy (int16, 2 per point), contour_off (n_contours + 1, in points), glyph_contour_off
//             (n_glyphs + 1, in contours)
//   tuples    glyph g owns the tuples [glyph_tuple_off[g], glyph_tuple_off[g + 1]), in the file's order; tuple t has the scalar
//             tuple_scalar[t] (the host's: the instance is in it) and the entries [tuple_pt_off[t], tuple_pt_off[t + 1]):
//             tp_index, the point's index within its glyph, strictly increasing within the tuple, and tp_dxy (int16, 2 per entry)
//   delta     of point i of a contour that owns the glyph-local indices [f, l], in one tuple: the entries whose index lies in
//             [f, l] are the contour's touched points; none: (0, 0); i among them: its stored delta; else, with p the touched
//             point before i (cyclic: the contour's last touched one) and q the one after (cyclic: the first), per axis from the
//             default outline's coordinates c_p, c_q, c_i and the deltas d_p, d_q: c_p == c_q gives d_p when d_p == d_q, else 0;
//             otherwise with the pair ordered so that c_1 < c_2: d_1 when c_i <= c_1, d_2 when c_i >= c_2, else
//             d_1 + (c_i - c_1) * ((d_2 - d_1) / (c_2 - c_1)), the product rounded before the sum
//   sum       D = 0.0, then D = D + scalar_t * delta_t for every tuple of the glyph in order: one product, one sum, each rounded
#pragma once
#include <cmath>
#include <cstdint>

#include "svgr_textpath.h"

#if defined(__HIPCC__)
#define GVAR_HD __host__ __device__ inline
#else
#define GVAR_HD inline
#endif

constexpr int64_t GVAR_COUNT_MAX = INT32_MAX / 2;

// What a lane reads.
struct GvarView {
    const int16_t* pt_xy;            // 2 per atlas point
    const int* contour_off;          // n_contours + 1
    const int* glyph_contour_off;    // n_glyphs + 1
    const int* glyph_tuple_off;      // n_glyphs + 1
    const double* tuple_scalar;      // n_tuples
    const int* tuple_pt_off;         // n_tuples + 1
    const int* tp_index;             // glyph-local point index of every entry
    const int16_t* tp_dxy;           // 2 per entry
    int n_contours, n_glyphs, n_points, n_tuples;
};

// The first position in [b, e) whose index is not below `key` (e when there is none); idx ascending there.
GVAR_HD int gvar_lower(const int* idx, int b, int e, int key) {
    const int len = e - b;
    if (len < 1) return b;
    int pos = b;   // every entry in front of pos is below key
    for (int step = 1 << (31 - __builtin_clz((unsigned)len)); step >= 1; step >>= 1) {
        const int at = pos + step;
        const int v = idx[at <= e ? at - 1 : b];
        const bool take = at <= e && v < key;
        pos = take ? at : pos;
    }
    return pos;
}

// One axis of an untouched point between the touched points p and q.
GVAR_HD double gvar_iup(double cp, double cq, double ci, double dp, double dq) {
    if (cp == cq) return dp == dq ? dp : 0.0;
    const bool swap = cp > cq;
    const double c1 = swap ? cq : cp, c2 = swap ? cp : cq, d1 = swap ? dq : dp, d2 = swap ? dp : dq;
    if (ci <= c1) return d1;
    if (ci >= c2) return d2;
    const double s = (d2 - d1) / (c2 - c1);
    const double prod = (ci - c1) * s;
    return d1 + prod;
}

// The delta of atlas point a, summed over its glyph's tuples.  false when the tables disagree (a point outside its contour
// or a tuple range outside the tables): dx = dy = 0 then.
GVAR_HD bool gvar_delta(const GvarView& v, int a, double& dx, double& dy) {
    dx = 0.0;
    dy = 0.0;
    if (a < 0 || a >= v.n_points) return false;
    const int c = textpath_owner(v.contour_off, v.n_contours, a);
    const int first = v.contour_off[c], n = v.contour_off[c + 1] - first;
    if (a < first || a >= first + n) return false;
    const int g = textpath_owner(v.glyph_contour_off, v.n_glyphs, c);
    if (c < v.glyph_contour_off[g] || c >= v.glyph_contour_off[g + 1]) return false;
    const int base = v.contour_off[v.glyph_contour_off[g]];   // the glyph's first atlas point
    const int f = first - base, l = f + n - 1, i = a - base;
    const int t0 = v.glyph_tuple_off[g], t1 = v.glyph_tuple_off[g + 1];
    if (t0 < 0 || t1 > v.n_tuples) return false;
    const double ci_x = (double)v.pt_xy[2 * (size_t)a], ci_y = (double)v.pt_xy[2 * (size_t)a + 1];
    for (int t = t0; t < t1; ++t) {
        const int b = v.tuple_pt_off[t], e = v.tuple_pt_off[t + 1];
        const int lo = gvar_lower(v.tp_index, b, e, f), hi = gvar_lower(v.tp_index, lo, e, l + 1);
        double tx = 0.0, ty = 0.0;
        if (lo < hi) {
            const int pos = gvar_lower(v.tp_index, lo, hi, i);
            if (pos < hi && v.tp_index[pos] == i) {
                tx = (double)v.tp_dxy[2 * (size_t)pos];
                ty = (double)v.tp_dxy[2 * (size_t)pos + 1];
            } else {
                const int p = pos > lo ? pos - 1 : hi - 1, q = pos < hi ? pos : lo;
                const size_t ap = (size_t)base + (size_t)v.tp_index[p], aq = (size_t)base + (size_t)v.tp_index[q];
                tx = gvar_iup((double)v.pt_xy[2 * ap], (double)v.pt_xy[2 * aq], ci_x, (double)v.tp_dxy[2 * (size_t)p],
                              (double)v.tp_dxy[2 * (size_t)q]);
                ty = gvar_iup((double)v.pt_xy[2 * ap + 1], (double)v.pt_xy[2 * aq + 1], ci_y, (double)v.tp_dxy[2 * (size_t)p + 1],
                              (double)v.tp_dxy[2 * (size_t)q + 1]);
            }
        }
        const double s = v.tuple_scalar[t];
        const double px = s * tx, py = s * ty;
        dx = dx + px;
        dy = dy + py;
    }
    return true;
}

// The host's side: what svgr_gvar_deltas and svgr_glyf_outline_var check before anything is launched.  SVGR_OK,
// SVGR_E_INVALID or SVGR_E_OVERFLOW (`why` says which).  No array is read beyond the counts given, and none is indexed by a
// value that has not been checked.
inline int gvar_tables(int64_t n_points, const int32_t* contour_off, int64_t n_contours, const int32_t* glyph_contour_off, int64_t n_glyphs,
                       const int32_t* glyph_tuple_off, const double* tuple_scalar, int64_t n_tuples, const int32_t* tuple_pt_off,
                       const int32_t* tp_index, const int16_t* tp_dxy, int64_t n_entries, const char*& why) {
    why = "";
    if (n_points < 0 || n_contours < 0 || n_glyphs < 0 || n_tuples < 0 || n_entries < 0 || !contour_off || !glyph_contour_off ||
        !glyph_tuple_off || !tuple_pt_off || (n_tuples > 0 && !tuple_scalar) || (n_entries > 0 && (!tp_index || !tp_dxy))) {
        why = "bad arguments";
        return SVGR_E_INVALID;
    }
    if (n_points > GVAR_COUNT_MAX || n_contours > GVAR_COUNT_MAX || n_glyphs > GVAR_COUNT_MAX || n_tuples > GVAR_COUNT_MAX ||
        n_entries > GVAR_COUNT_MAX) {
        why = "a count does not fit 32 bits";
        return SVGR_E_OVERFLOW;
    }
    if (contour_off[0] != 0 || glyph_contour_off[0] != 0 || glyph_tuple_off[0] != 0 || tuple_pt_off[0] != 0) {
        why = "offsets that do not begin at 0";
        return SVGR_E_INVALID;
    }
    for (int64_t c = 0; c < n_contours; ++c)
        if (contour_off[c + 1] < contour_off[c]) { why = "contour offsets that decrease"; return SVGR_E_INVALID; }
    if (contour_off[n_contours] != n_points) { why = "contour offsets that do not end at the point count"; return SVGR_E_INVALID; }
    for (int64_t g = 0; g < n_glyphs; ++g)
        if (glyph_contour_off[g + 1] < glyph_contour_off[g]) { why = "glyph offsets that decrease"; return SVGR_E_INVALID; }
    if (glyph_contour_off[n_glyphs] != n_contours) { why = "glyph offsets that do not end at the contour count"; return SVGR_E_INVALID; }
    for (int64_t g = 0; g < n_glyphs; ++g)
        if (glyph_tuple_off[g + 1] < glyph_tuple_off[g]) { why = "glyph tuple offsets that decrease"; return SVGR_E_INVALID; }
    if (glyph_tuple_off[n_glyphs] != n_tuples) { why = "glyph tuple offsets that do not end at the tuple count"; return SVGR_E_INVALID; }
    for (int64_t t = 0; t < n_tuples; ++t)
        if (tuple_pt_off[t + 1] < tuple_pt_off[t]) { why = "tuple point offsets that decrease"; return SVGR_E_INVALID; }
    if (tuple_pt_off[n_tuples] != n_entries) { why = "tuple point offsets that do not end at the entry count"; return SVGR_E_INVALID; }
    for (int64_t t = 0; t < n_tuples; ++t)
        if (!(std::fabs(tuple_scalar[t]) <= 1.0)) { why = "a tuple scalar that is not finite or lies outside [-1, 1]"; return SVGR_E_INVALID; }
    for (int64_t g = 0; g < n_glyphs; ++g) {
        const int32_t count = contour_off[glyph_contour_off[g + 1]] - contour_off[glyph_contour_off[g]];   // the glyph's points
        for (int64_t t = glyph_tuple_off[g]; t < glyph_tuple_off[g + 1]; ++t)
            for (int64_t k = tuple_pt_off[t]; k < tuple_pt_off[t + 1]; ++k) {
                if (tp_index[k] < 0 || tp_index[k] >= count) { why = "a tuple's point index outside its glyph"; return SVGR_E_INVALID; }
                if (k > tuple_pt_off[t] && tp_index[k] <= tp_index[k - 1]) {
                    why = "a tuple's point indices that do not increase strictly";
                    return SVGR_E_INVALID;
                }
            }
    }
    return SVGR_OK;
}
