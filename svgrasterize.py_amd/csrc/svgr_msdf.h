// svgr_msdf.h -- per-lane arithmetic of multi-channel distance fields: three channels (R, G, B) that each keep the nearest edge of
// one colour and report the signed distance to that edge's LINE (a pseudo-distance), so that their median keeps a corner sharp
// where svgr_sdf.h's single field rounds it, plus the true signed distance of svgr_sdf.h in a fourth channel (A).
//
// Plain double arithmetic on top of svgr_sdf.h, compilable for the host (tests/msdf_harness.cpp) and for the device
// (k_msdf_distance of svgr_hip.hip), both with -ffp-contract=off: every product and every sum is rounded on its own.  DESIGN.md 7s
// has the definitions; tests/msdf_ref.py restates them in numpy.
//
//   prepared  per EDGE, once (MSDF_EDGE_DOUBLES = 8):  a0, b0, x, y, inv, a1, b1, rl -- x, y, inv as sdf_edge_prepare has them,
//             rl = len2 > 0 ? 1.0 / sqrt(len2) : 0.0, the division and the square root each rounded on its own
//   candidate of an edge for a colour channel, at a FINITE point.  An edge with rl == 0 (len2 == 0; or len2 beyond the doubles) is
//             none; it still counts for A.
//               da = pa - a0;  db = pb - b0;  s = da*x + db*y;  t = s * inv                         (t is NOT clamped)
//               t <= 0:     d2c = da*da + db*db;                               se = s
//               t >= 1:     ea = pa - a1;  eb = pb - b1;  d2c = ea*ea + eb*eb;  se = ea*x + eb*y
//               otherwise:  d2c = sdf_edge_d2(...);                            se = 0
//               o    = (se*se) * inv        the squared cosine between the edge and the direction to the point, up to a factor
//                                           common to all edges that meet at that vertex
//               perp = (x*db - da*y) * rl   (sdf_edge_term's two products): the signed distance to the edge's line
//             The end-point cases measure to the STORED end point, not to a0 + 1*x: two edges that share a vertex give the same
//             d2c, bit for bit, and the tie goes to `o`.
//   better    a candidate replaces the kept one when d2c < best_d2, or d2c == best_d2 and o < best_o (the edge that faces the
//             point), or both are equal and perp > best_perp (so that the result does not depend on the order of the edges: the
//             kept edge set has none within a path).  A channel that has kept nothing has best_d2 = +inf.
//   group     one shape: a run of paths, each with a colour mask (bit 0 R, bit 1 G, bit 2 B; 1 .. 7), one fill rule, and an
//             orientation sigma = +1 / -1 chosen by the caller so that sigma * (x*db - da*y) > 0 inside a well-oriented outline.
//               A          sdf_finish(min sdf_edge_d2, sum sdf_edge_term) over ALL edges of the group: svgr_sdf.h's signed distance
//               channel c  keeps the best candidate among the edges of the paths whose mask has bit c; its value is A when it has
//                          kept nothing, when the point is not finite, or when the spread is finite and best_d2 >= spread*spread
//                          (the guard: DESIGN.md 7s); else sdf_clamp(-sigma * best_perp, spread)
//   repair    m = median(r, g, b); if ((m < 0) != (A < 0)) r = g = b = A: the side the median reports is the side A reports
//   union     per channel the minimum over the groups, from +spread (a skipped or empty group, or no group at all, is +spread)
//   encoding  svgr_sdf.h's, per channel; four values to a point: R, G, B, A
#pragma once
#include "svgr_sdf.h"

constexpr int MSDF_EDGE_DOUBLES = 8;   // a staged edge: a0, b0, x, y, inv, a1, b1, rl

// an edge as the inner loop wants it: out[0 .. 8) = a0, b0, x, y, inv, a1, b1, rl
HIT_HD void msdf_edge_prepare(double a0, double b0, double a1, double b1, double* out) {
    double q[SDF_EDGE_DOUBLES];
    sdf_edge_prepare(a0, b0, a1, b1, q);
    const double xx = q[2] * q[2], yy = q[3] * q[3];
    const double len2 = xx + yy;
    double rl = 0.0;
    if (len2 > 0.0) {
        const double len = sqrt(len2);
        rl = 1.0 / len;
    }
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3]; out[4] = q[4];
    out[5] = a1; out[6] = b1; out[7] = rl;
}

// what a lane keeps of one group: A's min d2 and winding number, and per channel the best candidate
struct MsdfState {
    double m;
    int w;
    double d2[3], o[3], perp[3];
};

HIT_HD void msdf_begin(MsdfState& s) {
    s.m = INFINITY;
    s.w = 0;
    for (int c = 0; c < 3; ++c) { s.d2[c] = INFINITY; s.o[c] = INFINITY; s.perp[c] = -INFINITY; }
}

// one prepared edge of a path with colour `mask` against the point (a NaN point leaves the state as it is: every compare is false)
HIT_HD void msdf_edge(MsdfState& s, int mask, double a0, double b0, double x, double y, double inv, double a1, double b1, double rl,
                      double pa, double pb) {
    const double da = pa - a0, db = pb - b0;
    const double d2 = sdf_edge_d2(a0, b0, x, y, inv, pa, pb, da, db);
    s.m = fmin(s.m, d2);
    s.w += sdf_edge_term(b0, b1, x, y, pb, da, db);
    const double m0 = da * x, m1 = db * y;
    const double sp = m0 + m1;
    const double t = sp * inv;
    double d2c = d2, se = 0.0;
    if (t <= 0.0) {
        const double da2 = da * da, db2 = db * db;
        d2c = da2 + db2;
        se = sp;
    } else if (t >= 1.0) {
        const double ea = pa - a1, eb = pb - b1;
        const double ea2 = ea * ea, eb2 = eb * eb;
        d2c = ea2 + eb2;
        const double n0 = ea * x, n1 = eb * y;
        se = n0 + n1;
    }
    const double se2 = se * se;
    const double o = se2 * inv;
    const double c0 = x * db, c1 = da * y;
    const double cr = c0 - c1;
    const double perp = cr * rl;
    const bool candidate = rl > 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c)
        if (mask >> c & 1) {
            const bool better = d2c < s.d2[c] || (d2c == s.d2[c] && (o < s.o[c] || (o == s.o[c] && perp > s.perp[c])));
            if (candidate && better) { s.d2[c] = d2c; s.o[c] = o; s.perp[c] = perp; }
        }
}

HIT_HD double msdf_median(double r, double g, double b) {
    const double lo = r < g ? r : g, hi = r < g ? g : r;
    const double mid = hi < b ? hi : b;
    return lo < mid ? mid : lo;
}

// the group's four clamped values at the point: out[0 .. 4) = R, G, B, A; `sigma` is +1 or -1
HIT_HD void msdf_finish(const MsdfState& s, int evenodd, int sigma, double spread, bool finite, double* out) {
    const double a = sdf_finish(s.m, s.w, evenodd, 1, spread);
    const double reach = spread * spread;
    for (int c = 0; c < 3; ++c) {
        const bool own = finite && s.d2[c] < INFINITY && !(spread < INFINITY && s.d2[c] >= reach);
        const double pseudo = sigma > 0 ? -s.perp[c] : s.perp[c];
        out[c] = own ? sdf_clamp(pseudo, spread) : a;
    }
    const double med = msdf_median(out[0], out[1], out[2]);
    if ((med < 0.0) != (a < 0.0)) out[0] = out[1] = out[2] = a;
    out[3] = a;
}

// the union: per channel the smaller value (a compare, not fmin: which zero survives must not depend on the library)
HIT_HD void msdf_union(double* best, const double* v) {
    for (int c = 0; c < 4; ++c) best[c] = v[c] < best[c] ? v[c] : best[c];
}

// The four values of one point against groups of paths (group g: the paths group_off[g] .. group_off[g + 1]; path p: the edges
// off[p] .. off[p + 1], 4 doubles each, colour[p], rule[p]), without any cull: what a lane of k_msdf_distance computes.
HIT_HD void msdf_point(const double* edges, const int32_t* off, const uint8_t* rule, const uint8_t* colour, const int32_t* group_off,
                       const int8_t* orient, long long n_groups, double spread, double pa, double pb, double* out) {
    const bool finite = hit_finite(pa, pb);
    if (!finite) pa = pb = NAN;
    double best[4] = {spread, spread, spread, spread};
    for (long long g = 0; g < n_groups; ++g) {
        if (group_off[g + 1] <= group_off[g]) continue;
        MsdfState s;
        msdf_begin(s);
        for (int p = group_off[g]; p < group_off[g + 1]; ++p)
            for (int e = off[p]; e < off[p + 1]; ++e) {
                double q[MSDF_EDGE_DOUBLES];
                msdf_edge_prepare(edges[4 * (long long)e], edges[4 * (long long)e + 1], edges[4 * (long long)e + 2], edges[4 * (long long)e + 3], q);
                msdf_edge(s, colour[p], q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], pa, pb);
            }
        double v[4];
        msdf_finish(s, rule[group_off[g]] & 1, orient[g], spread, finite, v);
        msdf_union(best, v);
    }
    for (int c = 0; c < 4; ++c) out[c] = best[c];
}
