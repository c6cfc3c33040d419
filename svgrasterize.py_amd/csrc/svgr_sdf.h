// svgr_sdf.h -- per-lane arithmetic of signed distance fields: how far a point is from a path's outline, with the sign of
// svgr_hit.h's inside predicate, clamped to a spread and encoded for a texture.
//
// Everything here is plain double arithmetic, compilable for the host (the CPU harness of tests/sdf_harness.cpp) and for the device
// (k_sdf_distance of svgr_hip.hip).  Both sides are compiled with -ffp-contract=off and nothing below is a fused multiply-add:
// every product and every sum is rounded on its own.  DESIGN.md 7r has the definitions; tests/sdf_ref.py restates them in numpy.
//
//   edge      (a0, b0) -> (a1, b1) and a point (pa, pb), in the coordinate order of svgr_batch_all_edges, as in svgr_hit.h
//   prepared  per EDGE, once, not per (point, edge) pair:
//               x = a1 - a0;  y = b1 - b0;  len2 = x*x + y*y;  inv = len2 > 0 ? 1.0 / len2 : 0.0
//   d2        for a FINITE point:
//               da = pa - a0;  db = pb - b0
//               t  = clamp((da*x + db*y) * inv, 0, 1)
//               qa = a0 + t*x;  qb = b0 + t*y
//               d2 = (pa - qa)*(pa - qa) + (pb - qb)*(pb - qb)
//             An edge of length zero has inv = 0, so t = 0 and d2 is the squared distance to its point.
//   term      the winding term of svgr_hit.h from the same x, y, da, db: x * db and da * y are hit_edge_term's two products, bit
//             for bit (a1 - a0 and b1 - b0 are rounded the same way wherever they are computed).
//   path      unsigned distance = sqrt(min over the edges of d2): fmin over the same set of values does not depend on its order.
//             A path without edges is +inf away.  A point with a NaN or infinite coordinate is +inf away from everything and
//             outside, as in svgr_hit.h.  Signed: NEGATIVE inside (hit_inside of the winding number under the path's rule),
//             positive outside.
//   spread    +inf, or finite and > 0:  d = min(max(d, -spread), spread)
//   encoding  F64  the clamped distance
//             F32  (float)(0.5 - d / (2*spread)): in [0, 1], 0.5 on the outline, larger inside (the convention of SDF text shaders)
//             U8   the double 0.5 - d / (2*spread) through the uint8 rounding of svgr_tensor.h: rint(v * 255), saturated
//             F32 and U8 need a finite spread.
//   union     the minimum over the paths of their signed clamped distances.  That is exact outside every path, and its sign is
//             exact everywhere (negative where some path holds the point).  INSIDE overlapping paths it is the depth in the
//             deepest single path, not the distance to the outline of the union (which may be farther).
#pragma once
#include <cmath>
#include <cstdint>

#include "svgr_hit.h"
#include "svgr_tensor.h"

constexpr int SDF_F64 = 0, SDF_F32 = 1, SDF_U8 = 2, SDF_ENCODINGS = 3;
constexpr int SDF_EDGE_DOUBLES = 6;   // a staged edge: a0, b0, x, y, inv, b1

HIT_HD int sdf_elem_bytes(int enc) { return enc == SDF_F64 ? 8 : enc == SDF_F32 ? 4 : 1; }

// an edge as the inner loop wants it: out[0 .. 6) = a0, b0, x, y, inv, b1
HIT_HD void sdf_edge_prepare(double a0, double b0, double a1, double b1, double* out) {
    const double x = a1 - a0, y = b1 - b0;
    const double xx = x * x, yy = y * y;
    const double len2 = xx + yy;
    out[0] = a0; out[1] = b0; out[2] = x; out[3] = y;
    out[4] = len2 > 0.0 ? 1.0 / len2 : 0.0;
    out[5] = b1;
}

// squared distance of a FINITE point to a prepared edge; da = pa - a0, db = pb - b0
HIT_HD double sdf_edge_d2(double a0, double b0, double x, double y, double inv, double pa, double pb, double da, double db) {
    const double m0 = da * x, m1 = db * y;
    const double s = m0 + m1;
    double t = s * inv;
    t = t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t;
    const double tx = t * x, ty = t * y;
    const double qa = a0 + tx, qb = b0 + ty;
    const double ea = pa - qa, eb = pb - qb;
    const double ea2 = ea * ea, eb2 = eb * eb;
    return ea2 + eb2;
}

// hit_edge_term from the shared differences: x * db is its (a1 - a0) * (pb - b0), da * y its (pa - a0) * (b1 - b0)
HIT_HD int sdf_edge_term(double b0, double b1, double x, double y, double pb, double da, double db) {
    const bool up = (b0 <= pb) && (b1 > pb), down = (b1 <= pb) && (b0 > pb);
    const double m0 = x * db, m1 = da * y;
    const double d = m0 - m1;
    return (up && d > 0.0) ? 1 : (down && d < 0.0) ? -1 : 0;
}

HIT_HD double sdf_clamp(double d, double spread) {
    d = d < -spread ? -spread : d;
    return d > spread ? spread : d;
}

// min d2 and winding number -> the clamped, optionally signed distance
HIT_HD double sdf_finish(double min_d2, int w, int evenodd, int is_signed, double spread) {
    double d = sqrt(min_d2);
    if (is_signed && hit_inside(w, evenodd)) d = -d;
    return sdf_clamp(d, spread);
}

// the clamped distance of one point to one path: `n` edges of 4 doubles each
HIT_HD double sdf_path_distance(const double* edges, long long n, int evenodd, int is_signed, double spread, double pa, double pb) {
    double m = INFINITY;
    int w = 0;
    if (hit_finite(pa, pb))
        for (long long e = 0; e < n; ++e) {
            double q[SDF_EDGE_DOUBLES];
            sdf_edge_prepare(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], q);
            const double da = pa - q[0], db = pb - q[1];
            m = fmin(m, sdf_edge_d2(q[0], q[1], q[2], q[3], q[4], pa, pb, da, db));
            w += sdf_edge_term(q[1], q[5], q[2], q[3], pb, da, db);
        }
    return sdf_finish(m, w, evenodd, is_signed, spread);
}

// The distance kernels' cull: may the path (or group of paths) with the extent ext[0 .. 4) = min a, min b, max a, max b be left
// out for EVERY point of `box`?  Never for cull_spread = +inf.  Else it is out of reach when the extent lies farther than
//     thr = cull_spread * (1 + 2^-40) + 2^-40 * (the largest magnitude among the extent's four numbers)
// from the box in a or in b.  DESIGN.md 7r shows that sdf_path_distance then gives every point of the box exactly +spread (a
// distance that clamps, and winding 0), so a caller that counts the path as +spread instead cannot be told from one that walks
// it; tests/test_sdf_host.py holds both the predicate and that claim.  The side on which the points' rays run THROUGH the path
// (the path wholly at larger a) is taken only when no point of the box has |pb| < 2^-400: the argument needs the winding term's
// products clear of underflow there.  An empty box (no finite point) is out of reach of everything.
HIT_HD bool sdf_out_of_reach(const double* ext, const HitBox& box, double cull_spread) {
    if (!(cull_spread < INFINITY)) return false;
    const double mna = ext[0], mnb = ext[1], mxa = ext[2], mxb = ext[3];
    const double big = fmax(fmax(fabs(mna), fabs(mxa)), fmax(fabs(mnb), fabs(mxb)));
    const double thr = cull_spread * (1.0 + 0x1p-40) + 0x1p-40 * big;
    return mnb - box.hi_b > thr || box.lo_b - mxb > thr || box.lo_a - mxa > thr || (box.min_absb >= 0x1p-400 && mna - box.hi_a > thr);
}

// 0.5 - d / (2*spread) of a clamped distance (finite spread): in [0, 1]
HIT_HD double sdf_unit(double d, double spread) {
    const double two = 2.0 * spread;
    const double r = d / two;
    return 0.5 - r;
}
HIT_HD float sdf_encode_f32(double d, double spread) { return (float)sdf_unit(d, spread); }
HIT_HD uint8_t sdf_encode_u8(double d, double spread) { return (uint8_t)tensor_encode(TENSOR_U8, sdf_unit(d, spread)); }
