// svgr_gradpaint.h -- per-pixel arithmetic of gradient paints in differentiable compositing: the renderer's linear and one-circle
// radial gradient evaluated at a pixel centre (forward), and the derivative of the painted pixel with respect to the paint
// multiplier, the "pixel centre -> gradient space" transform, the gradient's geometry, the stop positions and the stop colours.
//
// Plain double arithmetic for the host (tests/gradpaint_harness.cpp) and the device (k_compose_over_painted,
// k_compose_vjp_painted of svgr_hip.hip), both compiled with -ffp-contract=off.  The only fused multiply-adds are the ones the
// renderer has: the two of xform_point and the one of the linear offset.  Every other product and sum is rounded on its own, in
// the order written.  The forward restates grad_point / grad_colour_user of svgr_hip.hip operation for operation (kinds 1 and 2,
// stops in memory); DESIGN.md 7y has the derivation, tests/gradpaint_ref.py restates all of it in numpy.
//
//   point     px = (double)i + ((double)row0 + 0.5), py = (double)j + ((double)col0 + 0.5), (x, y) = xform_point(m6, px, py)
//   offset    linear  v = p1 - p0, vv = v0 v0 + v1 v1, dx = x - p0x, dy = y - p0y, t = fma(dx, v0, dy v1) / vv
//             radial  o0 = (x - cx) / r, o1 = (y - cy) / r, t = sqrt(o0 o0 + o1 o1)
//   spread    pad u = t;  repeat u = isinf(t) ? copysign(0, t) : t - trunc(t);  reflect a = t + 1, b = a - 2 floor(a 0.5), u = |b - 1|
//   stops     u <= o_0: c_0;  u > o_{n-1}: c_{n-1};  o_s < u <= o_{s+1}: ratio = (u - o_s) / (o_{s+1} - o_s),
//             col_k = 0 + ((1 - ratio) c_{s,k} + ratio c_{s+1,k}).  At most one test holds for non-decreasing positions; none for NaN.
//   paint     s_k = (col_k m) paint_k, then over_px: the tile kernel's order.  Walk 1 lets 1 - s_3 through.
//   backward  P_k = col_k paint_k is the effective paint of compose_vjp_step, whose t_k are the pixel's terms of d / d P_k:
//               d / d paint_k = t_k col_k;  q_k = t_k paint_k
//               clamp or n = 1:  d / d c_s[k] = q_k, nothing else
//               segment:  w0 = 1 - ratio;  d / d c_s[k] = q_k w0;  d / d c_{s+1}[k] = q_k ratio
//                         D = ((q_0 e_0 + q_1 e_1) + q_2 e_2) + q_3 e_3 with e_k = c_{s+1,k} - c_{s,k};  E = D / (o_{s+1} - o_s)
//                         d / d o_s = -(w0 E);  d / d o_{s+1} = -(ratio E);  a = sigma E is d / d t
//               linear:   gx = a (v0 / vv), gy = a (v1 / vv);  d / d p1 = a ((dx - (2 t) v0) / vv), a ((dy - (2 t) v1) / vv);
//                         d / d p0 = -(gx + d / d p1x), -(gy + d / d p1y)            (t the offset BEFORE the spread)
//               radial:   rt = r t;  gx = a (o0 / rt), gy = a (o1 / rt);  d / d c = -gx, -gy;  d / d r = -(a (t / r))
//               m6:       gx px, gx py, gx, gy px, gy py, gy
//   one side  where the derivative is not defined the tests above choose: u on a stop or a clamp belongs to the segment or clamp
//             that `<=` selects; an empty segment (two equal positions) is never selected, so nothing is divided by 0; the repeat
//             wrap has slope +1 on both sides; the reflect fold has sigma = +1 where b - 1 >= 0, else -1; a radial pixel with
//             t == 0 has no geometry and m6 terms; NaN selects no stop: colour and terms are 0.
#pragma once
#include "svgr_core.h"
#include "svgr_compose.h"

namespace svgr {

constexpr int GRADPAINT_MAX_STOPS = 32;   // the batch's GRAD_MAX_STOPS
constexpr int GRADPAINT_DENSE = 14;       // per path: 4 paint + 6 m6 + 4 geometry terms
constexpr int GRADPAINT_STOP = 5;         // per stop: position + 4 colour channels

// what the forward of one pixel of one gradient path leaves for its backward
struct GradPaintPx {
    double px, py;      // the pixel centre
    double t;           // the offset before the spread
    double sigma;       // the spread's slope
    double a0, a1;      // linear: dx, dy; radial: o0, o1
    double ratio;
    int lo, hi;         // the stops used: lo == hi at a clamp, lo + 1 == hi in a segment, -1 where none is (NaN)
};

// the colour of a gradient at pixel (i, j): kind 1 / 2, geom = {p0x, p0y, p1x, p1y} / {cx, cy, r, -}
SVGR_HD void gradpaint_colour(int kind, int spread, const double* m6, const double* geom, int n, const double* pos, const double* rgba,
                              long long i, long long j, long long row0, long long col0, double* col, GradPaintPx& e) {
    e.px = (double)i + ((double)row0 + 0.5);
    e.py = (double)j + ((double)col0 + 0.5);
    double x, y;
    xform_point(m6, e.px, e.py, x, y);
    double t;
    if (kind == 1) {
        const double v0 = geom[2] - geom[0], v1 = geom[3] - geom[1];
        const double vv = v0 * v0 + v1 * v1;
        e.a0 = x - geom[0];
        e.a1 = y - geom[1];
        t = fma(e.a0, v0, e.a1 * v1) / vv;
    } else {
        e.a0 = (x - geom[0]) / geom[2];
        e.a1 = (y - geom[1]) / geom[2];
        t = sqrt(e.a0 * e.a0 + e.a1 * e.a1);
    }
    e.t = t;
    e.sigma = 1.0;
    double u = t;
    if (spread == 1) {
        u = isinf(t) ? copysign(0.0, t) : t - trunc(t);
    } else if (spread == 2) {
        const double a = t + 1.0;
        const double b = (a - 2.0 * floor(a * 0.5)) - 1.0;
        e.sigma = b >= 0.0 ? 1.0 : -1.0;
        u = fabs(b);
    }
    col[0] = col[1] = col[2] = col[3] = 0.0;
    e.lo = e.hi = -1;
    e.ratio = 0.0;
    if (u <= pos[0]) {
        e.lo = e.hi = 0;
        for (int k = 0; k < 4; ++k) col[k] = rgba[k];
    }
    if (u > pos[n - 1]) {
        e.lo = e.hi = n - 1;
        for (int k = 0; k < 4; ++k) col[k] = rgba[4 * (n - 1) + k];
    }
    for (int s = 0; s + 1 < n; ++s) {
        const double o0 = pos[s], o1 = pos[s + 1];
        if (u > o0 && u <= o1) {
            const double ratio = (u - o0) / (o1 - o0);
            for (int k = 0; k < 4; ++k) col[k] = col[k] + ((1 - ratio) * rgba[4 * s + k] + ratio * rgba[4 * s + 4 + k]);
            e.lo = s;
            e.hi = s + 1;
            e.ratio = ratio;
        }
    }
}

// the painting step of a gradient path: s_k = (col_k m) paint_k source-over the canvas; returns s_3
SVGR_HD double gradpaint_step(double* C, double m, const double* col, const double* paint) {
    const double s0 = (col[0] * m) * paint[0], s1 = (col[1] * m) * paint[1], s2 = (col[2] * m) * paint[2], s3 = (col[3] * m) * paint[3];
    over_px(C, s0, s1, s2, s3);
    return s3;
}

// walk 1: what a gradient path lets through, 1 - s_3 with the forward's s_3
SVGR_HD double gradpaint_through(double m, const double* col, const double* paint) { return 1.0 - (col[3] * m) * paint[3]; }

// the effective paint of compose_vjp_step
SVGR_HD void gradpaint_effective(const double* col, const double* paint, double* P) {
    P[0] = col[0] * paint[0];
    P[1] = col[1] * paint[1];
    P[2] = col[2] * paint[2];
    P[3] = col[3] * paint[3];
}

// walk 2 at a gradient path of one pixel, after compose_vjp_step: t[0..3] its terms of d / d P.  dense[0..13] are the pixel's terms
// of d / d (paint, m6, geom); lo[0..4] and hi[0..4] those of (position, colour) of stops e.lo and e.hi (hi is used only in a segment).
SVGR_HD void gradpaint_vjp(int kind, const double* geom, const double* pos, const double* rgba, const double* col, const double* paint,
                           const GradPaintPx& e, const double* t, double* dense, double* lo, double* hi) {
    double q[4];
    for (int k = 0; k < 4; ++k) {
        dense[k] = t[k] * col[k];
        q[k] = t[k] * paint[k];
    }
    for (int k = 4; k < GRADPAINT_DENSE; ++k) dense[k] = 0.0;
    for (int k = 0; k < GRADPAINT_STOP; ++k) lo[k] = hi[k] = 0.0;
    if (e.lo < 0) return;
    if (e.lo == e.hi) {
        for (int k = 0; k < 4; ++k) lo[1 + k] = q[k];
        return;
    }
    const double* c0 = rgba + 4 * e.lo;
    const double* c1 = rgba + 4 * e.hi;
    const double w0 = 1 - e.ratio;
    for (int k = 0; k < 4; ++k) {
        lo[1 + k] = q[k] * w0;
        hi[1 + k] = q[k] * e.ratio;
    }
    const double D = ((q[0] * (c1[0] - c0[0]) + q[1] * (c1[1] - c0[1])) + q[2] * (c1[2] - c0[2])) + q[3] * (c1[3] - c0[3]);
    const double E = D / (pos[e.hi] - pos[e.lo]);
    lo[0] = -(w0 * E);
    hi[0] = -(e.ratio * E);
    const double a = e.sigma * E;
    double gx, gy;
    if (kind == 1) {
        const double v0 = geom[2] - geom[0], v1 = geom[3] - geom[1];
        const double vv = v0 * v0 + v1 * v1;
        const double t2 = 2.0 * e.t;
        gx = a * (v0 / vv);
        gy = a * (v1 / vv);
        dense[12] = a * ((e.a0 - t2 * v0) / vv);
        dense[13] = a * ((e.a1 - t2 * v1) / vv);
        dense[10] = -(gx + dense[12]);
        dense[11] = -(gy + dense[13]);
    } else {
        if (e.t == 0.0) return;
        const double rt = geom[2] * e.t;
        gx = a * (e.a0 / rt);
        gy = a * (e.a1 / rt);
        dense[10] = -gx;
        dense[11] = -gy;
        dense[12] = -(a * (e.t / geom[2]));
    }
    dense[4] = gx * e.px;
    dense[5] = gx * e.py;
    dense[6] = gx;
    dense[7] = gy * e.px;
    dense[8] = gy * e.py;
    dense[9] = gy;
}

}  // namespace svgr
