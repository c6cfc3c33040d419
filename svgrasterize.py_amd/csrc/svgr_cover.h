// svgr_cover.h -- per-lane arithmetic of differentiable coverage: a path's exact area coverage over a viewport together with
// the derivative of its fill rule (forward), and the derivative of sum(grad_out * cover) with respect to the path's control
// points and its transform (backward).
//
// Everything here is plain double arithmetic, compilable for the host (the CPU harness of tests/cover_harness.cpp) and for the
// device (k_cover_accumulate, k_cover_resolve, k_cover_vjp of svgr_hip.hip).  Both sides are compiled with -ffp-contract=off and
// nothing below is a fused multiply-add: every product and every sum is rounded on its own (the transform and the subdivision
// are svgr_core.h's, as the renderer evaluates them).  DESIGN.md 7w has the derivation; tests/cover_ref.py restates it in numpy.
//
//   plane     rows x cols pixels; a point is (row, col) in the viewport's own coordinates: presentation space minus (row0, col0)
//   edges     the control points go through xform_point; a cubic is subdivided in presentation space by cubic_flatness /
//             cubic_left_inplace / cubic_right_inplace against thr, in flatten_subtree's order and with its roundings, so the
//             edge set is the renderer's.  The piece at (level, idx) spans t0 = idx / 2^level .. t1 = (idx + 1) / 2^level of its
//             cubic; a line is its own edge with t0 = 0, t1 = 1.  The origin is subtracted from the END POINTS of an edge.
//   forward   A = the row-wise running sum of the row_step / row_record pieces of every edge (line_signed_coverage: left of the
//             plane a piece folds into column 0, right of it it is dropped); cover = fill_rule(A); slope = d fill_rule / dA:
//               nonzero   m = |A|:  0 if m < kZeroCut or m >= 1, else sign(A)
//               even-odd  r = (A + 1) - 2 floor((A + 1) / 2) - 1:  0 if |r| < kZeroCut, else sign(r)
//   backward  W = grad_out * slope per pixel.  An edge p0 -> p1, e = p1 - p0, restricted to the t inside [0, rows] x [0, cols], is
//             cut at every crossing of an integer row or column; the piece [ta, tb] belongs to the pixel floor() of its midpoint
//             (pieces outside the plane count nothing):
//               I0 = sum W ((tb - ta) - (tb^2 - ta^2) / 2)      I1 = sum W (tb^2 - ta^2) / 2
//             evaluated as W (tb - ta) (1 - tm) and W (tb - ta) tm with tm = (ta + tb) / 2: the same numbers without the
//             cancellation that the first form suffers near t = 1
//               g(p0) = (e_col I0, -e_row I0)                   g(p1) = (e_col I1, -e_row I1)         as (row, col)
//             a cubic's transformed control point k: g(c'_k) = sum over its pieces of B_k(t0) g(p0) + B_k(t1) g(p1)
//             user space: g(c_k) = (m00 g_r + m10 g_c, m01 g_r + m11 g_c)
//             transform:  (sum g_r x, sum g_r y, sum g_r, sum g_c x, sum g_c y, sum g_c) in point order
//   refused   a transformed control point that is not finite or beyond +-1e9, and a row of an edge whose columns leave +-1e9:
//             status bit 1, the segment (the row) contributes nothing.  Status bit 0: the subdivision reached its depth cap.
#pragma once
#include <math.h>
#include <stdint.h>

#include "svgr_core.h"

namespace svgr {

constexpr int COVER_F64 = 0, COVER_F32 = 1, COVER_PLANES = 2;
constexpr int kCoverDepthBit = 1, kCoverRangeBit = 2;
constexpr double kCoverLimit = 1.0e9;

SVGR_HD int cover_plane_bytes(int plane) { return plane == COVER_F64 ? 8 : 4; }

// d fill_rule(A) / dA: -1, 0 or +1
SVGR_HD int cover_slope(double A, int rule) {
    if (!rule) {
        const double m = fabs(A);
        if (m < kZeroCut || m >= 1.0) return 0;
        return A > 0.0 ? 1 : -1;
    }
    const double a = A + 1.0;
    const double f = 2.0 * floor(a * 0.5);
    const double r = (a - f) - 1.0;
    if (fabs(r) < kZeroCut) return 0;
    return r > 0.0 ? 1 : -1;
}

// W of one pixel: where the slope is 0 the gradient is not looked at (a NaN there stays out of the sums)
SVGR_HD double cover_weight(double grad, int slope) { return slope ? grad * (double)slope : 0.0; }

// the transformed control points of one segment (presentation space); false: one is not finite or beyond the limit
SVGR_HD bool cover_seg_points(const double* pts, int npts, const double* m6, double* c) {
    bool ok = true;
    for (int k = 0; k < npts; ++k) {
        xform_point(m6, pts[2 * k], pts[2 * k + 1], c[2 * k], c[2 * k + 1]);
        ok = ok && fabs(c[2 * k]) <= kCoverLimit && fabs(c[2 * k + 1]) <= kCoverLimit;   // (false for a NaN)
    }
    return ok;
}

// flatten_subtree's walk with the position of every piece: piece(cur, level, idx) once per flat piece in curve order, `cur` the
// piece's control points.  The same calls in the same order as flatten_subtree, so the pieces are its pieces to the bit.
template <class Piece>
SVGR_HD int cover_flatten(const double* root, double thr, Piece&& piece, bool& overflow) {
    double cur[8];
    for (int i = 0; i < 8; ++i) cur[i] = root[i];
    int level = 0, n = 0;
    unsigned long long idx = 0;
    for (;;) {
        bool flat = cubic_flatness(cur) < thr;
        if (!flat && level >= kMaxFlattenDepth) { flat = true; overflow = true; }
        if (flat) {
            piece(cur, level, idx);
            ++n;
            while (level > 0 && (idx & 1ull)) { idx >>= 1; --level; }
            if (level == 0) break;
            idx |= 1ull;
            for (int i = 0; i < 8; ++i) cur[i] = root[i];
            for (int l = level - 1; l >= 0; --l) {
                if ((idx >> l) & 1ull) cubic_right_inplace(cur); else cubic_left_inplace(cur);
            }
        } else {
            cubic_left_inplace(cur);
            ++level;
            idx <<= 1;
        }
    }
    return n;
}

// The edges of one segment in the viewport's coordinates: edge(p0r, p0c, p1r, p1c, t0, t1) per edge in curve order.  `c`: the
// segment's points in presentation space (cover_seg_points).
template <class Edge>
SVGR_HD void cover_seg_edges(const double* c, int is_cubic, double thr, double or0, double oc0, Edge&& edge, bool& overflow) {
    if (!is_cubic) {
        edge(c[0] - or0, c[1] - oc0, c[2] - or0, c[3] - oc0, 0.0, 1.0);
        return;
    }
    cover_flatten(c, thr, [&](const double* q, int level, unsigned long long idx) {
        const double scale = ldexp(1.0, -level);
        edge(q[0] - or0, q[1] - oc0, q[6] - or0, q[7] - oc0, (double)idx * scale, (double)(idx + 1ull) * scale);
    }, overflow);
}

// The pieces of one recorded row, as line_signed_coverage stores them into a row of `cols` pixels: put(col, v).  A run of equal
// pieces left of the plane goes into column 0 as ONE product (count * value) instead of count additions.
template <class Put>
SVGR_HD void cover_row_add(const RowPieces& r, int cols, Put&& put) {
    const int x0i = r.x0i, n = r.n;
    if (x0i >= cols) return;
    put(x0i > 0 ? x0i : 0, r.v[0]);
    if (x0i + 1 >= cols) return;
    put(x0i + 1 > 0 ? x0i + 1 : 0, r.v[1]);
    if (n >= 3) {
        const int lo = x0i + 2, hi = x0i + n - 1;   // the run [lo, hi)
        if (lo < 1) {
            const int k = (hi < 1 ? hi : 1) - lo;
            if (k > 0) put(0, (double)k * r.v[2]);
        }
        const int stop = hi < cols ? hi : cols;
        for (int xi = lo > 1 ? lo : 1; xi < stop; ++xi) put(xi, r.v[2]);
        if (hi >= cols) return;
        put(hi > 0 ? hi : 0, r.v[3]);
    }
    if (n >= 2) {
        const int xi = x0i + n;
        if (xi >= cols) return;
        put(xi > 0 ? xi : 0, r.v[4]);
    }
}

// One edge into the accumulation plane: add(row, col, v).  false: a row's columns left +-kCoverLimit (nothing of it is added).
template <class Add>
SVGR_HD bool cover_edge_accumulate(double ar, double ac, double br, double bc, int rows, int cols, Add&& add) {
    const EdgeSetup e = edge_setup(ar, ac, br, bc, rows);
    if (!e.valid) return true;
    bool ok = true;
    RowState s;
    s.x_next = e.x;
    s.x = s.d = 0.0;
    for (int y = e.y_begin; y < e.y_end; ++y) {
        row_step(s, y, e.p0y, e.p1y, e.dxdy, e.dir);
        if (!(fabs(s.x) < kCoverLimit && fabs(s.x_next) < kCoverLimit)) {
            ok = false;
            continue;
        }
        const RowPieces r = row_record(s.x, s.x_next, s.d);
        cover_row_add(r, cols, [&](int col, double v) { add(y, col, v); });
    }
    return ok;
}

// the cubic Bernstein weights at t
SVGR_HD void cover_bernstein(double t, double* B) {
    const double u = 1.0 - t;
    const double uu = u * u, tt = t * t;
    B[0] = uu * u;
    B[1] = 3.0 * (t * uu);
    B[2] = 3.0 * (tt * u);
    B[3] = tt * t;
}

// [tlo, thi] cut to the t at which p + t e lies in [0, limit]; false: none does
SVGR_HD bool cover_clip_axis(double p, double e, double limit, double& tlo, double& thi) {
    if (e == 0.0) return p >= 0.0 && p <= limit;
    double ta = (0.0 - p) / e, tb = (limit - p) / e;
    if (ta > tb) { const double t = ta; ta = tb; tb = t; }
    tlo = ta > tlo ? ta : tlo;
    thi = tb < thi ? tb : thi;
    return tlo < thi;
}

// The clipped walk of one edge over W: weight(row, col) is asked once per piece inside the plane.
template <class Weight>
SVGR_HD void cover_edge_walk(double p0r, double p0c, double p1r, double p1c, int rows, int cols, Weight&& weight, double& I0, double& I1) {
    I0 = 0.0;
    I1 = 0.0;
    const double er = p1r - p0r, ec = p1c - p0c;
    double tlo = 0.0, thi = 1.0;
    if (!cover_clip_axis(p0r, er, (double)rows, tlo, thi)) return;
    if (!cover_clip_axis(p0c, ec, (double)cols, tlo, thi)) return;
    const double sr = p0r + er * tlo, sc = p0c + ec * tlo;
    // the next integer row / column ahead of the start, and the step to the one after
    double kr = er > 0.0 ? floor(sr) + 1.0 : ceil(sr) - 1.0, kc = ec > 0.0 ? floor(sc) + 1.0 : ceil(sc) - 1.0;
    const double dr = er > 0.0 ? 1.0 : -1.0, dc = ec > 0.0 ? 1.0 : -1.0;
    double t = tlo;
    const int cap = rows + cols + 4;
    for (int it = 0; it < cap; ++it) {
        const double tr = er != 0.0 ? (kr - p0r) / er : INFINITY;
        const double tc = ec != 0.0 ? (kc - p0c) / ec : INFINITY;
        double tn;
        if (tr <= tc) { tn = tr; kr += dr; } else { tn = tc; kc += dc; }
        const bool last = !(tn < thi);
        if (last) tn = thi;
        if (tn > t) {
            const double tm = 0.5 * (t + tn);
            const double mr = floor(p0r + er * tm), mc = floor(p0c + ec * tm);
            if (mr >= 0.0 && mr < (double)rows && mc >= 0.0 && mc < (double)cols) {
                const double w = weight((int)mr, (int)mc);
                // (tb - ta) - (tb^2 - ta^2) / 2 = (tb - ta) (1 - tm) and (tb^2 - ta^2) / 2 = (tb - ta) tm: as products, so that an
                // edge whose FIRST point is far away (t near 1 in the plane) does not lose its weight to cancellation
                const double dt = tn - t;
                const double u = 1.0 - tm;
                I0 = I0 + w * (dt * u);
                I1 = I1 + w * (dt * tm);
            }
            t = tn;
        }
        if (last) break;
    }
}

// The backward pass of one segment: gseg[0 .. 8) = the derivative with respect to its points in user space (a line's last two
// points stay 0), gm6[0 .. 6) = its part of the transform's.  pts: its 4 x 2 user-space doubles.  Returns status bits.
template <class Weight>
SVGR_HD int cover_seg_vjp(const double* pts, int is_cubic, const double* m6, double or0, double oc0, int rows, int cols, double thr,
                          Weight&& weight, double* gseg, double* gm6) {
    for (int i = 0; i < 8; ++i) gseg[i] = 0.0;
    for (int i = 0; i < 6; ++i) gm6[i] = 0.0;
    const int npts = is_cubic ? 4 : 2;
    double c[8];
    if (!cover_seg_points(pts, npts, m6, c)) return kCoverRangeBit;
    double g[8];   // with respect to the transformed points, (row, col) each
    for (int i = 0; i < 8; ++i) g[i] = 0.0;
    bool overflow = false;
    cover_seg_edges(c, is_cubic, thr, or0, oc0, [&](double p0r, double p0c, double p1r, double p1c, double t0, double t1) {
        double I0, I1;
        cover_edge_walk(p0r, p0c, p1r, p1c, rows, cols, weight, I0, I1);
        const double er = p1r - p0r, ec = p1c - p0c;
        const double g0r = ec * I0, g0c = -er * I0, g1r = ec * I1, g1c = -er * I1;
        if (!is_cubic) {
            g[0] = g0r; g[1] = g0c; g[2] = g1r; g[3] = g1c;
            return;
        }
        double B0[4], B1[4];
        cover_bernstein(t0, B0);
        cover_bernstein(t1, B1);
        for (int k = 0; k < 4; ++k) {
            g[2 * k] = g[2 * k] + (B0[k] * g0r + B1[k] * g1r);
            g[2 * k + 1] = g[2 * k + 1] + (B0[k] * g0c + B1[k] * g1c);
        }
    }, overflow);
    for (int k = 0; k < npts; ++k) {
        const double gr = g[2 * k], gc = g[2 * k + 1], x = pts[2 * k], y = pts[2 * k + 1];
        gseg[2 * k] = m6[0] * gr + m6[3] * gc;
        gseg[2 * k + 1] = m6[1] * gr + m6[4] * gc;
        gm6[0] = gm6[0] + gr * x; gm6[1] = gm6[1] + gr * y; gm6[2] = gm6[2] + gr;
        gm6[3] = gm6[3] + gc * x; gm6[4] = gm6[4] + gc * y; gm6[5] = gm6[5] + gc;
    }
    return overflow ? kCoverDepthBit : 0;
}

// The forward pass of one segment: add(row, col, v) for every piece of its edges.  Returns status bits.
template <class Add>
SVGR_HD int cover_seg_accumulate(const double* pts, int is_cubic, const double* m6, double or0, double oc0, int rows, int cols, double thr,
                                 Add&& add) {
    double c[8];
    if (!cover_seg_points(pts, is_cubic ? 4 : 2, m6, c)) return kCoverRangeBit;
    bool overflow = false, in_range = true;
    cover_seg_edges(c, is_cubic, thr, or0, oc0, [&](double p0r, double p0c, double p1r, double p1c, double, double) {
        in_range = cover_edge_accumulate(p0r, p0c, p1r, p1c, rows, cols, add) && in_range;
    }, overflow);
    return (overflow ? kCoverDepthBit : 0) | (in_range ? 0 : kCoverRangeBit);
}

}  // namespace svgr
