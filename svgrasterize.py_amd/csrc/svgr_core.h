// svgr_core.h -- per-lane arithmetic of the hot path, shared by every HIP kernel.
//
// Everything here is straight-line double arithmetic written so that one lane reproduces
// what the reference evaluates for one element (S:n = svgrasterize.py line n of the reference):
//   xform_point      Transform.__call__            S:531-534
//   cubic_flatness   bezier3_flatness_batch        S:2071-2088
//   cubic_split      bezier3_split_batch           S:2066-2068
//   flatten_cubic    bezier3_flatten_batch         S:2091-2098 (depth-first instead of level-synchronous:
//                                                   same edge SET, curve order instead of level order)
//   EdgeWalk         line_signed_coverage          S:2213-2304 (row recurrence + per-row area pieces)
//   fill_rule_*      Path.mask                     S:984-990
//   over_px          canvas_compose(OVER)          S:286
// The functions are SVGR_HD so the same code can be compiled for the host by the unit-test
// harness (tests/host_harness.cpp); the product only ever runs them inside HIP kernels.
// Compile with -ffp-contract=off: the reference rounds every operation separately except
// where an explicit fma() below mirrors what BLAS evaluates for np.dot / @.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVGR_HD __host__ __device__ __forceinline__
#define SVGR_UNROLL _Pragma("unroll")
#else
#define SVGR_HD static inline
#define SVGR_UNROLL
#endif

namespace svgr {

constexpr int kMaxFlattenDepth = 40;   // reference has no cap; finite input never gets close
constexpr double kZeroCut = 1e-6;      // S:990

// ------------------------------------------------------------------------------------
// affine transform of one point: out_r = fma(p1, m_r1, p0*m_r0) + b_r     (dgemm form)
// m6 = {m00, m01, m02, m10, m11, m12}
// ------------------------------------------------------------------------------------
SVGR_HD void xform_point(const double* m6, double p0, double p1, double& o0, double& o1) {
    o0 = fma(p1, m6[1], p0 * m6[0]) + m6[2];
    o1 = fma(p1, m6[4], p0 * m6[3]) + m6[5];
}

// strided-ddot form of np.dot(W(k,4), batch(N,4,2)): fma(w0,x0, w2*x2) + fma(w1,x1, w3*x3)
SVGR_HD double dot4(double w0, double w1, double w2, double w3, double x0, double x1, double x2, double x3) {
    return fma(w0, x0, w2 * x2) + fma(w1, x1, w3 * x3);
}

// The weight rows used below contain zeros and ones.  With w == 0 the term fma(0, x, t) is t and 0 * x is +0, with
// w == 1 fma(1, x, t) is x + t: for finite x the shortened forms give the same bits as the full dot4 (up to the sign
// of a zero, which nothing downstream can see), at about half the instructions -- the compiler may not drop them
// itself (0 * x is not 0 for a NaN or an infinity).

// c = 4 points (row, col) interleaved: c[2*k + axis]
SVGR_HD double cubic_flatness(const double* c) {
    // u = -2 b0 + 3 b1 - b3 ; v = -b0 + 3 b2 - 2 b3 ; f = max(ux^2, uy^2) + max(vx^2, vy^2)
    // dot4(-2, 3, 0, -1, x) = fma(-2, x0, 0 * x2) + fma(3, x1, -1 * x3) = -2 x0 + fma(3, x1, -x3)
    // dot4(-1, 0, 3, -2, x) = fma(-1, x0, 3 * x2) + fma(0, x1, -2 * x3) = fma(-1, x0, 3 x2) + -2 x3
    double ux = -2.0 * c[0] + fma(3.0, c[2], -c[6]);
    double uy = -2.0 * c[1] + fma(3.0, c[3], -c[7]);
    double vx = fma(-1.0, c[0], 3.0 * c[4]) + -2.0 * c[6];
    double vy = fma(-1.0, c[1], 3.0 * c[5]) + -2.0 * c[7];
    double uxx = ux * ux, uyy = uy * uy, vxx = vx * vx, vyy = vy * vy;
    double mu = uxx > uyy ? uxx : uyy;
    double mv = vxx > vyy ? vxx : vyy;
    return mu + mv;
}

// de Casteljau at t = 1/2 with the reference's 8x4 weight matrix (rows as dot4, shortened as described above):
//   l0 = (1, 0, 0, 0)              l1 = (.5, .5, 0, 0)   l2 = (.25, .5, .25, 0)   l3 = r0 = (.125, .375, .375, .125)
//   r1 = (0, .25, .5, .25)         r2 = (0, 0, .5, .5)   r3 = (0, 0, 0, 1)
SVGR_HD double split_mid(double x0, double x1, double x2, double x3) { return dot4(0.125, 0.375, 0.375, 0.125, x0, x1, x2, x3); }
SVGR_HD void cubic_left(const double* c, double* l) {
    for (int ax = 0; ax < 2; ++ax) {
        double x0 = c[ax], x1 = c[2 + ax], x2 = c[4 + ax], x3 = c[6 + ax];
        l[ax] = x0;
        l[2 + ax] = 0.5 * x0 + 0.5 * x1;
        l[4 + ax] = fma(0.25, x0, 0.25 * x2) + 0.5 * x1;
        l[6 + ax] = split_mid(x0, x1, x2, x3);
    }
}
SVGR_HD void cubic_right(const double* c, double* r) {
    for (int ax = 0; ax < 2; ++ax) {
        double x0 = c[ax], x1 = c[2 + ax], x2 = c[4 + ax], x3 = c[6 + ax];
        r[ax] = split_mid(x0, x1, x2, x3);
        r[2 + ax] = 0.5 * x2 + fma(0.25, x1, 0.25 * x3);
        r[4 + ax] = 0.5 * x2 + 0.5 * x3;
        r[6 + ax] = x3;
    }
}
// The two halves IN PLACE (same rows, evaluated in an order in which every input is still the old value): no
// temporary cubic and no copy back, which is a quarter of the instructions of the flatten kernel otherwise.
SVGR_HD void half_left(double& x0, double& x1, double& x2, double& x3) {
    x3 = split_mid(x0, x1, x2, x3);
    x2 = fma(0.25, x0, 0.25 * x2) + 0.5 * x1;
    x1 = 0.5 * x0 + 0.5 * x1;
}
SVGR_HD void half_right(double& x0, double& x1, double& x2, double& x3) {
    x0 = split_mid(x0, x1, x2, x3);
    x1 = 0.5 * x2 + fma(0.25, x1, 0.25 * x3);
    x2 = 0.5 * x2 + 0.5 * x3;
}
SVGR_HD void cubic_left_inplace(double* c) {
    half_left(c[0], c[2], c[4], c[6]);
    half_left(c[1], c[3], c[5], c[7]);
}
SVGR_HD void cubic_right_inplace(double* c) {
    half_right(c[0], c[2], c[4], c[6]);
    half_right(c[1], c[3], c[5], c[7]);
}
SVGR_HD void cubic_split(const double* c, double* l, double* r) {
    cubic_left(c, l);
    cubic_right(c, r);
}

// Depth-first adaptive subdivision. `emit(p0r, p0c, p1r, p1c)` is called once per flat piece,
// in curve order. Returns the number of pieces, or -1 when the depth cap was hit (non-finite
// or absurd input; the reference would never terminate there).
template <class Emit>
SVGR_HD int flatten_cubic(const double* cubic, double thr, Emit&& emit) {
    double stack[kMaxFlattenDepth][8];
    double cur[8];
    for (int i = 0; i < 8; ++i) cur[i] = cubic[i];
    int sp = 0, n = 0;
    bool overflow = false;
    for (;;) {
        bool flat = cubic_flatness(cur) < thr;
        if (!flat && sp >= kMaxFlattenDepth) { flat = true; overflow = true; }
        if (flat) {
            emit(cur[0], cur[1], cur[6], cur[7]);
            ++n;
            if (sp == 0) break;
            --sp;
            for (int i = 0; i < 8; ++i) cur[i] = stack[sp][i];
        } else {
            double l[8];
            cubic_split(cur, l, stack[sp]);
            ++sp;
            for (int i = 0; i < 8; ++i) cur[i] = l[i];
        }
    }
    return overflow ? -1 : n;
}

// Stack-free depth-first subdivision of the subtree under `root` (whose ancestors the caller has
// already found non-flat).  The position is a (level, path-bits) pair; stepping to a right sibling
// recomputes the node from `root` by `level` half-splits, which is the same sequence of roundings
// the recursive form performs, so the pieces are bit-identical -- and nothing spills to scratch.
// `emit(p0r, p0c, p1r, p1c)` once per flat piece in curve order; returns the piece count and sets
// `overflow` when `max_depth` forced a piece out (non-finite / absurd input).
// `ends` (optional): the end points of the first two pieces {r1, c1, r2, c2}, so that a caller that first counts and then
// stores can skip the second traversal for the (very common) subtrees of one or two pieces.
// (`NE`: how many first end points `ends` receives, {r, c} each)
template <int NE = 2, class Emit>
SVGR_HD int flatten_subtree(const double* root, double thr, int max_depth, Emit&& emit, bool& overflow, double* ends = nullptr) {
    double cur[8];
    for (int i = 0; i < 8; ++i) cur[i] = root[i];
    int level = 0, n = 0;
    unsigned long long idx = 0;
    double er[NE], ec[NE];
    for (int k = 0; k < NE; ++k) er[k] = ec[k] = 0.0;
    for (;;) {
        bool flat = cubic_flatness(cur) < thr;
        if (!flat && level >= max_depth) { flat = true; overflow = true; }
        if (flat) {
            emit(cur[0], cur[1], cur[6], cur[7]);
            for (int k = 0; k < NE; ++k) { er[k] = n == k ? cur[6] : er[k]; ec[k] = n == k ? cur[7] : ec[k]; }
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
    if (ends)
        for (int k = 0; k < NE; ++k) { ends[2 * k] = er[k]; ends[2 * k + 1] = ec[k]; }
    return n;
}

// ------------------------------------------------------------------------------------
// order-preserving double <-> uint64 key (for integer atomicMin / atomicMax on coordinates)
// ------------------------------------------------------------------------------------
SVGR_HD uint64_t f64_key(double v) {
    union { double d; uint64_t u; } x;
    x.d = v;
    return (x.u >> 63) ? ~x.u : (x.u | 0x8000000000000000ull);
}
SVGR_HD double key_f64(uint64_t k) {
    union { double d; uint64_t u; } x;
    x.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return x.d;
}

// double -> int for values that are integral already (floor / ceil results) or get truncated toward zero.
// On the device v_cvt_i32_f64 saturates by itself (and gives 0 for a NaN); the host build clamps explicitly.
// Coordinates beyond +-1e9 are rejected before they get here (k_path_bbox), so both forms agree on everything used.
SVGR_HD int clamp_to_int(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2int_rz(v);
#else
    v = v < -1.0e9 ? -1.0e9 : (v > 1.0e9 ? 1.0e9 : v);
    return (int)v;
#endif
}

// ------------------------------------------------------------------------------------
// A path's layer: the integer bbox of its folded min / max keys (Path.mask: floor - 1 / ceil + 1, cut to the viewport,
// S:968-971), the bands of `tr` rows and the column tiles of `tc` columns it covers.  ONE statement of the rule: k_path_bbox
// places a path by it, and a render that keeps the plan's slab table (k_path_build<1>) checks the plan's record against it.
// ------------------------------------------------------------------------------------
// column tiles [ct0, ct0 + nct) of `tc` columns that the layer columns [c0, c0 + cols) of a viewport starting at column vc0 span
SVGR_HD void span_ctiles(int c0, int cols, int vc0, int tc, int& ct0, int& nct) {
    ct0 = (c0 - vc0) / tc;
    nct = (c0 + cols - 1 - vc0) / tc - ct0 + 1;
}
struct PathBox {
    int r0, c0, rows, cols;   // the layer (rows = cols = 0: empty; r0 / c0 then the clamped lower corner)
    int b0, nb, nct;          // first band, bands, column tiles (0 when empty)
    int refused;              // an extent beyond +-1e9 pixels or not finite: error bit 16, everything else 0
};
// k[0], k[1]: ~f64_key of the smallest row / column; k[2], k[3]: f64_key of the largest (k[0] == 0: the path made no edge)
SVGR_HD PathBox path_box(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, int has_vp, int vr0, int vc0, int vrows, int vcols,
                         int tr, int tc) {
    PathBox o;
    o.r0 = o.c0 = o.rows = o.cols = o.b0 = o.nb = o.nct = o.refused = 0;
    if (k0 == 0ull) return o;
    double mnr = key_f64(~k0), mnc = key_f64(~k1);
    double mxr = key_f64(k2), mxc = key_f64(k3);
    const double lim = 1.0e9;
    // (finite extents only: an infinite or NaN coordinate falls through to the refusal below, as it did before the clamp)
    const double fmax = 1.7976931348623157e308;
    if (has_vp && fabs(mnr) <= fmax && fabs(mnc) <= fmax && fabs(mxr) <= fmax && fabs(mxc) <= fmax) {
        // With a viewport the bbox is cut to it anyway (S:968-971): an extent beyond the 32-bit pixel range (the
        // reference computes it in Python integers) is brought to the viewport's border first, in double.  Only a
        // render WITHOUT a viewport is limited to +-1e9 pixels.
        const double r_lo = (double)vr0 - 4.0, r_hi = (double)vr0 + (double)vrows + 4.0;
        const double c_lo = (double)vc0 - 4.0, c_hi = (double)vc0 + (double)vcols + 4.0;
        mnr = mnr < r_lo ? r_lo : (mnr > r_hi ? r_hi : mnr); mxr = mxr < r_lo ? r_lo : (mxr > r_hi ? r_hi : mxr);
        mnc = mnc < c_lo ? c_lo : (mnc > c_hi ? c_hi : mnc); mxc = mxc < c_lo ? c_lo : (mxc > c_hi ? c_hi : mxc);
    }
    if (!(mnr > -lim && mnc > -lim && mxr < lim && mxc < lim)) {
        o.refused = 1;
        return o;
    }
    long long lo_r = (long long)floor(mnr) - 1, lo_c = (long long)floor(mnc) - 1;
    long long hi_r = (long long)ceil(mxr) + 1, hi_c = (long long)ceil(mxc) + 1;
    if (has_vp) {
        lo_r = lo_r > vr0 ? lo_r : vr0;
        lo_c = lo_c > vc0 ? lo_c : vc0;
        hi_r = hi_r < (long long)vr0 + vrows ? hi_r : (long long)vr0 + vrows;
        hi_c = hi_c < (long long)vc0 + vcols ? hi_c : (long long)vc0 + vcols;
    }
    const long long rows = hi_r - lo_r, cols = hi_c - lo_c;
    if (rows > 0 && cols > 0) {
        o.r0 = (int)lo_r; o.c0 = (int)lo_c; o.rows = (int)rows; o.cols = (int)cols;
        const int base_r = has_vp ? vr0 : (int)lo_r;
        o.b0 = ((int)lo_r - base_r) / tr;
        o.nb = ((int)(hi_r - 1) - base_r) / tr - o.b0 + 1;
        int ct0_;
        span_ctiles((int)lo_c, (int)cols, has_vp ? vc0 : (int)lo_c, tc, ct0_, o.nct);
    } else {
        const long long big = 1ll << 30;
        o.r0 = (int)(lo_r > big ? big : (lo_r < -big ? -big : lo_r));
        o.c0 = (int)(lo_c > big ? big : (lo_c < -big ? -big : lo_c));
    }
    return o;
}
// does a record {r0, c0, rows, cols, bands} -- what a plan kept of a path -- state what the rule gives for the path's keys now?
SVGR_HD bool path_box_is(const PathBox& o, int r0, int c0, int rows, int cols, int nb) {
    return o.r0 == r0 && o.c0 == c0 && o.rows == rows && o.cols == cols && o.nb == nb;
}

// ------------------------------------------------------------------------------------
// One edge of a path, prepared the way line_signed_coverage prepares it (S:2230-2242):
// coordinates relative to the layer origin, oriented so rows increase.
// ------------------------------------------------------------------------------------
struct EdgeSetup {
    double p0y, p1y, dxdy, x, dir;  // x = column at the first traced row's entry
    int y_begin, y_end;             // traced rows [y_begin, y_end) (clipped to [0, rows))
    bool valid;
};

SVGR_HD EdgeSetup edge_setup(double ar, double ac, double br, double bc, int rows) {
    EdgeSetup e;
    e.valid = false;
    e.p0y = e.p1y = e.dxdy = e.x = 0.0;
    e.dir = 1.0;
    e.y_begin = e.y_end = 0;
    if (ar == br) return e;  // horizontal: no signed coverage
    double p0y = ar, p0x = ac, p1y = br, p1x = bc;
    if (!(ar < br)) {
        e.dir = -1.0;
        p0y = br; p0x = bc; p1y = ar; p1x = ac;
    }
    e.p0y = p0y;
    e.p1y = p1y;
    e.dxdy = (p1x - p0x) / (p1y - p0y);
    e.x = p0x;
    e.y_begin = clamp_to_int(p0y > 0.0 ? p0y : 0.0);
    if (p0y < 0.0) e.x -= p0y * e.dxdy;
    int yend = clamp_to_int(ceil(p1y));
    e.y_end = yend < rows ? yend : rows;
    e.valid = e.y_begin < e.y_end;
    return e;
}

// Row recurrence (S:2243-2248). After step(y): x/x_next are the columns where the edge enters
// and leaves row y, d the signed height.
struct RowState {
    double x_next;  // carried between rows
    double x, d;
};

SVGR_HD void row_step(RowState& s, int y, double p0y, double p1y, double dxdy, double dir) {
    s.x = s.x_next;
    double yhi = (double)(y + 1) < p1y ? (double)(y + 1) : p1y;
    double ylo = (double)y > p0y ? (double)y : p0y;
    double dy = yhi - ylo;
    s.d = dir * dy;
    s.x_next = s.x + dxdy * dy;
}

// Area pieces of one row (S:2250-2303). `put(xi, v)` receives the UNCLAMPED column index; it
// returns false to stop the row (the reference `continue`s once a column is >= w).
template <class Put>
SVGR_HD void row_pieces(double x, double x_next, double d, Put&& put) {
    double x0 = x < x_next ? x : x_next;
    double x1 = x < x_next ? x_next : x;
    double x0_floor = floor(x0);
    int x0i = clamp_to_int(x0_floor);
    double x1_ceil = ceil(x1);
    int x1i = clamp_to_int(x1_ceil);
    if (x1i <= x0i + 1) {
        double xmf = 0.5 * (x + x_next) - x0_floor;
        if (!put(x0i, d * (1 - xmf))) return;
        put(x0i + 1, d * xmf);
    } else {
        double s = 1 / (x1 - x0);
        double x0f = x0 - x0_floor;
        double x1f = x1 - x1_ceil + 1.0;
        double o = 1 - x0f;
        double a0 = 0.5 * s * (o * o);
        double am = 0.5 * s * (x1f * x1f);
        if (!put(x0i, d * a0)) return;
        if (x1i == x0i + 2) {
            if (!put(x0i + 1, d * (1.0 - a0 - am))) return;
        } else {
            double a1 = s * (1.5 - x0f);
            if (!put(x0i + 1, d * (a1 - a0))) return;
            double ds = d * s;
            for (int xi = x0i + 2; xi < x1i - 1; ++xi)
                if (!put(xi, ds)) return;
            double a2 = a1 + (double)(x1i - x0i - 3) * s;
            if (!put(x1i - 1, d * (1.0 - a2 - am))) return;
        }
        put(x1i, d * am);
    }
}

// The same pieces in closed form, so that they can be computed once per edge row and applied by
// every tile that the row touches:
//   n == 1 : pieces at x0i (v[0]) and x0i+1 (v[1])                                  (one-pixel case)
//   n == 2 : x0i (v[0]), x0i+1 (v[1]), x0i+2 (v[4])
//   n >= 3 : x0i (v[0]), x0i+1 (v[1]), x0i+2 .. x0i+n-2 (v[2] each), x0i+n-1 (v[3]), x0i+n (v[4])
// where n = x1i - x0i (n = 1 also covers x1i == x0i).  Values are exactly those of row_pieces.
struct RowPieces {
    int x0i, n;
    double v[5];
};

SVGR_HD RowPieces row_record(double x, double x_next, double d) {
    RowPieces r;
    double x0 = x < x_next ? x : x_next;
    double x1 = x < x_next ? x_next : x;
    double x0_floor = floor(x0);
    r.x0i = clamp_to_int(x0_floor);
    double x1_ceil = ceil(x1);
    int x1i = clamp_to_int(x1_ceil);
    r.v[2] = r.v[3] = r.v[4] = 0.0;
    if (x1i <= r.x0i + 1) {
        double xmf = 0.5 * (x + x_next) - x0_floor;
        r.n = 1;
        r.v[0] = d * (1 - xmf);
        r.v[1] = d * xmf;
    } else {
        double s = 1 / (x1 - x0);
        double x0f = x0 - x0_floor;
        double x1f = x1 - x1_ceil + 1.0;
        double o = 1 - x0f;
        double a0 = 0.5 * s * (o * o);
        double am = 0.5 * s * (x1f * x1f);
        r.n = x1i - r.x0i;
        r.v[0] = d * a0;
        r.v[4] = d * am;
        if (r.n == 2) {
            r.v[1] = d * (1.0 - a0 - am);
        } else {
            double a1 = s * (1.5 - x0f);
            r.v[1] = d * (a1 - a0);
            r.v[2] = d * s;
            double a2 = a1 + (double)(x1i - r.x0i - 3) * s;
            r.v[3] = d * (1.0 - a2 - am);
        }
    }
    return r;
}

// k_path_build<2>: an UPPER BOUND of the adds the rows of one edge leave in ONE column tile of one band, from where the edge
// enters the band (`x_in`, the column at the start of its first row there) and where it leaves it (`x_out`), over `nr` rows of a
// layer `cols` wide whose tiles cut a run of equal pieces every `px` columns.  A row leaves two pieces (the pixel it lies in, the
// carry into the next) plus one per column border it crosses (row_record: n + 1 pieces, n = borders + 1); x runs monotonically along
// an edge, so over the rows that is 2 nr + |floor(x_out) - floor(x_in)| -- exactly; the closed-form ends are widened by a relative 1e-9
// so that a value the row recurrence rounds to the other side of an integer counts as crossing it.  Borders outside the layer make
// no piece of their own: right of it nothing is stored, left of it every piece folds into column 0 (up to five adds there per row
// instead of two).  A long span is cut into runs: four single pieces and a run piece per `px` columns -- 6 nr + borders / px + 1 --,
// 13 per row and tile at most (tiles are 64 columns, px = 8).  `lo` / `hi`: the first and last column the rows can touch (before the
// carry piece's + 1), for the caller's tile range.  tests/test_core_host.py::test_band_room_bounds_every_cell checks it against
// the pieces row_step / row_record / record_adds make, cell by cell, on millions of random edges.
SVGR_HD int band_room(double x_in, double x_out, int nr, int cols, int px, int& lo, int& hi) {
    double xlo = x_in < x_out ? x_in : x_out, xhi = x_in < x_out ? x_out : x_in;
    xlo -= 1e-9 * (1.0 + fabs(xlo));
    xhi += 1e-9 * (1.0 + fabs(xhi));
    lo = clamp_to_int(floor(xlo));
    hi = clamp_to_int(floor(xhi));
    const int lo_c = lo > -1 ? lo : -1;
    int hi_c = hi > -1 ? hi : -1;
    hi_c = hi_c < cols ? hi_c : cols;
    const int nc = hi_c - lo_c, fold = lo < 0 ? 3 * nr : 0;
    int room = 2 * nr + nc;
    room = room < 6 * nr + nc / px + 1 ? room : 6 * nr + nc / px + 1;
    return (room < 13 * nr ? room : 13 * nr) + fold;
}

// feed the pieces of a record to `put(xi, v)` in increasing column order; put returns false to stop
template <class Put>
SVGR_HD void apply_record(int x0i, int n, const double* v, Put&& put) {
    if (!put(x0i, v[0])) return;
    if (!put(x0i + 1, v[1])) return;
    if (n >= 3) {
        for (int xi = x0i + 2; xi < x0i + n - 1; ++xi)
            if (!put(xi, v[2])) return;
        if (!put(x0i + n - 1, v[3])) return;
    }
    if (n >= 2) put(x0i + n, v[4]);
}

// column span touched by a row, without computing the pieces: [lo, hi] inclusive
SVGR_HD void row_span(double x, double x_next, int& lo, int& hi) {
    double x0 = x < x_next ? x : x_next;
    double x1 = x < x_next ? x_next : x;
    lo = clamp_to_int(floor(x0));
    int x1i = clamp_to_int(ceil(x1));
    hi = (x1i <= lo + 1) ? lo + 1 : x1i;
}

// ------------------------------------------------------------------------------------
// fill rules + zero cut (S:984-990)
// ------------------------------------------------------------------------------------
// *_raw: before the zero cut (callers that only need "is it >= 1e-6" skip the select)
SVGR_HD double fill_nonzero_raw(double s) {
    double m = fabs(s);
    return m > 1.0 ? 1.0 : m;
}
SVGR_HD double fill_nonzero(double s) {
    double m = fill_nonzero_raw(s);
    return m < kZeroCut ? 0.0 : m;
}
SVGR_HD double fill_evenodd_raw(double s) {
    double a = s + 1.0;
    double r = a - 2.0 * floor(a * 0.5);
    return fabs(r - 1.0);
}
SVGR_HD double fill_evenodd(double s) {
    // np.remainder(a, 2.0) (sign follows the divisor) without fmod: a/2, floor, *2 and the final
    // subtraction are all exact for a power-of-two divisor, so r == a - 2*floor(a/2) bit for bit
    double a = s + 1.0;
    double r = a - 2.0 * floor(a * 0.5);
    double m = fabs(r - 1.0);
    return m < kZeroCut ? 0.0 : m;
}
SVGR_HD double fill_rule(double s, int rule) { return rule ? fill_evenodd(s) : fill_nonzero(s); }

// ------------------------------------------------------------------------------------
// source-over of one premultiplied pixel: dst = src + dst * (1 - src_a)   (S:286)
// ------------------------------------------------------------------------------------
SVGR_HD void over_px(double* dst, double s0, double s1, double s2, double s3) {
    double k = 1 - s3;
    dst[0] = s0 + dst[0] * k;
    dst[1] = s1 + dst[1] * k;
    dst[2] = s2 + dst[2] * k;
    dst[3] = s3 + dst[3] * k;
}

// float32-output variant: dst = fma(dst, 1 - src_a, src).  One rounding less than the reference's
// mul-then-add per channel (<= 0.5 ulp of a double closer to the exact value); only used where the
// canvas is rounded to float32 on store, the double outputs keep over_px.
SVGR_HD void over_px_fma(double* dst, double s0, double s1, double s2, double s3) {
    double k = 1 - s3;
    dst[0] = fma(dst[0], k, s0);
    dst[1] = fma(dst[1], k, s1);
    dst[2] = fma(dst[2], k, s2);
    dst[3] = fma(dst[3], k, s3);
}

// The final clamp of the filter primitives below: [0, 1], and NaN -> 0 (every comparison with NaN is false), so that a
// NaN pixel or a NaN intermediate never leaves a primitive.  -0 becomes +0; every other value is what
// `r < 0 ? 0 : (r > 1 ? 1 : r)` gives.  clamp_to is the same with an upper end `hi` of its own, itself a clamped value.
SVGR_HD double clamp_unit(double r) { return r > 0.0 ? (r < 1.0 ? r : 1.0) : 0.0; }
SVGR_HD double clamp_to(double r, double hi) { return r > 0.0 ? (r < hi ? r : hi) : 0.0; }

// ------------------------------------------------------------------------------------
// feTurbulence (SVG 1.1 / Filter Effects 1, the spec's C reference code).  The lattice depends on the seed only and is
// set up on the host once per primitive (turb_init); turb_point evaluates the four channels of one user-space point.
// Gradients are stored lattice-major: grad[(i * 4 + k) * 2 + axis] = the spec's gradient[k][i][axis], so the eight
// numbers one lattice point contributes to the four channels sit side by side.  Indices and stitch state are int64:
// the spec's ints overflow once `wrap` has doubled for twenty octaves.  Every finite coordinate has a defined result
// (turb_cell), and a stitch state that would leave the exactly representable integers is refused (turb_params_valid):
// no conversion is out of range and no integer overflows (DESIGN.md "Filter primitives at the edges of their values").
// ------------------------------------------------------------------------------------
constexpr int kTurbBSize = 0x100, kTurbBM = 0xff, kTurbN = 0x1000;
constexpr int kTurbLattice = kTurbBSize + kTurbBSize + 2;   // 514
constexpr int kTurbMaxOctaves = 32;
constexpr int64_t kTurbM = 2147483647, kTurbA = 16807, kTurbQ = 127773, kTurbR = 2836;

SVGR_HD int64_t turb_setup_seed(int64_t s) {
    if (s <= 0) s = -(s % (kTurbM - 1)) + 1;
    if (s > kTurbM - 1) s = kTurbM - 1;
    return s;
}

SVGR_HD int64_t turb_random(int64_t s) {
    int64_t r = kTurbA * (s % kTurbQ) - kTurbR * (s / kTurbQ);
    if (r <= 0) r += kTurbM;
    return r;
}

// sel: 514 ints, grad: 514 * 4 * 2 doubles.  A zero gradient (both draws 256) stays zero instead of 0 / 0.
SVGR_HD void turb_init(int64_t seed, int* sel, double* grad) {
    int64_t s = turb_setup_seed(seed);
    for (int k = 0; k < 4; ++k) {
        for (int i = 0; i < kTurbBSize; ++i) {
            sel[i] = i;
            for (int j = 0; j < 2; ++j) {
                s = turb_random(s);
                grad[(i * 4 + k) * 2 + j] = (double)(s % (2 * kTurbBSize) - kTurbBSize) / kTurbBSize;
            }
            double* g = grad + (i * 4 + k) * 2;
            const double len = sqrt(g[0] * g[0] + g[1] * g[1]);
            if (len > 0.0) {
                g[0] = g[0] / len;
                g[1] = g[1] / len;
            }
        }
    }
    for (int i = kTurbBSize - 1; i > 0; --i) {
        const int t = sel[i];
        s = turb_random(s);
        const int j = (int)(s % kTurbBSize);
        sel[i] = sel[j];
        sel[j] = t;
    }
    for (int i = 0; i < kTurbBSize + 2; ++i) {
        sel[kTurbBSize + i] = sel[i];
        for (int q = 0; q < 8; ++q) grad[(kTurbBSize + i) * 8 + q] = grad[i * 8 + q];
    }
}

// Everything of a primitive that is the same for every pixel: the (stitch-adjusted) base frequencies and the stitch state
// of the first octave.  tile = {x, y, width, height} in user space.
struct TurbParams {
    double fx, fy;
    int64_t width, height, wrap_x, wrap_y;
    int octaves, fractal, stitch;
};

SVGR_HD double turb_stitch_freq(double f, double w) {
    const double lo = floor(w * f) / w, hi = ceil(w * f) / w;
    return f / lo < hi / f ? lo : hi;
}

// What turb_params and turb_point accept: finite base frequencies >= 0 and, when stitching, a finite tile of positive
// width and height whose stitch state stays within the exactly representable integers up to the last octave.  The state
// of octave k is width_k = 2^k width_0 and wrap_k = 2^k (wrap_0 - 4096) + 4096 (wrap' = 2 wrap - 4096 unrolled), with
// width_0 = trunc(tile.w f + 0.5) and wrap_0 = trunc(tile.x f + 4096 + width_0), f the adjusted frequency; the last
// octave is k = octaves - 1.  So the bound is  2^(octaves - 1) max(width_0, |wrap_0 - 4096|) + 4096 <= 2^53  on each axis.
constexpr double kTurbStateMax = 9007199254740992.0;   // 2^53

SVGR_HD bool turb_axis_valid(double f, double t0, double tw, double scale) {
    if (!(tw > 0.0)) return false;
    if (f != 0.0) f = turb_stitch_freq(f, tw);
    const double w0 = tw * f + 0.5;
    if (!(f >= 0.0) || !(w0 < kTurbStateMax)) return false;   // (NaN and inf fail both)
    const double width = trunc(w0), r0 = t0 * f + kTurbN + width;
    if (!(fabs(r0) < kTurbStateMax)) return false;
    const double wrap = trunc(r0);
    return scale * fmax(width, fabs(wrap - kTurbN)) + kTurbN <= kTurbStateMax;
}

SVGR_HD bool turb_params_valid(double fx, double fy, const double* tile, int octaves, int stitch) {
    if (!(fx >= 0.0 && fx <= 1.7976931348623157e308) || !(fy >= 0.0 && fy <= 1.7976931348623157e308)) return false;
    if (octaves < 0 || octaves > kTurbMaxOctaves) return false;
    if (!stitch) return true;
    for (int k = 0; k < 4; ++k)
        if (!(fabs(tile[k]) <= 1.7976931348623157e308)) return false;
    const double scale = (double)((int64_t)1 << (octaves > 0 ? octaves - 1 : 0));
    return turb_axis_valid(fx, tile[0], tile[2], scale) && turb_axis_valid(fy, tile[1], tile[3], scale);
}

// The caller has checked turb_params_valid: every conversion below is in range.
SVGR_HD TurbParams turb_params(double fx, double fy, const double* tile, int octaves, int fractal, int stitch) {
    TurbParams p;
    p.octaves = octaves;
    p.fractal = fractal;
    p.stitch = stitch;
    p.width = p.height = p.wrap_x = p.wrap_y = 0;
    if (stitch) {
        if (fx != 0.0) fx = turb_stitch_freq(fx, tile[2]);
        if (fy != 0.0) fy = turb_stitch_freq(fy, tile[3]);
        p.width = (int64_t)(tile[2] * fx + 0.5);
        p.wrap_x = (int64_t)(tile[0] * fx + kTurbN + (double)p.width);
        p.height = (int64_t)(tile[3] * fy + 0.5);
        p.wrap_y = (int64_t)(tile[1] * fy + kTurbN + (double)p.height);
    }
    p.fx = fx;
    p.fy = fy;
    return p;
}

SVGR_HD double turb_s_curve(double t) { return t * t * (3.0 - 2.0 * t); }

// The lattice cell of coordinate t: its integer part (toward zero) and frac = t - trunc(t), which is 0 from 2^52 on.  The
// integer part is clamped to +-2^62 before it is converted, so no conversion is out of range.  Beyond 2^62, t is a multiple
// of 2^10, and +-2^62 stands in for it: the same residue modulo 256 (0), the same side of every stitch wrap
// (|wrap| <= 2^53 + 4096), and room for the + 1 and - width that follow.  So the index is that of the exact integer part in
// unbounded integers.  An infinite t (an overflowed product of finite numbers) has the fraction inf - inf = NaN, as has a NaN t
// (from a non-finite coordinate): the point's noise is NaN, which the final clamp turns into 0 in every channel.  The clamp
// is two f64 min / max in front of the conversion, and the fraction no longer needs the way back from int64: together no
// slower than the bare cast (profiles/filter_edges/README.md, which also has the forms that were slower).
SVGR_HD int64_t turb_cell(double t, double& frac) {
    const double it = trunc(t);
    frac = t - it;
    return (int64_t)fmin(fmax(it, -4611686018427387904.0), 4611686018427387904.0);   // (fmax drops a NaN: -2^62)
}

// The four channels of feTurbulence at user-space point (px, py), clamped to [0, 1] (straight alpha, RGBA).  The lattice
// indices, the s-curves and the stitch state of an octave are shared by the channels; each channel then runs the spec's
// noise2 arithmetic in the spec's order.
// sel and grad are read by index only (pointers in the product; the unit tests pass bounds-checked views).
template <class Sel, class Grad>
SVGR_HD void turb_point(Sel sel, Grad grad, const TurbParams& p, double px, double py, double* out) {
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    double vx = px * p.fx, vy = py * p.fy, ratio = 1.0;
    int64_t width = p.width, height = p.height, wrap_x = p.wrap_x, wrap_y = p.wrap_y;
    for (int o = 0; o < p.octaves; ++o) {
        const double tx = vx + kTurbN, ty = vy + kTurbN;
        double rx0, ry0;
        int64_t bx0 = turb_cell(tx, rx0), by0 = turb_cell(ty, ry0);
        int64_t bx1 = bx0 + 1, by1 = by0 + 1;
        const double rx1 = rx0 - 1.0, ry1 = ry0 - 1.0;
        if (p.stitch) {
            if (bx0 >= wrap_x) bx0 -= width;
            if (bx1 >= wrap_x) bx1 -= width;
            if (by0 >= wrap_y) by0 -= height;
            if (by1 >= wrap_y) by1 -= height;
        }
        bx0 &= kTurbBM; bx1 &= kTurbBM; by0 &= kTurbBM; by1 &= kTurbBM;
        const int i = sel[bx0], j = sel[bx1];
        const int b00 = sel[i + by0], b10 = sel[j + by0], b01 = sel[i + by1], b11 = sel[j + by1];
        const double sx = turb_s_curve(rx0), sy = turb_s_curve(ry0);
        for (int k = 0; k < 4; ++k) {
            const int q00 = (b00 * 4 + k) * 2, q10 = (b10 * 4 + k) * 2, q01 = (b01 * 4 + k) * 2, q11 = (b11 * 4 + k) * 2;
            double u = rx0 * grad[q00] + ry0 * grad[q00 + 1];
            double v = rx1 * grad[q10] + ry0 * grad[q10 + 1];
            const double a = u + sx * (v - u);
            u = rx0 * grad[q01] + ry1 * grad[q01 + 1];
            v = rx1 * grad[q11] + ry1 * grad[q11 + 1];
            const double b = u + sx * (v - u);
            const double n = a + sy * (b - a);
            sum[k] = sum[k] + (p.fractal ? n : fabs(n)) / ratio;
        }
        vx = vx * 2.0;
        vy = vy * 2.0;
        ratio = ratio * 2.0;
        if (p.stitch) {
            width = width + width;
            height = height + height;
            wrap_x = 2 * wrap_x - kTurbN;
            wrap_y = 2 * wrap_y - kTurbN;
        }
    }
    for (int k = 0; k < 4; ++k) {
        double c = p.fractal ? (sum[k] + 1.0) * 0.5 : sum[k];
        out[k] = clamp_unit(c);
    }
}

// ------------------------------------------------------------------------------------
// feComponentTransfer: one transfer function on one channel value (straight alpha).  type: 0 identity, 1 table,
// 2 discrete, 3 linear, 4 gamma; prm = {slope, intercept, amplitude, exponent, offset}; v = the n table values.
// ------------------------------------------------------------------------------------
enum { kXferIdentity = 0, kXferTable = 1, kXferDiscrete = 2, kXferLinear = 3, kXferGamma = 4 };

// v is read by index only (a pointer in the product; the unit tests pass a bounds-checked view).
template <class Table>
SVGR_HD double transfer_fn(double c, int type, const double* prm, Table v, int n) {
    c = c > 0.0 ? (c < 1.0 ? c : 1.0) : 0.0;   // (NaN -> 0: it must not reach a table index)
    double r = c;
    if (type == kXferTable && n > 0) {
        if (n == 1) {
            r = v[0];
        } else {
            const int m = n - 1;
            const double t = c * m;
            int k = (int)floor(t);
            k = k < m - 1 ? k : m - 1;
            r = v[k] + (t - k) * (v[k + 1] - v[k]);
        }
    } else if (type == kXferDiscrete && n > 0) {
        int k = (int)floor(c * n);
        k = k < n - 1 ? k : n - 1;
        r = v[k];
    } else if (type == kXferLinear) {
        r = prm[0] * c + prm[1];
    } else if (type == kXferGamma) {
        r = prm[2] * pow(c, prm[3]) + prm[4];
    }
    return clamp_unit(r);   // (a NaN from finite parameters, 0 * inf or a huge table's inf - inf, ends as 0)
}

// ------------------------------------------------------------------------------------
// feConvolveMatrix: what follows the weighted sums s[0..3] of one pixel.  s / divisor + bias, then preserve = 0: alpha clamped
// to [0, 1] and the premultiplied colours to [0, alpha]; 1: the straight colours clamped to [0, 1] and `alpha` (the source
// pixel's) copied.  A NaN sum -- a NaN pixel anywhere under the kernel, weight 0 included, or inf - inf -- ends as 0.
// ------------------------------------------------------------------------------------
SVGR_HD void convolve_finish(double* s, double divisor, double bias, int preserve, double alpha) {
    s[0] = s[0] / divisor + bias;
    s[1] = s[1] / divisor + bias;
    s[2] = s[2] / divisor + bias;
    if (preserve) {
        s[0] = clamp_unit(s[0]); s[1] = clamp_unit(s[1]); s[2] = clamp_unit(s[2]);
        s[3] = alpha;
    } else {
        const double al = clamp_unit(s[3] / divisor + bias);
        s[0] = clamp_to(s[0], al); s[1] = clamp_to(s[1], al); s[2] = clamp_to(s[2], al);
        s[3] = al;
    }
}

// ------------------------------------------------------------------------------------
// feDiffuseLighting / feSpecularLighting: one output pixel from the 3 x 3 alpha neighbourhood around it (Filter Effects 1).
// Device frame (d0 = row, d1 = column, z); a[3 k + j] is the alpha at row offset k - 1 and column offset j - 1, zero outside
// the input.  top / bottom / left / right: the pixel is in the first / last row / column of the region (the spec's Sobel table,
// include/svgr.h).  light.l: distant {L0, L1, L2} (unit, constant); point {P0, P1, P2}; spot {P0, P1, P2, S0, S1, S2 (unit),
// spot exponent, cos of the cone (-1: no cone)}.
// ------------------------------------------------------------------------------------
enum { kLightDistant = 0, kLightPoint = 1, kLightSpot = 2 };

struct LightParams {
    double l[8];
    double color[3];
    double surface_scale, constant, specular_exponent;
    int kind, specular;
};

// N (unit) from the neighbourhood.  Along each axis: the difference across the pixel (hi - lo, one-sided at an edge) in each
// of the three lines across it, weighted 1, 2, 1 (a line outside the region weighs 0) and summed in line order; times
// -surface_scale * 2 / (sum of the weights * the span of the difference).  A region one row or one column wide is flat.
SVGR_HD void light_normal(const double* a, int top, int bottom, int left, int right, double ss, double* n) {
    if ((top && bottom) || (left && right)) {
        n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
        return;
    }
    const int r_lo = top ? 1 : 0, r_hi = bottom ? 1 : 2, c_lo = left ? 1 : 0, c_hi = right ? 1 : 2;
    const double wt = top ? 0.0 : 1.0, wb = bottom ? 0.0 : 1.0;     // weights of the rows above / below
    const double wl = left ? 0.0 : 1.0, wr = right ? 0.0 : 1.0;     // and of the columns left / right
    // along d0: column-wise differences (row r_hi - row r_lo), columns left, centre, right
    const double g0 = wl * (a[3 * r_hi + 0] - a[3 * r_lo + 0]) + 2.0 * (a[3 * r_hi + 1] - a[3 * r_lo + 1]) + wr * (a[3 * r_hi + 2] - a[3 * r_lo + 2]);
    // along d1: row-wise differences (column c_hi - column c_lo), rows top, middle, bottom
    const double g1 = wt * (a[c_hi] - a[c_lo]) + 2.0 * (a[3 + c_hi] - a[3 + c_lo]) + wb * (a[6 + c_hi] - a[6 + c_lo]);
    const double f0 = 2.0 / ((wl + 2.0 + wr) * (double)(r_hi - r_lo));
    const double f1 = 2.0 / ((wt + 2.0 + wb) * (double)(c_hi - c_lo));
    const double n0 = -ss * f0 * g0, n1 = -ss * f1 * g1;
    const double len = sqrt(n0 * n0 + n1 * n1 + 1.0);
    n[0] = n0 / len; n[1] = n1 / len; n[2] = 1.0 / len;
}

// One pixel: (d0, d1) its device centre, a / edge flags as for light_normal.  out = {r, g, b, a}: diffuse opaque, specular
// premultiplied (alpha = the largest colour channel).
SVGR_HD void light_pixel(const LightParams& p, const double* a, int top, int bottom, int left, int right, double d0, double d1,
                         double* out) {
    double n[3];
    light_normal(a, top, bottom, left, right, p.surface_scale, n);
    double l0, l1, l2;
    if (p.kind == kLightDistant) {
        l0 = p.l[0]; l1 = p.l[1]; l2 = p.l[2];
    } else {
        const double v0 = p.l[0] - d0, v1 = p.l[1] - d1, v2 = p.l[2] - p.surface_scale * a[4];
        const double len = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
        if (len > 0.0) {
            l0 = v0 / len; l1 = v1 / len; l2 = v2 / len;
        } else {
            l0 = 0.0; l1 = 0.0; l2 = 1.0;
        }
    }
    double c0 = p.color[0], c1 = p.color[1], c2 = p.color[2];
    if (p.kind == kLightSpot) {
        const double m = -(l0 * p.l[3] + l1 * p.l[4] + l2 * p.l[5]);
        if (m > 0.0 && m >= p.l[7]) {
            const double f = pow(m, p.l[6]);
            c0 = c0 * f; c1 = c1 * f; c2 = c2 * f;
        } else {
            c0 = 0.0; c1 = 0.0; c2 = 0.0;
        }
    }
    double k;
    if (p.specular) {
        const double h0 = l0, h1 = l1, h2 = l2 + 1.0;
        const double len = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
        double nh = 0.0;
        if (len > 0.0) nh = n[0] * (h0 / len) + n[1] * (h1 / len) + n[2] * (h2 / len);
        nh = nh > 0.0 ? nh : 0.0;
        k = p.constant * pow(nh, p.specular_exponent);
    } else {
        const double nl = n[0] * l0 + n[1] * l1 + n[2] * l2;
        k = p.constant * (nl > 0.0 ? nl : 0.0);
    }
    double r = k * c0, g = k * c1, b = k * c2;
    r = clamp_unit(r); g = clamp_unit(g); b = clamp_unit(b);   // (a NaN alpha in the neighbourhood ends as 0)
    out[0] = r; out[1] = g; out[2] = b;
    out[3] = p.specular ? (r > g ? (r > b ? r : b) : (g > b ? g : b)) : 1.0;
}

// ------------------------------------------------------------------------------------
// mix-blend-mode (W3C Compositing and Blending Level 1, sections 5.1-5.9): one pixel of a premultiplied source over a
// premultiplied backdrop.  Modes in the spec's order (SVGR_BLEND_*, include/svgr.h); 0..11 separable, 12..15 not.
// With Cb = cb / ab and Cs = cs / as (0 where the alpha is 0):
//   co = cs (1 - ab) + cb (1 - as) + as ab B(Cb, Cs),  ao = as + ab (1 - as)
// Normal is computed as source-over, co = cs + cb (1 - as) (over_px's expression): the same value in exact arithmetic,
// and bit for bit what Layer.compose(OVER) gives.
// ------------------------------------------------------------------------------------
enum {
    kBlendNormal = 0, kBlendMultiply, kBlendScreen, kBlendOverlay, kBlendDarken, kBlendLighten, kBlendColorDodge,
    kBlendColorBurn, kBlendHardLight, kBlendSoftLight, kBlendDifference, kBlendExclusion,
    kBlendHue, kBlendSaturation, kBlendColor, kBlendLuminosity, kBlendModes
};

// B(Cb, Cs) of a separable mode, one channel
SVGR_HD double blend_sep(int mode, double b, double s) {
    switch (mode) {
        case kBlendMultiply: return b * s;
        case kBlendScreen: return b + s - b * s;
        case kBlendOverlay: {   // HardLight(Cs, Cb): the roles swapped
            const double b2 = 2.0 * b;
            return b <= 0.5 ? s * b2 : s + (b2 - 1.0) - s * (b2 - 1.0);
        }
        case kBlendDarken: return b < s ? b : s;
        case kBlendLighten: return b > s ? b : s;
        case kBlendColorDodge: {
            if (b == 0.0) return 0.0;
            if (s == 1.0) return 1.0;
            const double q = b / (1.0 - s);
            return q < 1.0 ? q : 1.0;
        }
        case kBlendColorBurn: {
            if (b == 1.0) return 1.0;
            if (s == 0.0) return 0.0;
            const double q = (1.0 - b) / s;
            return 1.0 - (q < 1.0 ? q : 1.0);
        }
        case kBlendHardLight: {
            const double s2 = 2.0 * s;
            return s <= 0.5 ? b * s2 : b + (s2 - 1.0) - b * (s2 - 1.0);
        }
        case kBlendSoftLight: {
            if (s <= 0.5) return b - (1.0 - 2.0 * s) * b * (1.0 - b);
            const double d = b <= 0.25 ? ((16.0 * b - 12.0) * b + 4.0) * b : sqrt(b);
            return b + (2.0 * s - 1.0) * (d - b);
        }
        case kBlendDifference: return b > s ? b - s : s - b;
        case kBlendExclusion: return b + s - 2.0 * b * s;
        default: return s;   // (normal)
    }
}

SVGR_HD double blend_lum(const double* c) { return 0.3 * c[0] + 0.59 * c[1] + 0.11 * c[2]; }

// SetLum(c, l) = ClipColor(c + (l - Lum(c))), in place.  ClipColor's divisions are skipped when their divisor is not positive
// (every channel equal to the luminance: nothing to clip towards it).
SVGR_HD void blend_set_lum(double* c, double l) {
    const double d = l - blend_lum(c);
    c[0] = c[0] + d; c[1] = c[1] + d; c[2] = c[2] + d;
    const double L = blend_lum(c);
    const double n = fmin(fmin(c[0], c[1]), c[2]), x = fmax(fmax(c[0], c[1]), c[2]);
    if (n < 0.0 && L - n > 0.0)
        for (int k = 0; k < 3; ++k) c[k] = L + ((c[k] - L) * L) / (L - n);
    if (x > 1.0 && x - L > 0.0)
        for (int k = 0; k < 3; ++k) c[k] = L + ((c[k] - L) * (1.0 - L)) / (x - L);
}

// SetSat(c, s), in place: the largest channel becomes s, the smallest 0, the middle one (Cmid - Cmin) s / (Cmax - Cmin); all 0
// when Cmax = Cmin.  Ties take the same value (two largest: both s; two smallest: both 0), whichever the spec's sort put first.
SVGR_HD void blend_set_sat(double* c, double s) {
    const double n = fmin(fmin(c[0], c[1]), c[2]), x = fmax(fmax(c[0], c[1]), c[2]);
    for (int k = 0; k < 3; ++k) {
        if (x <= n) c[k] = 0.0;
        else if (c[k] == x) c[k] = s;
        else if (c[k] == n) c[k] = 0.0;
        else c[k] = ((c[k] - n) * s) / (x - n);
    }
}

// B(Cb, Cs) of a non-separable mode: hue SetLum(SetSat(Cs, Sat(Cb)), Lum(Cb)), saturation SetLum(SetSat(Cb, Sat(Cs)), Lum(Cb)),
// color SetLum(Cs, Lum(Cb)), luminosity SetLum(Cb, Lum(Cs))
SVGR_HD void blend_nonsep(int mode, const double* b, const double* s, double* out) {
    double t[3];
    if (mode == kBlendHue || mode == kBlendColor) { t[0] = s[0]; t[1] = s[1]; t[2] = s[2]; }
    else { t[0] = b[0]; t[1] = b[1]; t[2] = b[2]; }
    if (mode == kBlendHue || mode == kBlendSaturation) {
        const double* f = mode == kBlendHue ? b : s;   // (the colour whose saturation is taken)
        blend_set_sat(t, fmax(fmax(f[0], f[1]), f[2]) - fmin(fmin(f[0], f[1]), f[2]));
    }
    blend_set_lum(t, blend_lum(mode == kBlendLuminosity ? s : b));
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
}

// One pixel, premultiplied in and out: d = the backdrop {cb, ab}, replaced by the result; s = the source.  `mode` is uniform
// over a launch: the kernel instantiates this per family (template parameter) and passes a constant.
SVGR_HD void mix_blend_px(int mode, double* d, const double* s) {
    const double ab = d[3], as = s[3];
    const double ka = 1.0 - as;
    if (mode == kBlendNormal) {
        d[0] = s[0] + d[0] * ka; d[1] = s[1] + d[1] * ka; d[2] = s[2] + d[2] * ka; d[3] = as + ab * ka;
        return;
    }
    double Cb[3], Cs[3], B[3];
    for (int k = 0; k < 3; ++k) {
        Cb[k] = ab > 0.0 ? d[k] / ab : 0.0;
        Cs[k] = as > 0.0 ? s[k] / as : 0.0;
    }
    if (mode >= kBlendHue) {
        blend_nonsep(mode, Cb, Cs, B);
    } else {
        for (int k = 0; k < 3; ++k) B[k] = blend_sep(mode, Cb[k], Cs[k]);
    }
    const double kb = 1.0 - ab, w = as * ab;
    for (int k = 0; k < 3; ++k) d[k] = (s[k] * kb + d[k] * ka) + w * B[k];
    d[3] = as + ab * ka;
}


// =====================================================================================
// JPEG pixel stage (read_jpeg; beyond the reference): coefficients -> 8-bit samples -> RGBA.
// Everything is integer arithmetic, so the host build of this file (tests/jpeg_harness.cpp) and the
// kernels (k_jpeg_idct, k_jpeg_colour) produce the same bits.
//
// Inverse DCT: the separable definition itself, s(y, x) = sum_v sum_u T[y][v] T[x][u] F(v, u) with
// T[k][j] = 1/2 c(j) cos((2k + 1) j pi / 16), c(0) = 1 / sqrt 2, as two 8-tap passes.  T is stored as
// round(2^15 T); the passes accumulate in 64 bits and nothing is rounded before the one shift at the
// end.  A dequantised coefficient is clamped to +-2^16: an 8-bit image cannot produce one beyond
// +-2^11 (+-2^12 after the quantiser's rounding), and with the clamp no stream, however corrupt, can
// overflow: sum_j |2^15 T[k][j]| < 2^17, so pass 1 stays below 2^33 and pass 2 below 2^50.
// =====================================================================================
constexpr int kJpegIdctBits = 15;
constexpr int32_t kJpegIdct[64] = {   // [k][j]: output k, frequency j
    11585,  16069,  15137,  13623,  11585,   9102,   6270,   3196,
    11585,  13623,   6270,  -3196, -11585, -16069, -15137,  -9102,
    11585,   9102,  -6270, -16069, -11585,   3196,  15137,  13623,
    11585,   3196, -15137,  -9102,  11585,  13623,  -6270, -16069,
    11585,  -3196, -15137,   9102,  11585, -13623,  -6270,  16069,
    11585,  -9102,  -6270,  16069, -11585,  -3196,  15137, -13623,
    11585, -13623,   6270,   3196, -11585,  16069, -15137,   9102,
    11585, -16069,  15137, -13623,  11585,  -9102,   6270,  -3196,
};

SVGR_HD int32_t jpeg_dequant(int16_t coef, uint16_t q) {
    const int32_t v = (int32_t)coef * (int32_t)q;   // (|v| <= 32768 * 65535 < 2^31)
    return v < -65536 ? -65536 : (v > 65536 ? 65536 : v);
}

// one 8-tap pass: out[k] = sum_j 2^15 T[k][j] in[j * stride]  (In: int32_t for the first pass, int64_t for the second)
template <class In>
SVGR_HD void jpeg_idct_pass(const In* in, int stride, int64_t* out) {
    SVGR_UNROLL
    for (int k = 0; k < 8; ++k) {
        int64_t acc = 0;
        SVGR_UNROLL
        for (int j = 0; j < 8; ++j) acc += (int64_t)kJpegIdct[8 * k + j] * (int64_t)in[j * stride];
        out[k] = acc;
    }
}

// the sample of a finished sum of both passes: scaled back (round half up), level shift, clamp
SVGR_HD uint8_t jpeg_sample(int64_t acc) {
    const int64_t v = ((acc + ((int64_t)1 << (2 * kJpegIdctBits - 1))) >> (2 * kJpegIdctBits)) + 128;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// A whole block on one thread (the host harness; the kernel spreads the same calls over eight lanes per block): coef[64] in
// natural order, q[64] likewise, out = the block's top-left sample in a plane whose rows are `stride` bytes apart.
SVGR_HD void jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, int64_t stride) {
    int32_t d[64];
    int64_t t[64], row[8];
    for (int i = 0; i < 64; ++i) d[i] = jpeg_dequant(coef[i], q[i]);
    for (int u = 0; u < 8; ++u) {   // columns: t[y][u] = sum_v T[y][v] d[v][u]
        jpeg_idct_pass(d + u, 8, row);
        for (int y = 0; y < 8; ++y) t[8 * y + u] = row[y];
    }
    for (int y = 0; y < 8; ++y) {   // rows: s[y][x] = sum_u T[x][u] t[y][u]
        jpeg_idct_pass(t + 8 * y, 1, row);
        for (int x = 0; x < 8; ++x) out[y * stride + x] = jpeg_sample(row[x]);
    }
}

// A component's plane of samples: `w` x `h` of them are the component's own (its edge, for the replication below), in rows
// `stride` bytes apart; `hs`, `vs` = 1 or 2 full-resolution pixels per sample along each axis.
struct JpegPlane {
    const uint8_t* p;
    int64_t stride;
    int w, h, hs, vs;
};

// 16 x the component's value at full-resolution pixel (x, y).  Along a subsampled axis the pixel lies a quarter of a sample
// from its own sample's centre: 3/4 of that sample and 1/4 of the neighbour on the pixel's side, the edge sample repeated
// ("fancy" upsampling; not pixel replication).  Along a full-resolution axis the neighbour is the sample itself, so the same
// sum is 4 x the sample.  Exact: the one rounding comes after the colour matrix.
SVGR_HD int jpeg_upsampled16(const JpegPlane& c, int x, int y) {
    if (c.hs == 1 && c.vs == 1) return 16 * (int)c.p[y * c.stride + x];
    int x0 = x, x1 = x, y0 = y, y1 = y;
    if (c.hs == 2) {
        x0 = x >> 1;
        x1 = (x & 1) ? (x0 + 1 < c.w ? x0 + 1 : x0) : (x0 > 0 ? x0 - 1 : 0);
    }
    if (c.vs == 2) {
        y0 = y >> 1;
        y1 = (y & 1) ? (y0 + 1 < c.h ? y0 + 1 : y0) : (y0 > 0 ? y0 - 1 : 0);
    }
    const uint8_t *r0 = c.p + y0 * c.stride, *r1 = c.p + y1 * c.stride;
    const int near = 3 * (int)r0[x0] + (int)r0[x1], far = 3 * (int)r1[x0] + (int)r1[x1];
    return 3 * near + far;
}

// colour models of a frame
constexpr int kJpegGrey = 0, kJpegYCbCr = 1, kJpegRGB = 2;

SVGR_HD int jpeg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One pixel from its three 16 x samples (jpeg_upsampled16): R | G << 8 | B << 16 | 255 << 24.  YCbCr is the JFIF matrix
// (R = Y + 1.402 Cr', G = Y - 0.344136 Cb' - 0.714136 Cr', B = Y + 1.772 Cb', primes = minus 128) with the factors rounded
// to 16 fractional bits; 20 bits come off at the end, rounding half up.  Grey and RGB only drop the 4 bits.
SVGR_HD uint32_t jpeg_rgba(int colour, int s0, int s1, int s2) {
    int r, g, b;
    if (colour == kJpegYCbCr) {
        const int y = s0 * 65536 + (1 << 19), cb = s1 - 128 * 16, cr = s2 - 128 * 16;
        r = jpeg_clamp8((y + 91881 * cr) >> 20);
        g = jpeg_clamp8((y - 22553 * cb - 46802 * cr) >> 20);
        b = jpeg_clamp8((y + 116130 * cb) >> 20);
    } else {
        r = (s0 + 8) >> 4;
        g = colour == kJpegRGB ? (s1 + 8) >> 4 : r;
        b = colour == kJpegRGB ? (s2 + 8) >> 4 : r;
    }
    return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16 | 0xFF000000u;
}


// =====================================================================================
// JPEG encode stage (write_jpeg; beyond the reference): RGBA -> sample planes -> quantised coefficients,
// the decode stage run backwards.  Integer arithmetic again: the host build (tests/jpeg_enc_harness.cpp)
// and the kernels (k_jpeg_planes, k_jpeg_fdct) produce the same bits.
//
// Colour: the JFIF matrix Y = 0.299 R + 0.587 G + 0.114 B, Cb = -0.168736 R - 0.331264 G + 0.5 B + 128,
// Cr = 0.5 R - 0.418688 G - 0.081312 B + 128 with every factor stored as round(2^16 factor):
//     Y : 19595  38470   7471      Cb : -11058 -21710  32768      Cr : 32768 -27439  -5329
// (each row of Y sums to 2^16, each chroma row to 0: grey stays grey).  2^15 is added before the 16 bits
// come off with an arithmetic shift, which is rounding half up; the result is clamped to 0 .. 255 (pure
// blue gives Cb = 128 + 128).  Alpha is ignored.
//
// Chroma: the mean of the h x v (1 or 2 per axis) 8-bit values a sample covers, rounded half up -- the box filter whose
// samples sit where the decoder's triangle upsampler (jpeg_upsampled16) takes them to sit.  A plane is padded to whole
// MCUs by repeating the image's last column and row (the pixel index is clamped, before the colour matrix and the mean).
//
// Forward DCT: the transpose of the inverse above, with the same table: F(v, u) = sum_y sum_x T[y][v] T[x][u] (s(y, x) - 128)
// as two 8-tap passes over kJpegIdct = 2^15 T, nothing rounded in between, so a finished sum is 2^30 F whichever axis went
// first.  No overflow: |s - 128| <= 128 = 2^7 and sum_k |2^15 T[k][j]| < 2^17, so the first pass stays below 2^24 (int32)
// and the second below 2^41 (int64).  The quantiser divides the sum by q 2^30 in one step, rounding half away from zero:
// with n = |sum|, (n + q 2^29) / (q 2^30) = ((n + q 2^29) >> 30) / q exactly (floors of non-negative numbers nest), and
// the shifted numerator is below 2^12, so the division is a 32-bit one.  The quotient is clamped to what the Huffman
// categories of a baseline scan can carry: -1024 .. 1023 for DC (differences then fit category 11), +-1023 for AC
// (category 10).  8-bit samples cannot reach the AC clamp (|F(v, u)| <= 128 sum_k |T[k][v]| sum_k |T[k][u]| < 929 off DC); DC reaches -1024.
// =====================================================================================

// R | G << 8 | B << 16 (| A << 24, ignored) -> Y, Cb, Cr in 0 .. 255
SVGR_HD void jpeg_ycc(uint32_t px, int* y, int* cb, int* cr) {
    const int r = (int)(px & 255u), g = (int)((px >> 8) & 255u), b = (int)((px >> 16) & 255u);
    *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;   // (a weighted mean of bytes: no clamp needed)
    *cb = jpeg_clamp8(((-11058 * r - 21710 * g + 32768 * b + 32768) >> 16) + 128);
    *cr = jpeg_clamp8(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128);
}

// One H x V group of pixels (row-major in px): its H x V luma samples and the one chroma pair that covers it
template <int H, int V>
SVGR_HD void jpeg_group(const uint32_t* px, uint8_t* y, int* cb, int* cr) {
    int sb = 0, sr = 0;
    SVGR_UNROLL
    for (int i = 0; i < H * V; ++i) {
        int yy, b, r;
        jpeg_ycc(px[i], &yy, &b, &r);
        y[i] = (uint8_t)yy;
        sb += b;
        sr += r;
    }
    *cb = (sb + H * V / 2) / (H * V);
    *cr = (sr + H * V / 2) / (H * V);
}

// one 8-tap pass of the forward transform: out[j] = sum_k 2^15 T[k][j] in[k * stride]  (int32 in -> int32 out for the
// first pass, int32 in -> int64 out for the second)
template <class Out, class In>
SVGR_HD void jpeg_fdct_pass(const In* in, int stride, Out* out) {
    SVGR_UNROLL
    for (int j = 0; j < 8; ++j) {
        Out acc = 0;
        SVGR_UNROLL
        for (int k = 0; k < 8; ++k) acc += (Out)kJpegIdct[8 * k + j] * (Out)in[k * stride];
        out[j] = acc;
    }
}

// acc = 2^30 F, q = 1 .. 255: F / q rounded half away from zero
SVGR_HD int32_t jpeg_quantise(int64_t acc, uint16_t q) {
    const uint64_t n = (uint64_t)(acc < 0 ? -acc : acc);
    const uint32_t m = (uint32_t)((n + ((uint64_t)q << 29)) >> 30) / (uint32_t)q;
    return acc < 0 ? -(int32_t)m : (int32_t)m;
}
// the quantised value as the scan stores it (index 0 of a block is its DC)
SVGR_HD int16_t jpeg_coefficient(int64_t acc, uint16_t q, bool dc) {
    const int32_t v = jpeg_quantise(acc, q), lo = dc ? -1024 : -1023;
    return (int16_t)(v < lo ? lo : (v > 1023 ? 1023 : v));
}

// A whole block on one thread (the host harness; the kernel spreads the same sums over eight lanes per block): in = the
// block's top-left sample in a plane whose rows are `stride` bytes apart, q[64] and coef[64] in natural order.
SVGR_HD void jpeg_fdct_block(const uint8_t* in, int64_t stride, const uint16_t* q, int16_t* coef) {
    int32_t s[8], r[64];
    int64_t col[8];
    for (int y = 0; y < 8; ++y) {   // rows: r[y][u] = sum_x T[x][u] (s[y][x] - 128)
        for (int x = 0; x < 8; ++x) s[x] = (int32_t)in[y * stride + x] - 128;
        jpeg_fdct_pass(s, 1, r + 8 * y);
    }
    for (int u = 0; u < 8; ++u) {   // columns: F[v][u] = sum_y T[y][v] r[y][u]
        jpeg_fdct_pass(r + u, 8, col);
        for (int v = 0; v < 8; ++v) coef[8 * v + u] = jpeg_coefficient(col[v], q[8 * v + u], v == 0 && u == 0);
    }
}

// A whole frame on one thread (the host harness): rgba = height x width pixels, hmax x vmax = the luma sampling factors
// (chroma has 1 x 1; n_comp = 1: a grey frame, Y alone), planes = room for the MCU-padded planes (64 bytes per block, the
// components one after the other), coef = the coefficients in the layout of include/svgr.h.
template <int H, int V>
SVGR_HD void jpeg_encode_frame_hv(const uint32_t* rgba, int width, int height, int n_comp, const uint16_t* quant, uint8_t* planes,
                                  int16_t* coef) {
    const int64_t mcus_x = (width + 8 * H - 1) / (8 * H), mcus_y = (height + 8 * V - 1) / (8 * V);
    const int64_t yw = mcus_x * 8 * H, yh = mcus_y * 8 * V, cw = mcus_x * 8, ch = mcus_y * 8;
    uint8_t *py = planes, *pb = py + yw * yh, *pr = pb + cw * ch;
    for (int64_t gy = 0; gy < ch; ++gy)
        for (int64_t gx = 0; gx < cw; ++gx) {
            uint32_t px[H * V];
            uint8_t y[H * V];
            int cb, cr;
            for (int j = 0; j < V; ++j)
                for (int i = 0; i < H; ++i) {
                    const int64_t sx = gx * H + i < width ? gx * H + i : width - 1, sy = gy * V + j < height ? gy * V + j : height - 1;
                    px[j * H + i] = rgba[sy * width + sx];
                }
            jpeg_group<H, V>(px, y, &cb, &cr);
            for (int j = 0; j < V; ++j)
                for (int i = 0; i < H; ++i) py[(gy * V + j) * yw + gx * H + i] = y[j * H + i];
            if (n_comp == 3) {
                pb[gy * cw + gx] = (uint8_t)cb;
                pr[gy * cw + gx] = (uint8_t)cr;
            }
        }
    int64_t b = 0;
    for (int c = 0; c < n_comp; ++c) {
        const uint8_t* p = c == 0 ? py : (c == 1 ? pb : pr);
        const int64_t bw = (c == 0 ? yw : cw) / 8, bh = (c == 0 ? yh : ch) / 8;
        for (int64_t by = 0; by < bh; ++by)
            for (int64_t bx = 0; bx < bw; ++bx, ++b) jpeg_fdct_block(p + by * 8 * bw * 8 + bx * 8, bw * 8, quant + 64 * c, coef + b * 64);
    }
}
SVGR_HD void jpeg_encode_frame(const uint32_t* rgba, int width, int height, int n_comp, int hmax, int vmax, const uint16_t* quant,
                               uint8_t* planes, int16_t* coef) {
    if (hmax == 2 && vmax == 2) jpeg_encode_frame_hv<2, 2>(rgba, width, height, n_comp, quant, planes, coef);
    else if (hmax == 2) jpeg_encode_frame_hv<2, 1>(rgba, width, height, n_comp, quant, planes, coef);
    else if (vmax == 2) jpeg_encode_frame_hv<1, 2>(rgba, width, height, n_comp, quant, planes, coef);
    else jpeg_encode_frame_hv<1, 1>(rgba, width, height, n_comp, quant, planes, coef);
}


// =====================================================================================
// feTile (k_layer_tile; beyond the reference): which pixel of the source layer an output pixel copies.
// Along one axis the tile covers the device coordinates [t0, t0 + tn) and the source layer [s0, s0 + sn).
// The output coordinate p repeats the tile: its tile coordinate is t = (p - t0) floor-mod tn (p may lie
// before t0; the caller keeps p - t0 inside an int), the next coordinate's is tile_next(t) -- a walk
// along an axis takes one modulo, not one per pixel --, and what p copies is the source index
// t0 + t - s0, or nothing (-1: transparent) where the tile reaches beyond the layer.  With t0 = the
// output's first coordinate and tn = its extent nothing repeats and the map is a plain crop
// ("window").  The two axes are independent.
// =====================================================================================
SVGR_HD int tile_wrap(int v, int n) {
    const int m = v % n;
    return m < 0 ? m + n : m;
}
SVGR_HD int tile_next(int t, int n) { return t + 1 == n ? 0 : t + 1; }
SVGR_HD int tile_source(int t, int t0, int s0, int sn) {
    const int64_t s = (int64_t)t0 + t - s0;
    return s >= 0 && s < sn ? (int)s : -1;
}

// =====================================================================================
// <image>: from a coordinate to texel indices (k_image_fill; on the host: tests/image_harness.cpp)
//
// image_corner: (x, y) in the texel grid of one (h, w) level, texel centres on the integers -> the four clamped indices of
// the bilinear footprint and its two fractions.  The corner is clamped in double before it becomes an index, so a NaN or
// huge coordinate lands on the edge, never outside the level: floor(NaN) goes through fmax(., -1) to -1, anything >= w to
// w; every index lies in [0, w - 1] / [0, h - 1] and both fractions in [0, 1].
// image_nearest: the level-0 texel (floor v, floor u) of nearest sampling, clamped the same way (NaN -> 0).
// =====================================================================================
#if !defined(__HIPCC__)
static inline int min(int a, int b) { return b < a ? b : a; }
static inline int max(int a, int b) { return a < b ? b : a; }
#endif
struct ImageCorner {
    int c0, c1, r0, r1;
    double fx, fy;
};
SVGR_HD ImageCorner image_corner(double x, double y, int w, int h) {
    const double xf = fmin(fmax(floor(x), -1.0), (double)w), yf = fmin(fmax(floor(y), -1.0), (double)h);
    const double fx = fmin(fmax(x - xf, 0.0), 1.0), fy = fmin(fmax(y - yf, 0.0), 1.0);
    const int xi = (int)xf, yi = (int)yf;
    const int c0 = min(max(xi, 0), w - 1), c1 = min(xi + 1, w - 1), r0 = min(max(yi, 0), h - 1), r1 = min(yi + 1, h - 1);
    return ImageCorner{c0, c1, r0, r1, fx, fy};
}
SVGR_HD void image_nearest(double u, double v, int w, int h, double& xf, double& yf) {
    xf = fmin(fmax(floor(u), 0.0), (double)(w - 1));
    yf = fmin(fmax(floor(v), 0.0), (double)(h - 1));
}

}  // namespace svgr
