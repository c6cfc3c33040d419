// svgr_dash.h -- per-lane arithmetic of the path dasher (stroke-dasharray / stroke-dashoffset, SVG 2 13.5).
//
// Everything here is plain double arithmetic without a data-dependent loop bound, compilable for the host (the CPU harness
// of tests/dash_harness.cpp) and for the device (the k_dash_* kernels of svgr_hip.hip).  DESIGN.md, "Dashed strokes", has
// the definitions; tests/dash_ref.py restates them in numpy / long double.
//
//   metric    a line is sqrt(dx^2 + dy^2) long; a cubic's parameter range is cut into DASH_SUB = 32 equal sub-intervals, each
//             measured by 4-point Gauss-Legendre quadrature of |B'(t)|; the cubic's length is their sum
//   pattern   DashPat: the dash list (used twice over when its count is odd, at most DASH_MAX entries then), its prefix sums
//             `pre`, the period P = pre[m], phase = offset mod P.  Interval (k, j) of the pattern is
//             [k P + pre[j], k P + pre[j + 1]); it is "on" when j is even.  Only on-intervals of non-zero length make pieces.
//   pieces    a segment owns the arc lengths [s0, s1) of its subpath; its pieces are the on-intervals that overlap that range
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DASH_HD __host__ __device__ inline
#else
#define DASH_HD inline
#endif

constexpr int DASH_SUB = 32;   // sub-intervals of a cubic (one per lane of a half-wave)
constexpr int DASH_MAX = 64;   // pattern entries after doubling
constexpr int DASH_NEWTON = 8; // safeguarded Newton steps of an inversion

struct DashPat {
    double pre[DASH_MAX + 1];       // pre[0] = 0, pre[j + 1] = pre[j] + entry j; pre[m] = P
    double P, phase;
    int m, N;                       // entries; on-intervals of non-zero length per period
    int solid;                      // no gap of non-zero length: the stroke is solid
    unsigned char nzp[DASH_MAX + 1]; // nzp[j]: on-intervals of non-zero length among the entries below j
    unsigned char nzj[DASH_MAX / 2]; // entry of the n-th on-interval of non-zero length
};

// `raw`: n >= 1 finite entries >= 0 with a positive sum (the caller has checked), 2 n <= DASH_MAX when n is odd, else n <= DASH_MAX.
// `scale` multiplies the entries and the offset (pathLength).
DASH_HD void dash_build_pattern(const double* raw, int n, double offset, double scale, DashPat& pat) {
    const int m = (n & 1) ? 2 * n : n;
    pat.m = m;
    pat.pre[0] = 0.0;
    int N = 0, gaps = 0;
    for (int j = 0; j < m; ++j) {
        const double e = raw[j % n] * scale;
        pat.pre[j + 1] = pat.pre[j] + e;
        pat.nzp[j] = (unsigned char)N;
        const bool nz = pat.pre[j + 1] > pat.pre[j];
        if (nz && !(j & 1)) pat.nzj[N++] = (unsigned char)j;
        if (nz && (j & 1)) ++gaps;
    }
    pat.nzp[m] = (unsigned char)N;
    for (int j = m + 1; j <= DASH_MAX; ++j) { pat.pre[j] = pat.pre[m]; pat.nzp[j] = (unsigned char)N; }
    pat.N = N;
    pat.solid = gaps == 0;
    pat.P = pat.pre[m];
    const double off = offset * scale;
    double ph = off - std::floor(off / pat.P) * pat.P;
    if (!(ph >= 0.0) || ph >= pat.P) ph = 0.0;
    pat.phase = ph;
}

// interval (k, j) that holds pattern position u: the largest boundary <= u (a boundary belongs to what follows it); r = u - k P
DASH_HD void dash_idx_ge(const DashPat& pat, double u, long long& k, int& j, double& r) {
    double kf = std::floor(u / pat.P);
    r = u - kf * pat.P;
    if (r < 0.0) { kf -= 1.0; r += pat.P; }
    if (r >= pat.P) { kf += 1.0; r -= pat.P; }
    if (!(r >= 0.0)) r = 0.0;
    k = (long long)kf;
    int lo = 0;   // pre[0] = 0 <= r
    for (int step = DASH_MAX / 2; step >= 1; step >>= 1)
        if (lo + step < pat.m && pat.pre[lo + step] <= r) lo += step;
    j = lo;
}
// the last interval that begins in front of u: the largest boundary < u
DASH_HD void dash_idx_lt(const DashPat& pat, double u, long long& k, int& j) {
    double kf = std::floor(u / pat.P);
    double r = u - kf * pat.P;
    if (r < 0.0) { kf -= 1.0; r += pat.P; }
    if (r >= pat.P) { kf += 1.0; r -= pat.P; }
    if (!(r >= 0.0)) r = 0.0;
    k = (long long)kf;
    if (!(r > 0.0)) { k -= 1; j = pat.m - 1; return; }
    int lo = 0;   // pre[0] = 0 < r
    for (int step = DASH_MAX / 2; step >= 1; step >>= 1)
        if (lo + step < pat.m && pat.pre[lo + step] < r) lo += step;
    j = lo;
}
DASH_HD bool dash_is_piece(const DashPat& pat, int j) { return pat.nzp[j + 1] > pat.nzp[j]; }

// ---- the metric
DASH_HD double dash_line_length(const double* q) {
    const double dx = q[2] - q[0], dy = q[3] - q[1];
    return std::sqrt(dx * dx + dy * dy);
}
DASH_HD double dash_speed(const double* c, double t) {   // |B'(t)|
    const double s = 1.0 - t;
    const double a = s * s, b = 2.0 * (s * t), d = t * t;
    const double x = 3.0 * ((a * (c[2] - c[0]) + b * (c[4] - c[2])) + d * (c[6] - c[4]));
    const double y = 3.0 * ((a * (c[3] - c[1]) + b * (c[5] - c[3])) + d * (c[7] - c[5]));
    return std::sqrt(x * x + y * y);
}
DASH_HD double dash_gl4(const double* c, double ta, double tb) {   // length of the cubic over [ta, tb]
    const double x0 = 0.3399810435848563, w0 = 0.6521451548625461, x1 = 0.8611363115940526, w1 = 0.3478548451374538;
    const double h = (tb - ta) * 0.5, mid = (ta + tb) * 0.5;
    const double s0 = dash_speed(c, mid - h * x0) + dash_speed(c, mid + h * x0);
    const double s1 = dash_speed(c, mid - h * x1) + dash_speed(c, mid + h * x1);
    return h * (w0 * s0 + w1 * s1);
}
DASH_HD double dash_sub_length(const double* c, int i) { return dash_gl4(c, (double)i / DASH_SUB, (double)(i + 1) / DASH_SUB); }
// tab[i] = length of the first i + 1 sub-intervals (sequential sum; the kernel scans the same values across lanes)
DASH_HD void dash_cubic_table(const double* c, double* tab) {
    double acc = 0.0;
    for (int i = 0; i < DASH_SUB; ++i) { acc += dash_sub_length(c, i); tab[i] = acc; }
}
// the parameter at arc length s (0 < s < tab[31]) of the cubic: sub-interval from the table, then safeguarded Newton inside it
DASH_HD double dash_invert(const double* c, const double* tab, double s) {
    int i = 0;   // sub-intervals that end at or before s
    for (int step = DASH_SUB / 2; step >= 1; step >>= 1)
        if (tab[i + step - 1] <= s) i += step;
    if (i > DASH_SUB - 1) i = DASH_SUB - 1;
    const double base = i ? tab[i - 1] : 0.0;
    const double rem = s - base, sub = tab[i] - base;
    const double ta = (double)i / DASH_SUB, tb = (double)(i + 1) / DASH_SUB;
    if (!(sub > 0.0) || !(rem > 0.0)) return ta;
    double lo = ta, hi = tb;
    double t = ta + (tb - ta) * (rem / sub);
    if (!(t > lo && t < hi)) t = 0.5 * (lo + hi);
    for (int it = 0; it < DASH_NEWTON; ++it) {
        const double f = dash_gl4(c, ta, t) - rem;
        if (f > 0.0) hi = t; else lo = t;
        double tn = t - f / dash_speed(c, t);
        if (!(tn >= lo && tn <= hi)) tn = 0.5 * (lo + hi);   // (inclusive: a converged step, tn == t == lo or hi, stays)
        t = tn;
    }
    return t;
}
// the restriction of the cubic to [ta, tb] (de Casteljau twice; ta = 0 / tb = 1 keep the end points bit for bit)
DASH_HD void dash_split(const double* c, double ta, double tb, double* o) {
    double p[8];
    for (int i = 0; i < 8; ++i) p[i] = c[i];
    if (tb < 1.0) {   // left part at tb
        for (int a = 0; a < 2; ++a) {
            const double p0 = p[a], p1 = p[2 + a], p2 = p[4 + a], p3 = p[6 + a];
            const double q0 = p0 + (p1 - p0) * tb, q1 = p1 + (p2 - p1) * tb, q2 = p2 + (p3 - p2) * tb;
            const double r0 = q0 + (q1 - q0) * tb, r1 = q1 + (q2 - q1) * tb;
            p[2 + a] = q0; p[4 + a] = r0; p[6 + a] = r0 + (r1 - r0) * tb;
        }
    }
    if (ta > 0.0) {   // right part at ta / tb
        const double u = tb < 1.0 ? ta / tb : ta;
        for (int a = 0; a < 2; ++a) {
            const double p0 = p[a], p1 = p[2 + a], p2 = p[4 + a], p3 = p[6 + a];
            const double q0 = p0 + (p1 - p0) * u, q1 = p1 + (p2 - p1) * u, q2 = p2 + (p3 - p2) * u;
            const double r0 = q0 + (q1 - q0) * u, r1 = q1 + (q2 - q1) * u;
            p[a] = r0 + (r1 - r0) * u; p[2 + a] = r1; p[4 + a] = q2;
        }
    }
    for (int i = 0; i < 8; ++i) o[i] = p[i];
}

// ---- subpaths and segments
enum { DASH_NORMAL = 0, DASH_MERGED = 1, DASH_WHOLE = 2 };
// a closed subpath of length L that begins and ends inside an on-interval: the same interval -> it stays whole (and closed),
// two intervals -> the trailing and the leading dash are one output subpath
DASH_HD int dash_sub_mode(const DashPat& pat, double L, bool closed) {
    if (!closed || !(L > 0.0) || pat.N == 0) return DASH_NORMAL;
    long long k0, k1;
    int j0, j1;
    double r0;
    dash_idx_ge(pat, pat.phase, k0, j0, r0);
    dash_idx_lt(pat, L + pat.phase, k1, j1);
    if (!dash_is_piece(pat, j0) || !dash_is_piece(pat, j1)) return DASH_NORMAL;
    return (k0 == k1 && j0 == j1) ? DASH_WHOLE : DASH_MERGED;
}

struct DashSeg {
    long long c0, cnt;   // ordinal of the first piece among all on-intervals; pieces
    long long ka, kb;    // first and last interval that reach the segment
    int ja, jb;
    int cont;            // the first piece continues a dash that began in front of the segment
    double u0;
};
// a segment of type `type` and length `len` that owns [s0, s1) of a subpath in mode `mode`
DASH_HD void dash_seg_pieces(const DashPat& pat, int type, double len, double s0, double s1, int mode, DashSeg& g) {
    g.c0 = 0; g.cnt = 0; g.cont = 0; g.ka = g.kb = 0; g.ja = g.jb = 0;
    g.u0 = s0 + pat.phase;
    if (!(len > 0.0) || type == 5 /* PATH_UNCLOSED */ || pat.N == 0) return;
    if (mode == DASH_WHOLE) {   // every segment is its own piece; the closing line comes back as the subpath's terminator
        g.cnt = type == 4 /* PATH_CLOSED */ ? 0 : 1;
        g.cont = g.cnt > 0 && s0 != 0.0;
        return;
    }
    double ra;
    dash_idx_ge(pat, g.u0, g.ka, g.ja, ra);
    dash_idx_lt(pat, s1 + pat.phase, g.kb, g.jb);
    g.c0 = g.ka * pat.N + pat.nzp[g.ja];
    const long long c1 = g.kb * pat.N + pat.nzp[g.jb + 1];
    g.cnt = c1 > g.c0 ? c1 - g.c0 : 0;
    if (g.cnt > 0 && dash_is_piece(pat, g.ja))
        g.cont = s0 != 0.0 ? (ra > pat.pre[g.ja]) : (mode == DASH_MERGED);
}
// piece q of the segment: its interval (k, j) and its control points `o` (8 doubles, unused slots 0); returns the output type
DASH_HD int dash_piece(const DashPat& pat, const DashSeg& g, int type, const double* c, const double* tab, double len, int mode,
                       long long q, long long& k, int& j, double* o) {
    const bool cubic = type == 2 /* PATH_CUBIC */;
    if (mode == DASH_WHOLE) {
        k = 0; j = 0;
        for (int i = 0; i < 8; ++i) o[i] = (cubic || i < 4) ? c[i] : 0.0;
        return cubic ? 2 : 0;
    }
    const long long Q = g.c0 + q;
    k = Q / pat.N;
    long long rem = Q - k * pat.N;
    if (rem < 0) { rem += pat.N; k -= 1; }
    j = pat.nzj[rem];
    const bool first = k == g.ka && j == g.ja, last = k == g.kb && j == g.jb;
    const double kP = (double)k * pat.P;
    double la = first ? 0.0 : (kP + pat.pre[j]) - g.u0;
    double lb = last ? len : (kP + pat.pre[j + 1]) - g.u0;
    if (!(la > 0.0)) la = 0.0;
    if (!(lb < len)) lb = len;
    if (cubic) {
        const double ta = la > 0.0 ? dash_invert(c, tab, la) : 0.0;
        const double tb = lb < len ? dash_invert(c, tab, lb) : 1.0;
        dash_split(c, ta, tb, o);
        return 2;
    }
    const double dx = c[2] - c[0], dy = c[3] - c[1];
    o[0] = la > 0.0 ? c[0] + dx * (la / len) : c[0];
    o[1] = la > 0.0 ? c[1] + dy * (la / len) : c[1];
    o[2] = lb < len ? c[0] + dx * (lb / len) : c[2];
    o[3] = lb < len ? c[1] + dy * (lb / len) : c[3];
    o[4] = o[5] = o[6] = o[7] = 0.0;
    return 0;
}
