// svgr_textpath.h -- per-lane arithmetic of text on a path (<textPath>, SVG 1.1 10.13): the frame -- point and unit tangent --
// of a path at an arc length, and the placement of a glyph outline in that frame.
//
// Everything here is plain double arithmetic without a data-dependent loop bound, compilable for the host (the CPU harness
// of tests/textpath_harness.cpp) and for the device (the k_textpath_* kernels of svgr_hip.hip).  DESIGN.md, "Text on a path",
// has the definitions; tests/textpath_ref.py restates them in numpy / long double.
//
//   metric    the dasher's (svgr_dash.h): len[i] of a line is dash_line_length, of a cubic the sum of DASH_SUB sub-intervals of
//             4-point Gauss-Legendre (tab: its 32 running sums); a PATH_UNCLOSED line has length 0, PATH_CLOSED is a line.
//             inc[i] = len[0] + ... + len[i] over the whole path -- a move between subpaths has length 0 -- and L = inc[n - 1];
//             cum[i], the length in front of segment i, is inc[i - 1]
//   locate    the segment of s is the last one of non-zero length with cum[i] <= s: the first i with inc[i] > s; for s = L the
//             last segment that added to the sum, at its end.  (A segment counts as of non-zero length when inc[i] > inc[i - 1].)
//   place     the outline point (x, y) of a glyph with half advance h, shifted by dy across the path, in the frame (P, u)
#pragma once
#include <cmath>
#include <cstdint>

#include "svgr_dash.h"
#include "svgr_marker.h"

#if defined(__HIPCC__)
#define TEXTPATH_HD __host__ __device__ inline
#else
#define TEXTPATH_HD inline
#endif

struct TextFrame { double x, y, ux, uy; };   // point and unit direction of the path at an arc length

// The number of j < n with a[j] <= s (strict: a[j] < s), a ascending: a binary search whose trip count depends on n alone and
// whose loads are clamped instead of skipped.
TEXTPATH_HD int textpath_count(const double* a, int n, double s, bool strict) {
    if (n < 1) return 0;
    int lo = 0;
    for (int step = 1 << (31 - __builtin_clz((unsigned)n)); step >= 1; step >>= 1) {
        const int at = lo + step;
        const double v = a[at <= n ? at - 1 : 0];
        const bool take = at <= n && (strict ? v < s : v <= s);
        lo = take ? at : lo;
    }
    return lo;
}
// The largest k in [0, n) with off[k] <= j (off ascending, off[0] = 0 <= j): the owner of slot j among n ranges, of which the
// empty ones own nothing.
TEXTPATH_HD int textpath_owner(const int* off, int n, int j) {
    if (n < 1) return 0;
    int lo = 0;   // off[lo] <= j
    for (int step = 1 << (31 - __builtin_clz((unsigned)n)); step >= 1; step >>= 1) {
        const int at = lo + step;
        const int v = off[at < n ? at : 0];
        const bool take = at < n && v <= j;
        lo = take ? at : lo;
    }
    return lo;
}

// B(t) of the cubic c by de Casteljau; t <= 0 and t >= 1 give the end points bit for bit.
TEXTPATH_HD void textpath_cubic_point(const double* c, double t, double& x, double& y) {
    if (!(t > 0.0)) { x = c[0]; y = c[1]; return; }
    if (!(t < 1.0)) { x = c[6]; y = c[7]; return; }
    double o[2];
    for (int a = 0; a < 2; ++a) {
        const double p0 = c[a], p1 = c[2 + a], p2 = c[4 + a], p3 = c[6 + a];
        const double q0 = p0 + (p1 - p0) * t, q1 = p1 + (p2 - p1) * t, q2 = p2 + (p3 - p2) * t;
        const double r0 = q0 + (q1 - q0) * t, r1 = q1 + (q2 - q1) * t;
        o[a] = r0 + (r1 - r0) * t;
    }
    x = o[0];
    y = o[1];
}
// B'(t) of the cubic c, in the form dash_speed takes its norm of.
TEXTPATH_HD void textpath_cubic_deriv(const double* c, double t, double& x, double& y) {
    const double s = 1.0 - t;
    const double a = s * s, b = 2.0 * (s * t), d = t * t;
    x = 3.0 * ((a * (c[2] - c[0]) + b * (c[4] - c[2])) + d * (c[6] - c[4]));
    y = 3.0 * ((a * (c[3] - c[1]) + b * (c[5] - c[3])) + d * (c[7] - c[5]));
}

// The frame of segment (type, c) of length len (> 0), r of it from its start (0 <= r <= len); tab: a cubic's 32 running sums.
TEXTPATH_HD void textpath_seg_frame(int type, const double* c, const double* tab, double len, double r, TextFrame& f) {
    f.ux = 1.0;
    f.uy = 0.0;
    if (type != SVGR_PATH_CUBIC) {
        const double dx = c[2] - c[0], dy = c[3] - c[1], q = r / len;
        f.x = c[0] + dx * q;
        f.y = c[1] + dy * q;
        (void)marker_unit(dx, dy, f.ux, f.uy);
        return;
    }
    const double t = !(r > 0.0) ? 0.0 : (!(r < len) ? 1.0 : dash_invert(c, tab, r));
    textpath_cubic_point(c, t, f.x, f.y);
    double dx, dy;
    textpath_cubic_deriv(c, t, dx, dy);
    if (!marker_unit(dx, dy, f.ux, f.uy)) {   // B'(t) = (0, 0) exactly: the segment's direction at its nearer end
        MarkerDirs d{1.0, 0.0, 1.0, 0.0};
        (void)marker_seg_dirs(type, c, d);
        f.ux = t < 0.5 ? d.sx : d.ex;
        f.uy = t < 0.5 ? d.sy : d.ey;
    }
}

// What a locating lane reads: the path (n >= 1 segments), k_dash_measure's lengths and tables, the inclusive sums.
struct TextPathView {
    const int* types;
    const double* params;   // 8 per segment
    const double* len;
    const double* tab;      // DASH_SUB per segment (written for cubics)
    const double* inc;
    int n;
};

// The frame at arc length s (finite); returns inside = 0 <= s <= L.  Outside, s is clamped.  A path with L = 0 has no frame:
// the start of its first segment with the direction (1, 0), inside = 0.
TEXTPATH_HD int textpath_locate(const TextPathView& v, double s, TextFrame& f) {
    const double L = v.inc[v.n - 1];
    if (!(L > 0.0)) {
        f.x = v.params[0]; f.y = v.params[1]; f.ux = 1.0; f.uy = 0.0;
        return 0;
    }
    const int inside = (s >= 0.0 && s <= L) ? 1 : 0;
    const double sc = !(s > 0.0) ? 0.0 : (s > L ? L : s);
    const bool at_end = !(sc < L);
    int i = textpath_count(v.inc, v.n, sc, at_end);
    if (i > v.n - 1) i = v.n - 1;
    const double len = v.len[i];
    double r = at_end ? len : sc - (i ? v.inc[i - 1] : 0.0);
    if (!(r < len)) r = len;
    if (!(r > 0.0)) r = 0.0;
    if (!(len > 0.0)) {   // (only a sum that swallowed a tiny segment gets here)
        f.x = v.params[(size_t)i * 8]; f.y = v.params[(size_t)i * 8 + 1]; f.ux = 1.0; f.uy = 0.0;
        return inside;
    }
    textpath_seg_frame(v.types[i], v.params + (size_t)i * 8, v.tab + (size_t)i * DASH_SUB, len, r, f);
    return inside;
}

// The outline point (x, y) in the frame f: X = Px + ux (x - h) - uy (y + dy), Y = Py + uy (x - h) + ux (y + dy), each as two
// fused multiply-adds in this order -- host and device round alike.
TEXTPATH_HD void textpath_place(const TextFrame& f, double h, double dy, double x, double y, double& X, double& Y) {
    const double a = x - h, b = y + dy;
    X = std::fma(f.ux, a, std::fma(-f.uy, b, f.x));
    Y = std::fma(f.uy, a, std::fma(f.ux, b, f.y));
}

// What an emitting lane reads.
struct TextEmitView {
    const int* atlas_types;
    const double* atlas_params;    // 8 per atlas segment, relative to the glyph's origin
    const int* glyph_seg_off;      // n_glyphs + 1
    const int* inst_glyph;
    const int* inst_off;           // n_inst + 1: prefix sums of the instances' segment counts (host-built)
    const double* inst_half;
    const double* inst_dy;
    const double* frames;          // 4 per instance: x, y, ux, uy
    const int* visible;
    int n_inst, n_atlas;
};

// Output segment j: the instance that owns it, its atlas segment, transformed into o[8] (a line: two points, the rest 0; the
// segments of a hidden instance: all 0).  false when the tables disagree (nothing is written then).
TEXTPATH_HD bool textpath_emit(const TextEmitView& v, int j, double* o) {
    const int k = textpath_owner(v.inst_off, v.n_inst, j);
    const long long a = (long long)v.glyph_seg_off[v.inst_glyph[k]] + (j - v.inst_off[k]);
    if (j < v.inst_off[k] || j >= v.inst_off[k + 1] || a < 0 || a >= v.n_atlas) return false;
    double c[8];
#if defined(__HIP_DEVICE_COMPILE__)
    const double4* rec = reinterpret_cast<const double4*>(v.atlas_params) + (size_t)a * 2;
    const double4 lo = rec[0], hi = rec[1];
    c[0] = lo.x; c[1] = lo.y; c[2] = lo.z; c[3] = lo.w; c[4] = hi.x; c[5] = hi.y; c[6] = hi.z; c[7] = hi.w;
#else
    for (int e = 0; e < 8; ++e) c[e] = v.atlas_params[(size_t)a * 8 + e];
#endif
    TextFrame f;
    marker_load2(v.frames + (size_t)k * 4, f.x, f.y);
    marker_load2(v.frames + (size_t)k * 4 + 2, f.ux, f.uy);
    const int np = !v.visible[k] ? 0 : (v.atlas_types[a] == SVGR_PATH_CUBIC ? 4 : 2);
    const double h = v.inst_half[k], dy = v.inst_dy[k];
    for (int p = 0; p < 4; ++p) {
        double X = 0.0, Y = 0.0;
        if (p < np) textpath_place(f, h, dy, c[2 * p], c[2 * p + 1], X, Y);
        marker_store2(o + 2 * p, X, Y);
    }
    return true;
}
