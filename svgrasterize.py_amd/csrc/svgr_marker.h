// svgr_marker.h -- per-lane arithmetic of the marker vertex pass (marker-start / -mid / -end, SVG 2 11.6; the directions are the
// path implementation notes of SVG 1.1 F.5).
//
// Everything here is plain double arithmetic without a data-dependent loop bound, compilable for the host (the CPU harness
// of tests/marker_harness.cpp) and for the device (the k_marker_* kernels of svgr_hip.hip).  DESIGN.md, "Markers", has the
// definitions; tests/marker_ref.py restates them in numpy / long double.
//
//   outline   the segments of a subpath but a trailing PATH_UNCLOSED line; PATH_CLOSED (and a PATH_UNCLOSED that is not the last
//             segment) is a line.  A subpath is closed when its last segment is PATH_CLOSED.
//   classify  per segment: the unit directions at its start and its end (MarkerDirs) and its flags -- in the outline, ends at a
//             vertex, has a direction of its own (not degenerate)
//   tables    cnt[i] = (segments with a direction, vertices) up to and with segment i over the whole path (an inclusive sum
//             scan); tab[k] = the k-th segment with a direction.  A degenerate segment i finds its neighbours at
//             tab[cnt[i].nd - 1] (earlier) and tab[cnt[i].nd] (later) and takes them only from its own subpath
//   emit      per segment: the first segment of a subpath emits the subpath's first vertex at the slot in front of its own, every
//             vertex-flagged segment emits its end point at slot cnt[i].v - 1
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/svgr.h"

#if defined(__HIPCC__)
#define MARKER_HD __host__ __device__ inline
#else
#define MARKER_HD inline
#endif

constexpr int MARKER_F_DIR = 1;       // the segment has a direction of its own
constexpr int MARKER_F_VERTEX = 2;    // its end point is a vertex of the author's path
constexpr int MARKER_F_OUTLINE = 4;   // it is part of the outline
constexpr int MARKER_START = 0, MARKER_MID = 1, MARKER_END = 2;
// u_in + u_out counts as cancelled -- the path turns back on itself -- when neither component exceeds 2^-40 in magnitude: two
// unit vectors of a few ulp error each leave their sum uncertain by ~1e-15, so that above 9.1e-13 the bisector is still good to
// three digits, and below it u_in turned by +90 degrees is the better answer.
constexpr double MARKER_CANCEL = 9.094947017729282e-13;

struct MarkerDirs { double sx, sy, ex, ey; };   // unit direction at the start and at the end of a segment
struct MarkerCnt { long long nd, v; };          // segments with a direction, vertices

// (dx, dy) / |(dx, dy)|, scaled by the larger component first: neither 1e-170 nor 1e150 leaves the doubles when squared.
// false, and nothing written, for exactly (0, 0).
MARKER_HD bool marker_unit(double dx, double dy, double& ux, double& uy) {
    const double m = std::fmax(std::fabs(dx), std::fabs(dy));
    if (!(m > 0.0)) return false;
    const double x = dx / m, y = dy / m;
    const double h = std::sqrt(x * x + y * y);
    ux = x / h;
    uy = y / h;
    return true;
}

// The directions of one segment (c: its 8 doubles); false for a degenerate one (d is then not written).  Line: P1 - P0 at both
// ends.  Cubic, start: the first of P1 - P0, P2 - P0, P3 - P0 that is not (0, 0); end: the first of P3 - P2, P3 - P1, P3 - P0.
MARKER_HD bool marker_seg_dirs(int type, const double* c, MarkerDirs& d) {
    if (type != SVGR_PATH_CUBIC) {
        if (!marker_unit(c[2] - c[0], c[3] - c[1], d.sx, d.sy)) return false;
        d.ex = d.sx;
        d.ey = d.sy;
        return true;
    }
    if (!(marker_unit(c[2] - c[0], c[3] - c[1], d.sx, d.sy) || marker_unit(c[4] - c[0], c[5] - c[1], d.sx, d.sy) ||
          marker_unit(c[6] - c[0], c[7] - c[1], d.sx, d.sy)))
        return false;
    // (some point differs from P0, so one of these differs from P3)
    (void)(marker_unit(c[6] - c[4], c[7] - c[5], d.ex, d.ey) || marker_unit(c[6] - c[2], c[7] - c[3], d.ex, d.ey) ||
           marker_unit(c[6] - c[0], c[7] - c[1], d.ex, d.ey));
    return true;
}

// The mid-vertex rule: normalise(u_in + u_out); a reversal gives u_in turned by +90 degrees.
MARKER_HD void marker_bisect(double ix, double iy, double ox, double oy, double& ux, double& uy) {
    const double sx = ix + ox, sy = iy + oy;
    if (std::fmax(std::fabs(sx), std::fabs(sy)) <= MARKER_CANCEL) {
        ux = -iy;
        uy = ix;
        return;
    }
    (void)marker_unit(sx, sy, ux, uy);
}

// two adjacent doubles in one load (p: 16-byte aligned on the device)
MARKER_HD void marker_load2(const double* p, double& a, double& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double2 t = *reinterpret_cast<const double2*>(p);
    a = t.x;
    b = t.y;
#else
    a = p[0];
    b = p[1];
#endif
}

MARKER_HD void marker_store2(double* p, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<double2*>(p) = make_double2(a, b);
#else
    p[0] = a;
    p[1] = b;
#endif
}

// What the emitting lanes read.
struct MarkerView {
    const int* types;
    const double* params;      // 8 per segment
    const int* seg_sub;        // subpath of every segment (empty subpaths are not counted)
    const int* sub_off;        // first segment of every subpath, n_sub + 1 entries
    const int* flags;          // MARKER_F_*
    const MarkerDirs* dirs;    // written where MARKER_F_DIR is set
    const MarkerCnt* cnt;      // inclusive scan
    const int* tab;            // tab[k]: the k-th segment with MARKER_F_DIR
    int n;
};

// Flags and vertex count of segment i: the counts of its row of the scan.
MARKER_HD int marker_classify(const int* types, const int* seg_sub, const int* sub_off, const int* seg_vertex, int i, const double* c,
                              MarkerDirs& d, MarkerCnt& row) {
    const int sp = seg_sub[i], first = sub_off[sp], last = sub_off[sp + 1] - 1;
    int f = 0;
    row.nd = row.v = 0;
    if (i == last && types[i] == SVGR_PATH_UNCLOSED) return 0;   // not part of the outline
    f = MARKER_F_OUTLINE;
    if (marker_seg_dirs(types[i], c, d)) { f |= MARKER_F_DIR; row.nd = 1; }
    if (!seg_vertex || seg_vertex[i]) { f |= MARKER_F_VERTEX; row.v = 1; }
    if (i == first) row.v += 1;   // the subpath's first vertex
    return f;
}

// Direction of segment j (a segment of the outline of the subpath [first, last_o]) at its start (end = false) or its end: its
// own, or for a degenerate one the end direction of the nearest earlier segment of the subpath that has one, failing that the start
// direction of the nearest later one, failing that (1, 0).
MARKER_HD void marker_resolved(const MarkerView& v, int j, int first, int last_o, bool end, double& ux, double& uy) {
    if (v.flags[j] & MARKER_F_DIR) {
        marker_load2(end ? &v.dirs[j].ex : &v.dirs[j].sx, ux, uy);
        return;
    }
    const long long k = v.cnt[j].nd, total = v.cnt[v.n - 1].nd;   // k segments with a direction lie in front of j
    if (k > 0) {
        const int e = v.tab[k - 1];
        if (e >= first) { marker_load2(&v.dirs[e].ex, ux, uy); return; }
    }
    if (k < total) {
        const int l = v.tab[k];
        if (l <= last_o) { marker_load2(&v.dirs[l].sx, ux, uy); return; }
    }
    ux = 1.0;
    uy = 0.0;
}

// The vertices segment i emits (none, one or two), written at their slots: xyuv[4 * slot] = x, y, ux, uy; kind[slot].  Returns
// false when a slot lies outside [0, n_vert): the tables disagree, nothing is written there.
MARKER_HD bool marker_emit(const MarkerView& v, int i, long long n_vert, double* xyuv, int* kind) {
    const int f = v.flags[i];
    if (!(f & MARKER_F_OUTLINE)) return true;
    const int sp = v.seg_sub[i], first = v.sub_off[sp], last = v.sub_off[sp + 1] - 1;
    const int t_last = v.types[last];
    const int last_o = last - (t_last == SVGR_PATH_UNCLOSED ? 1 : 0);
    const bool closed = t_last == SVGR_PATH_CLOSED;
    bool ok = true;
    for (int which = 0; which < 2; ++which) {   // 0: the subpath's first vertex; 1: this segment's end point
        if (which == 0 ? i != first : !(f & MARKER_F_VERTEX)) continue;
        const long long slot = which == 0 ? (i ? v.cnt[i - 1].v : 0) : v.cnt[i].v - 1;
        if (slot < 0 || slot >= n_vert) { ok = false; continue; }
        const double* c = v.params + (size_t)i * 8;
        double x, y, ix, iy, ox, oy, ux, uy;
        marker_load2(which == 0 ? c : (v.types[i] == SVGR_PATH_CUBIC ? c + 6 : c + 2), x, y);
        const bool at_end = which == 0 || i == last_o;   // an end vertex of the subpath
        if (at_end && !closed) {
            if (which == 0) marker_resolved(v, first, first, last_o, false, ux, uy);
            else marker_resolved(v, last_o, first, last_o, true, ux, uy);
        } else {
            marker_resolved(v, at_end ? last_o : i, first, last_o, true, ix, iy);
            marker_resolved(v, at_end ? first : i + 1, first, last_o, false, ox, oy);
            marker_bisect(ix, iy, ox, oy, ux, uy);
        }
        double* o = xyuv + (size_t)slot * 4;
        marker_store2(o, x, y);
        marker_store2(o + 2, ux, uy);
        kind[slot] = slot == 0 ? MARKER_START : (slot == n_vert - 1 ? MARKER_END : MARKER_MID);
    }
    return ok;
}
