// svgr_hit.h -- per-lane arithmetic of hit testing: is a point inside a path (SVG DOM isPointInFill / isPointInStroke), and which
// path of a paint-ordered list is the topmost one under it (elementFromPoint).
//
// Everything here is plain double / integer arithmetic, compilable for the host (the CPU harness of tests/hit_harness.cpp) and for
// the device (k_hit_winding and k_hit_resolve of svgr_hip.hip).  Both sides are compiled with -ffp-contract=off: no product below
// is fused into a sum.  DESIGN.md 7q has the definitions; tests/hit_ref.py restates them in numpy.
//
//   edge      a flattened edge (a0, b0) -> (a1, b1) in presentation space: `a` is the first coordinate of an edge as
//             svgr_batch_all_edges stores it (the row), `b` the second (the column); a point (pa, pb) is given in the same order.
//             The ray runs from the point towards +a.
//   term      up   = b0 <= pb && b1 > pb,   down = b1 <= pb && b0 > pb          (an edge with b0 == b1 is neither)
//             d    = (a1 - a0) * (pb - b0) - (pa - a0) * (b1 - b0)              (two products rounded apart, then subtracted)
//             +1 if up && d > 0,  -1 if down && d < 0,  else 0
//             A vertex belongs to exactly one of its two edges (half-open in b).  A point with a NaN or infinite coordinate
//             gets 0 from every edge: it is outside, which is no error.
//   winding   the sum of the terms over a path's edges: an integer, so it does not depend on the order of summation, and the
//             device's sum equals the host's exactly.  inside = w != 0 (nonzero) or w & 1 (even-odd).
//   contract  the edges are those the renderer itself flattens under the given transform and flatness, so "inside" agrees with
//             what is drawn.  A point within rounding distance of an edge may fall either way -- d is two rounded products --
//             but it falls the same way on the host and on the device and from run to run.
//   resolve   paths 0 .. n-1 in paint order; path p has clip groups clip_group[clip_off[p] .. clip_off[p + 1]), group g has the
//             sources group_src[group_off[g] .. group_off[g + 1]), every one of them a path in front of p (smaller index):
//               pass(p) = inside(p) && for every clip group g of p: (exists s in g: pass(s))
//             evaluated for p = 0 .. n-1 in increasing order, in place over the point's row of bits (32 paths to a word);
//               top = the largest p with pickable[p] && pass(p), or -1
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HIT_HD __host__ __device__ inline
#else
#define HIT_HD inline
#endif

constexpr int HIT_BLOCK = 256;   // points per workgroup of k_hit_winding (a 16 x 16 pixel tile of a grid query)
constexpr int HIT_TILE = 16;
constexpr int HIT_CHUNK = 256;   // edges of a path staged through LDS at a time (8 KiB)
static_assert(HIT_TILE * HIT_TILE == HIT_BLOCK, "a workgroup of a grid query is one square tile");

// the box of a workgroup's finite points, lo <= hi in a and in b, and their smallest |pb|; without a finite point lo = +inf,
// hi = -inf and min_absb = +inf (what the point queries' culls test a path's extent against)
struct HitBox {
    double lo_a, hi_a, lo_b, hi_b, min_absb;
};

// x - x is 0 for a finite x and NaN for NaN and +-inf
HIT_HD bool hit_finite(double pa, double pb) { return (pa - pa == 0.0) && (pb - pb == 0.0); }

// the term of one edge for a FINITE point (the callers sort the other points out once, not per edge)
HIT_HD int hit_edge_term(double a0, double b0, double a1, double b1, double pa, double pb) {
    const bool up = (b0 <= pb) && (b1 > pb), down = (b1 <= pb) && (b0 > pb);
    const double m0 = (a1 - a0) * (pb - b0), m1 = (pa - a0) * (b1 - b0);
    const double d = m0 - m1;
    return (up && d > 0.0) ? 1 : (down && d < 0.0) ? -1 : 0;
}

// winding number of `n` edges (4 doubles each) at one point
HIT_HD int hit_winding(const double* edges, long long n, double pa, double pb) {
    if (!hit_finite(pa, pb)) return 0;
    int w = 0;
    for (long long e = 0; e < n; ++e) w += hit_edge_term(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], pa, pb);
    return w;
}

HIT_HD bool hit_inside(int w, int evenodd) { return evenodd ? (w & 1) != 0 : w != 0; }

// The clip tables are usable: offsets ascend from 0, every group index is in range and every source of a path's group lies in
// front of the path.  0, or 1 + the first path whose tables are not (host only: the C entry's check before any launch).
inline long long hit_check_tables(long long n_paths, const int32_t* clip_off, const int32_t* clip_group, const int32_t* group_off,
                                  const int32_t* group_src, long long n_groups) {
    if (n_groups > 0 && group_off[0] != 0) return 1;
    for (long long g = 0; g < n_groups; ++g)
        if (group_off[g + 1] < group_off[g]) return 1;
    if (n_paths > 0 && clip_off[0] != 0) return 1;
    for (long long p = 0; p < n_paths; ++p) {
        if (clip_off[p + 1] < clip_off[p]) return p + 1;
        for (int k = clip_off[p]; k < clip_off[p + 1]; ++k) {
            const int g = clip_group[k];
            if (g < 0 || g >= n_groups) return p + 1;
            for (int j = group_off[g]; j < group_off[g + 1]; ++j)
                if (group_src[j] < 0 || group_src[j] >= p) return p + 1;
        }
    }
    return 0;
}

// One point's row: `row` holds inside bits on entry and pass bits on return; returns top.
HIT_HD int hit_resolve(uint32_t* row, int n_paths, const uint8_t* pickable, const int32_t* clip_off, const int32_t* clip_group,
                       const int32_t* group_off, const int32_t* group_src) {
    int top = -1;
    for (int w0 = 0; w0 < n_paths; w0 += 32) {
        uint32_t word = row[w0 >> 5];
        const int end = n_paths - w0 < 32 ? n_paths - w0 : 32;
        for (int k = 0; k < end; ++k) {
            if (!((word >> k) & 1u)) continue;
            const int p = w0 + k;
            bool pass = true;
            for (int c = clip_off[p]; pass && c < clip_off[p + 1]; ++c) {
                const int g = clip_group[c];
                bool any = false;
                for (int j = group_off[g]; !any && j < group_off[g + 1]; ++j) {
                    const int s = group_src[j];
                    // (s < p: a source in this word has been resolved into `word` already, one in an earlier word into the row)
                    const uint32_t sw = (s >> 5) == (w0 >> 5) ? word : row[s >> 5];
                    any = (sw >> (s & 31)) & 1u;
                }
                pass = any;
            }
            if (!pass) word &= ~(1u << k);
            else if (pickable[p]) top = p;
        }
        row[w0 >> 5] = word;
    }
    return top;
}
