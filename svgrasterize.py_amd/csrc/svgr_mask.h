// svgr_mask.h -- per-pixel arithmetic of luminance-masked groups in differentiable compositing, on top of svgr_group.h: the value
// of a mask and its derivative, a masked group as a source, and the check of a program that may hold masked pairs.
//
// Plain double arithmetic for the host (tests/mask_harness.cpp) and the device (k_compose_over_program, k_compose_vjp_program of
// svgr_hip.hip), both compiled with -ffp-contract=off.  The two fma calls of mask_value are explicit, as in k_layer_luminance;
// nothing else is fused: every product and sum is rounded on its own, in the order written.  DESIGN.md 7za has the derivation,
// tests/mask_ref.py restates all of it in numpy.
//
//   mask value  M is the premultiplied canvas of the mask group (the renderer: convert to straight alpha, luminance, times alpha)
//                 al = M_3;  r_c = (al > 0.0001) ? M_c / al : M_c  (c < 3);  x_c = clip01(r_c);  a = clip01(al)
//                 lum = fma(x_2, 0.072, fma(x_1, 0.7154, x_0 * 0.2125));  k = lum a
//               derivative, with w = (0.2125, 0.7154, 0.072) and in(v) = 1 on the CLOSED interval 0 <= v <= 1, else 0:
//                 s_c = in(r_c) ? w_c a : 0
//                 d k / d M_c = (al > 0.0001) ? s_c / al : s_c                                                           (c < 3)
//                 d k / d M_3 = (in(al) ? lum : 0) - ((al > 0.0001) ? (((s_0 r_0 + s_1 r_1) + s_2 r_2) / al) : 0)
//               One side at every kink: the threshold takes the forward's branch (al == 0.0001 does not divide); a clip passes
//               the gradient AT 0 and AT 1, so an opaque white mask (x = 1, a = 1) still moves its paint.  The only division is
//               by al where al > 0.0001: nothing is NaN or infinite for a finite M; M = 0 gives k = 0 and d k = (0, 0, 0, 0).
//   program     svgr_group.h's, and a masked PAIR: the target group closed by HOLD instead of END, at once followed by the mask
//               group, which is closed by END_MASK.  Both sit on the same level and may hold anything, pairs included.
//                 HOLD g       pop G;  k_clip and o as at END;  keep H_c = (G_c o) k_clip instead of compositing
//                 END_MASK g'  pop M;  k_mask = mask_value(M);  S_c = H_c k_mask = ((G_c o) k_clip) k_mask: Layer.opacity, COMPOSE_IN
//                              with the clip, COMPOSE_IN with the mask, the loader's MASK(CLIP(OPACITY(GROUP)));  over_px(X, S)
//   walk 0      first item to last, the forward: parks M of every pair (k_mask and d k / d M are needed before M exists in walks
//               1 and 2)
//   walk 1      last item to first
//                 END_MASK     T_end[target] = above;  above = 1
//                 BEGIN (mask) nothing carries over
//                 HOLD         above = 1
//                 BEGIN (held target)  P = above;  u_g = 1 - (((1 - P) o) k_clip) k_mask;  above = T_end[target] u_g
//   walk 2      first item to last
//                 BEGIN (held target)  adj as in svgr_group.h;  push X' = 0, B'_c = ((adj_c k_clip) k_mask) o
//                 HOLD         pop;  adj from the same three values (the same bits);  q = adj . G;  d / d o = (q k_clip) k_mask;
//                              d / d k_clip = (q o) k_mask, to the clip planes as at END;  keep H and qok = (q o) k_clip
//                 BEGIN (mask) push X' = 0, B'_c = qok (d k / d M)_c: the mask's canvas takes this in the place of the image's gradient
//                 END_MASK     pop;  the forward step
//               The mask follows its target because walk 2 needs the target's finished canvas G for q before the mask's fills.
#pragma once
#include <cmath>

#include "svgr_group.h"

namespace svgr {

constexpr int MASK_HOLD = 3, MASK_END = 4;               // the ABI's two ops beside GROUP_FILL, GROUP_BEGIN, GROUP_END
constexpr int MASK_BEGIN_HELD = 5, MASK_BEGIN_MASK = 6;  // the kernels' form only: the BEGIN of a pair's target and of its mask group
constexpr double MASK_ALPHA_MIN = 0.0001;

// the kernels' form keeps the pair's number above the op: x = op | pair << 3
SVGR_HD int mask_op(int x) { return x & 7; }
SVGR_HD int mask_pair(int x) { return x >> 3; }

SVGR_HD double mask_clip01(double x) { return x < 0 ? 0 : (x > 1 ? 1 : x); }
SVGR_HD bool mask_in01(double x) { return x >= 0 && x <= 1; }

SVGR_HD double mask_value(const double* M) {
    const double al = M[3];
    const bool divide = al > MASK_ALPHA_MIN;
    const double x0 = mask_clip01(divide ? M[0] / al : M[0]);
    const double x1 = mask_clip01(divide ? M[1] / al : M[1]);
    const double x2 = mask_clip01(divide ? M[2] / al : M[2]);
    const double lum = fma(x2, 0.072, fma(x1, 0.7154, x0 * 0.2125));
    return lum * mask_clip01(al);
}

// d k / d M into dM[4]
SVGR_HD void mask_value_vjp(const double* M, double* dM) {
    const double al = M[3];
    const bool divide = al > MASK_ALPHA_MIN;
    const double r0 = divide ? M[0] / al : M[0];
    const double r1 = divide ? M[1] / al : M[1];
    const double r2 = divide ? M[2] / al : M[2];
    const double lum = fma(mask_clip01(r2), 0.072, fma(mask_clip01(r1), 0.7154, mask_clip01(r0) * 0.2125));
    const double a = mask_clip01(al);
    const double s0 = mask_in01(r0) ? 0.2125 * a : 0.0;
    const double s1 = mask_in01(r1) ? 0.7154 * a : 0.0;
    const double s2 = mask_in01(r2) ? 0.072 * a : 0.0;
    const double top = mask_in01(al) ? lum : 0.0;
    if (divide) {
        dM[0] = s0 / al;
        dM[1] = s1 / al;
        dM[2] = s2 / al;
        dM[3] = top - ((s0 * r0 + s1 * r1) + s2 * r2) / al;
    } else {
        dM[0] = s0;
        dM[1] = s1;
        dM[2] = s2;
        dM[3] = top;
    }
}

// HOLD: the popped target with its opacity and clip, kept until its mask is known
SVGR_HD void mask_hold(const double* G, double o, double k_clip, double* H) { group_source(G, o, k_clip, H); }

// END_MASK: the held group through its mask onto the canvas below
SVGR_HD void mask_step(double* X, const double* H, double k_mask) {
    over_px(X, H[0] * k_mask, H[1] * k_mask, H[2] * k_mask, H[3] * k_mask);
}

// walk 1 at the BEGIN of a held target
SVGR_HD double mask_through(double P, double o, double k_clip, double k_mask) { return 1.0 - (((1.0 - P) * o) * k_clip) * k_mask; }

// walk 2 at the BEGIN of a held target: the base adjoint of the target's canvas
SVGR_HD void mask_base(const double* adj, double o, double k_clip, double k_mask, double* B) {
    B[0] = ((adj[0] * k_clip) * k_mask) * o;
    B[1] = ((adj[1] * k_clip) * k_mask) * o;
    B[2] = ((adj[2] * k_clip) * k_mask) * o;
    B[3] = ((adj[3] * k_clip) * k_mask) * o;
}

// walk 2 at HOLD, from q = adj . G
SVGR_HD double mask_opacity_term(double q, double k_clip, double k_mask) { return (q * k_clip) * k_mask; }
SVGR_HD double mask_clip_term(double q, double o, double k_mask) { return (q * o) * k_mask; }
SVGR_HD double mask_held_dot(double q, double o, double k_clip) { return (q * o) * k_clip; }

// walk 2 at the BEGIN of a mask group: the base adjoint of the mask's canvas
SVGR_HD void mask_base_of_mask(double qok, const double* M, double* B) {
    double dM[4];
    mask_value_vjp(M, dM);
    B[0] = qok * dM[0];
    B[1] = qok * dM[1];
    B[2] = qok * dM[2];
    B[3] = qok * dM[3];
}

// The check of a program that may hold masked pairs, shared by the entry and the host harness, in group_program_check's form:
// nullptr, or what is wrong (a static string; `at` gets the item, plane, slot or clip it is about).  items is n_items x 4 in the
// ABI's form: group_program_check's three, {1, index of its closer, 0, 0} with the closer an END, a HOLD or an END_MASK,
// {3, index of its BEGIN, opacity index or -1, clip index or -1} and {4, index of its BEGIN, 0, 0}.  A HOLD at item i is followed
// at i + 1 by the BEGIN of a group closed by END_MASK, and only such a BEGIN is closed by END_MASK.  On success dev holds the
// kernels' form: group_program_check's for FILL, BEGIN and END (a program without pairs gives its table), and for a pair number n
// {5 | n << 3, g, opacity, clip} the target's BEGIN, {3 | n << 3, g, opacity, clip} its HOLD, {6 | n << 3, g', g, 0} the mask
// group's BEGIN and {4 | n << 3, g', g, 0} its END_MASK, with pairs numbered as their targets open.  seen is scratch of
// n_paths + n_opacities + n_groups ints; last_mask gets the index of the last END_MASK, or -1.
inline const char* mask_program_check(const int32_t* items, int64_t n_items, int64_t n_paths, int64_t n_groups, int64_t n_clip_planes,
                                      int64_t n_opacities, const int32_t* clip_off, const int32_t* clip_planes, int* seen, int* dev, int* n_clips,
                                      int* n_pairs, int* last_mask, long long* at) {
    *at = -1;
    if (n_groups < 0 || n_clip_planes < 0 || n_opacities < 0 || n_items < 1) return "negative counts or no item";
    if (n_opacities > n_groups || n_clip_planes > n_paths) return "more opacities than groups or more clip planes than planes";
    if (n_items != (n_paths - n_clip_planes) + 2 * n_groups) return "n_items is not one FILL per plane that is no clip plane and two items per group";
    if (!items) return "items is NULL";
    int* plane_seen = seen;
    int* op_seen = seen + n_paths;
    int* clip_seen = op_seen + n_opacities;
    for (int64_t j = 0; j < n_paths + n_opacities + n_groups; ++j) seen[j] = 0;
    int stack[GROUP_DEPTH], depth = 0, g_next = 0, clips = 0, pairs = 0, last = -1;
    for (int64_t i = 0; i < n_items; ++i) {
        const int32_t* it = items + 4 * i;
        if ((it[0] == GROUP_END || it[0] == MASK_HOLD) && it[3] != -1) ++clips;
    }
    if (clips > 0 && (!clip_off || !clip_planes)) return "clip_off or clip_planes is NULL";
    if (clips == 0 && n_clip_planes != 0) return "clip planes without a clip";
    for (int64_t i = 0; i < n_items; ++i) {
        const int32_t* it = items + 4 * i;
        int* d = dev + 4 * i;
        *at = i;
        if (it[0] == GROUP_FILL) {
            if (it[1] < 0 || it[1] >= n_paths) return "FILL of a plane out of range";
            if (plane_seen[it[1]]++) return "a plane is used twice";
            d[0] = GROUP_FILL; d[1] = it[1]; d[2] = 0; d[3] = 0;
        } else if (it[0] == GROUP_BEGIN) {
            if (it[1] <= i || it[1] >= n_items || items[4 * (int64_t)it[1] + 1] != i) return "BEGIN without its closer";
            const int32_t* e = items + 4 * (int64_t)it[1];
            if (e[0] != GROUP_END && e[0] != MASK_HOLD && e[0] != MASK_END) return "BEGIN without its closer";
            const bool after_hold = i > 0 && items[4 * (i - 1)] == MASK_HOLD;
            if (e[0] == MASK_END && !after_hold) return "an END_MASK whose BEGIN does not follow a HOLD";
            if (e[0] != MASK_END && after_hold) return "a HOLD is not followed by the BEGIN of a mask group";
            if (e[0] == MASK_HOLD) {
                if ((int64_t)it[1] + 1 >= n_items) return "a HOLD is the last item";
                if (items[4 * ((int64_t)it[1] + 1)] != GROUP_BEGIN) return "a HOLD is not followed by the BEGIN of a mask group";
            }
            if (depth == GROUP_DEPTH) return "groups nest deeper than svgr_group_depth()";
            if (g_next == n_groups) return "more groups than n_groups";
            if (e[0] == GROUP_END) {
                d[0] = GROUP_BEGIN; d[1] = g_next; d[2] = e[2]; d[3] = e[3];
            } else if (e[0] == MASK_HOLD) {
                d[0] = MASK_BEGIN_HELD | (pairs << 3); d[1] = g_next; d[2] = e[2]; d[3] = e[3];
                ++pairs;
            } else {   // (the HOLD before it is checked: it closed the open group, whose BEGIN holds the pair)
                const int* h = dev + 4 * (i - 1);
                d[0] = MASK_BEGIN_MASK | (mask_pair(h[0]) << 3); d[1] = g_next; d[2] = h[1]; d[3] = 0;
            }
            stack[depth++] = (int)i;
            ++g_next;
        } else if (it[0] == GROUP_END || it[0] == MASK_HOLD) {
            if (depth == 0 || stack[depth - 1] != it[1]) return it[0] == GROUP_END ? "END does not close the open group" : "HOLD does not close the open group";
            const int* b = dev + 4 * (int64_t)it[1];
            if ((mask_op(b[0]) == GROUP_BEGIN) != (it[0] == GROUP_END) || mask_op(b[0]) == MASK_BEGIN_MASK) return "a group is closed by another op than its BEGIN names";
            --depth;
            if (it[0] == MASK_HOLD && i + 1 >= n_items) return "a HOLD is the last item";
            if (it[2] != -1) {
                if (it[2] < 0 || it[2] >= n_opacities) return "opacity index out of range";
                if (op_seen[it[2]]++) return "an opacity slot is used twice";
            }
            if (it[3] != -1) {
                if (it[3] < 0 || it[3] >= clips) return "clip index out of range";
                if (clip_seen[it[3]]++) return "a clip is used twice";
            }
            d[0] = it[0] == GROUP_END ? GROUP_END : (MASK_HOLD | (mask_pair(b[0]) << 3));
            d[1] = b[1]; d[2] = it[2]; d[3] = it[3];
        } else if (it[0] == MASK_END) {
            if (depth == 0 || stack[depth - 1] != it[1]) return "END_MASK does not close the open group";
            const int* b = dev + 4 * (int64_t)it[1];
            if (mask_op(b[0]) != MASK_BEGIN_MASK) return "a group is closed by another op than its BEGIN names";
            --depth;
            d[0] = MASK_END | (mask_pair(b[0]) << 3); d[1] = b[1]; d[2] = b[2]; d[3] = 0;
            last = (int)i;
        } else {
            return "unknown op (0 FILL, 1 BEGIN, 2 END, 3 HOLD, 4 END_MASK)";
        }
    }
    *at = -1;
    if (depth != 0) return "a group is not closed";
    if (g_next != n_groups) return "fewer groups than n_groups";
    for (int64_t j = 0; j < n_opacities; ++j)
        if (!op_seen[j]) { *at = j; return "an opacity slot is not used"; }
    if (clips) {
        if (clip_off[0] != 0 || (int64_t)clip_off[clips] != n_clip_planes) return "clip_off does not go from 0 to n_clip_planes";
        for (int c = 0; c < clips; ++c) {
            *at = c;
            if (clip_off[c + 1] <= clip_off[c]) return "a clip without a plane, or clip_off decreases";
            if ((int64_t)clip_off[c + 1] > n_clip_planes) return "clip_off beyond n_clip_planes";
        }
        for (int64_t j = 0; j < n_clip_planes; ++j) {
            *at = j;
            if (clip_planes[j] < 0 || clip_planes[j] >= n_paths) return "clip plane out of range";
            if (plane_seen[clip_planes[j]]++) return "a plane is used twice";
        }
    }
    for (int64_t p = 0; p < n_paths; ++p)
        if (!plane_seen[p]) { *at = p; return "a plane is not used"; }
    *at = -1;
    *n_clips = clips;
    *n_pairs = pairs;
    *last_mask = last;
    return nullptr;
}

}  // namespace svgr
