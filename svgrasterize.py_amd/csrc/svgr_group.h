// svgr_group.h -- per-pixel arithmetic of isolated groups in differentiable compositing: group opacity and clip paths on top of
// svgr_compose.h (solid fills) and svgr_gradpaint.h (gradient fills), forward and backward, and the check of a group program.
//
// Plain double arithmetic for the host (tests/group_harness.cpp) and the device (k_compose_over_program, k_compose_vjp_program of
// svgr_hip.hip), both compiled with -ffp-contract=off.  Nothing here is fused: every product and sum is rounded on its own, in the
// order written.  DESIGN.md 7z has the derivation, tests/group_ref.py restates all of it in numpy.
//
//   program   n_items items in paint order over the planes of cover; the root canvas starts at bg
//               FILL p    the per-path step of the painted compositor on the current canvas (compose_step / gradpaint_step)
//               BEGIN g   push a transparent canvas G = 0
//               END g     pop G;  k = 1 without a clip, else k = m_j0, then k = m_j + k (1 - m_j) over the clip planes in order
//                         (the renderer's one-channel OVER of mask layers, first layer copied);  S_c = (G_c o) k with o the group's
//                         opacity (1 without one): Layer.opacity, then COMPOSE_IN with the mask;  over_px(X, S) on the canvas below
//             every plane is used exactly once, by one FILL or as one clip plane of one group; every opacity slot and every clip by
//             exactly one group; groups nest at most GROUP_DEPTH deep, the root not counted
//   walk 1    last item to first, carries `above`
//               FILL p    through[p] = above;  above = above u_p                         (compose_through / gradpaint_through)
//               END g     T_end[g] = above;  above = 1
//               BEGIN g   P = above;  u_g = 1 - ((1 - P) o) k_g;  above = T_end[g] u_g
//             The group's alpha is the CLOSED FORM 1 - P here, the product of what its members let through, not the forward's
//             rounded sum G_3: the two differ by roundings, as 1 - m a and the forward's s_3 do not.
//   walk 2    first item to last, per level a canvas X and a base adjoint B; the root has X = bg, B = the pixel of grad_image
//               FILL p    compose_vjp_step(X, through[p], B, ...) with B in the place of the image's gradient, then the forward step
//               BEGIN g   g = T_end[g] B,  gc = g . X,  adj = (g_0, g_1, g_2, g_3 - gc);  push X' = 0, B'_c = (adj_c k_g) o
//               END g     q = adj . G;  d / d o = q k_g (summed over the pixels);  d / d k = q o;  clip plane j at position a:
//                         d / d m_j = d / d k (((a == 0) ? 1 : 1 - k_before_j) prod_{i after j} (1 - m_i));  then the forward step
//             adj at END is recomputed from the same three values as at BEGIN (the canvas below does not change in between): the
//             same bits.  Nothing is divided: o = 0, k = 0, an opaque group and an empty group are not special cases.
#pragma once
#include "svgr_core.h"
#include "svgr_compose.h"
#include "svgr_gradpaint.h"

namespace svgr {

constexpr int GROUP_DEPTH = 4;                       // nesting below the root
constexpr int GROUP_MAX_ITEMS = 1 << 24;             // of one program
constexpr int GROUP_FILL = 0, GROUP_BEGIN = 1, GROUP_END = 2;

// one more clip plane on the mask: the first is copied, the others go OVER in one channel
SVGR_HD double group_mask_step(double k, double m, bool first) { return first ? m : m + k * (1.0 - m); }

// the popped group as a source: Layer.opacity, then COMPOSE_IN with the mask
SVGR_HD void group_source(const double* G, double o, double k, double* S) {
    S[0] = (G[0] * o) * k;
    S[1] = (G[1] * o) * k;
    S[2] = (G[2] * o) * k;
    S[3] = (G[3] * o) * k;
}

// the forward step of END: the group onto the canvas below
SVGR_HD void group_step(double* X, const double* G, double o, double k) {
    double S[4];
    group_source(G, o, k, S);
    over_px(X, S[0], S[1], S[2], S[3]);
}

// walk 1 at BEGIN: what the whole group lets through, from the product P of what its members let through
SVGR_HD double group_through(double P, double o, double k) { return 1.0 - ((1.0 - P) * o) * k; }

// walk 2: the adjoint of the group's source S from the canvas X below it, T = T_end[g] and the base adjoint B of that canvas
SVGR_HD void group_adjoint(const double* X, double T, const double* B, double* adj) {
    const double g[4] = {T * B[0], T * B[1], T * B[2], T * B[3]};
    const double gc = compose_dot(g, X);
    adj[0] = g[0];
    adj[1] = g[1];
    adj[2] = g[2];
    adj[3] = g[3] - gc;
}

// walk 2 at BEGIN: the base adjoint of the group's own canvas
SVGR_HD void group_base(const double* adj, double o, double k, double* B) {
    B[0] = (adj[0] * k) * o;
    B[1] = (adj[1] * k) * o;
    B[2] = (adj[2] * k) * o;
    B[3] = (adj[3] * k) * o;
}

// walk 2 at END, clip plane at position a: k_before is the mask of the planes before it, suffix the product of 1 - m_i after it
SVGR_HD double group_clip_vjp(double dk, bool first, double k_before, double suffix) { return dk * ((first ? 1.0 : 1.0 - k_before) * suffix); }

// The check of a program, shared by the entry and the host harness: nullptr, or what is wrong (a static string; `at` gets the item,
// plane, slot or clip it is about).  items is n_items x 4 in the ABI's form: {0, p, 0, 0}, {1, index of its END, 0, 0},
// {2, index of its BEGIN, opacity index or -1, clip index or -1}.  On success dev (n_items x 4) holds the kernels' form: {0, p, 0, 0},
// {1 or 2, g, opacity index or -1, clip index or -1} with g counting the groups in BEGIN order, and n_clips the number of clips.
// seen is scratch of n_paths + n_opacities + n_groups ints.
inline const char* group_program_check(const int32_t* items, int64_t n_items, int64_t n_paths, int64_t n_groups, int64_t n_clip_planes,
                                       int64_t n_opacities, const int32_t* clip_off, const int32_t* clip_planes, int* seen, int* dev, int* n_clips,
                                       long long* at) {
    *at = -1;
    if (n_groups < 0 || n_clip_planes < 0 || n_opacities < 0 || n_items < 1) return "negative counts or no item";
    if (n_opacities > n_groups || n_clip_planes > n_paths) return "more opacities than groups or more clip planes than planes";
    if (n_items != (n_paths - n_clip_planes) + 2 * n_groups) return "n_items is not one FILL per plane that is no clip plane and two items per group";
    if (!items) return "items is NULL";
    int* plane_seen = seen;
    int* op_seen = seen + n_paths;
    int* clip_seen = op_seen + n_opacities;
    for (int64_t j = 0; j < n_paths + n_opacities + n_groups; ++j) seen[j] = 0;
    int stack[GROUP_DEPTH], depth = 0, g_next = 0, clips = 0;
    for (int64_t i = 0; i < n_items; ++i) {
        const int32_t* it = items + 4 * i;
        if (it[0] == GROUP_END && it[3] != -1) ++clips;
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
            if (it[1] <= i || it[1] >= n_items || items[4 * (int64_t)it[1]] != GROUP_END || items[4 * (int64_t)it[1] + 1] != i) return "BEGIN without its END";
            if (depth == GROUP_DEPTH) return "groups nest deeper than svgr_group_depth()";
            if (g_next == n_groups) return "more groups than n_groups";
            const int32_t* e = items + 4 * (int64_t)it[1];
            d[0] = GROUP_BEGIN; d[1] = g_next; d[2] = e[2]; d[3] = e[3];
            stack[depth++] = (int)i;
            ++g_next;
        } else if (it[0] == GROUP_END) {
            if (depth == 0 || stack[depth - 1] != it[1]) return "END does not close the open group";
            --depth;
            const int* b = dev + 4 * (int64_t)it[1];
            if (it[2] != -1) {
                if (it[2] < 0 || it[2] >= n_opacities) return "opacity index out of range";
                if (op_seen[it[2]]++) return "an opacity slot is used twice";
            }
            if (it[3] != -1) {
                if (it[3] < 0 || it[3] >= clips) return "clip index out of range";
                if (clip_seen[it[3]]++) return "a clip is used twice";
            }
            d[0] = GROUP_END; d[1] = b[1]; d[2] = it[2]; d[3] = it[3];
        } else {
            return "unknown op (0 FILL, 1 BEGIN, 2 END)";
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
    return nullptr;
}

}  // namespace svgr
