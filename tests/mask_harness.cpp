// mask_harness.cpp -- the mask header (csrc/svgr_mask.h) compiled for the host, for tests/test_mask_host.py
// (g++ -ffp-contract=off): what the lanes of k_compose_over_masked and k_compose_vjp_masked do, one pixel after the other.
// Planes, images and gradients are doubles: a float plane widens exactly, and the device rounds once at its stores.  desc is
// n_paths x 4 ints {kind, spread, first stop, end stop}; view is {row0, col0, cols}; items is the kernels' form that mkh_check
// makes of the ABI's.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_mask.h"

using namespace svgr;

namespace {

struct Scene {
    const double *cover, *paints;
    const int* desc;
    const double *m6, *geom, *pos, *rgba;
    const long long* view;
    const int *items, *clip_off, *clip_planes;
    const double* opacity;
    long long n_px;
};

double mask_of(const Scene& s, int clip, long long i) {
    if (clip < 0) return 1.0;
    double k = 0.0;
    for (int a = s.clip_off[clip]; a < s.clip_off[clip + 1]; ++a)
        k = group_mask_step(k, s.cover[(size_t)s.clip_planes[a] * s.n_px + i], a == s.clip_off[clip]);
    return k;
}

double opacity_of(const Scene& s, int slot) { return slot < 0 ? 1.0 : s.opacity[slot]; }

// the colour of a gradient path at pixel i; false for a solid path
bool colour_of(const Scene& s, int p, long long i, double* col, GradPaintPx& e) {
    const int* d = s.desc + 4 * (size_t)p;
    if (d[0] == 0) return false;
    gradpaint_colour(d[0], d[1], s.m6 + 6 * (size_t)p, s.geom + 4 * (size_t)p, d[3] - d[2], s.pos + d[2], s.rgba + 4 * (size_t)d[2], i / s.view[2],
                     i % s.view[2], s.view[0], s.view[1], col, e);
    return true;
}

// the forward of pixel i over items[0 .. n_run) on the root canvas X0; park (n_pairs x 4), if not null, gets M of every pair
void forward_px(const Scene& s, int n_run, long long i, double* X0, double* park) {
    double X[GROUP_DEPTH + 1][4], H[GROUP_DEPTH][4];
    for (int k = 0; k < 4; ++k) X[0][k] = X0[k];
    int level = 0;
    for (int q = 0; q < n_run; ++q) {
        const int* it = s.items + 4 * (size_t)q;
        const int op = mask_op(it[0]);
        if (op == GROUP_FILL) {
            const int p = it[1];
            const double m = s.cover[(size_t)p * s.n_px + i];
            double col[4];
            GradPaintPx e;
            if (colour_of(s, p, i, col, e)) gradpaint_step(X[level], m, col, s.paints + 4 * (size_t)p);
            else compose_step(X[level], m, s.paints + 4 * (size_t)p);
        } else if (op == GROUP_BEGIN || op == MASK_BEGIN_HELD || op == MASK_BEGIN_MASK) {
            ++level;
            for (int k = 0; k < 4; ++k) X[level][k] = 0.0;
        } else if (op == GROUP_END) {
            --level;
            group_step(X[level], X[level + 1], opacity_of(s, it[2]), mask_of(s, it[3], i));
        } else if (op == MASK_HOLD) {
            --level;
            mask_hold(X[level + 1], opacity_of(s, it[2]), mask_of(s, it[3], i), H[level]);
        } else {
            --level;
            const double* M = X[level + 1];
            if (park)
                for (int k = 0; k < 4; ++k) park[4 * (size_t)mask_pair(it[0]) + k] = M[k];
            mask_step(X[level], H[level], mask_value(M));
        }
    }
    for (int k = 0; k < 4; ++k) X0[k] = X[0][k];
}

}  // namespace

extern "C" {

int mkh_depth() { return GROUP_DEPTH; }

double mkh_value(const double* M) { return mask_value(M); }

void mkh_value_vjp(const double* M, double* dM) { mask_value_vjp(M, dM); }

// mask_program_check: nullptr or what is wrong; dev is n_items x 4, info {n_clips, at, n_pairs, last END_MASK}
const char* mkh_check(const int32_t* items, long long n_items, long long n_paths, long long n_groups, long long n_clip_planes, long long n_opacities,
                      const int32_t* clip_off, const int32_t* clip_planes, int* dev, long long* info) {
    std::vector<int> seen((size_t)(n_paths > 0 ? n_paths : 0) + (size_t)(n_opacities > 0 ? n_opacities : 0) + (size_t)(n_groups > 0 ? n_groups : 0) + 1);
    int n_clips = 0, n_pairs = 0, last = -1;
    long long at = -1;
    const char* msg = mask_program_check(items, n_items, n_paths, n_groups, n_clip_planes, n_opacities, clip_off, clip_planes, seen.data(), dev, &n_clips,
                                         &n_pairs, &last, &at);
    info[0] = n_clips;
    info[1] = at;
    info[2] = n_pairs;
    info[3] = last;
    return msg;
}

void mkh_forward(const double* cover, const double* paints, const int* desc, const double* m6, const double* geom, const double* pos,
                 const double* rgba, const double* bg, const long long* view, const int* items, int n_items, const int* clip_off,
                 const int* clip_planes, const double* opacity, long long n_px, double* image) {
    const Scene s = {cover, paints, desc, m6, geom, pos, rgba, view, items, clip_off, clip_planes, opacity, n_px};
    for (long long i = 0; i < n_px; ++i) {
        double X[4] = {bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0};
        forward_px(s, n_items, i, X, nullptr);
        for (int k = 0; k < 4; ++k) image[4 * (size_t)i + k] = X[k];
    }
}

// grad_cover n_paths x n_px holds T_p between the two walks and the clip planes' suffix products inside END and HOLD, as on the
// device; every summed output gets its terms in pixel order.  n_walk0 is the index after the last END_MASK.
void mkh_backward(const double* cover, const double* paints, const int* desc, const double* m6, const double* geom, const double* pos,
                  const double* rgba, const double* bg, const long long* view, const int* items, int n_items, int n_walk0, const int* clip_off,
                  const int* clip_planes, const double* opacity, const double* grad_image, int n_paths, int n_stops, int n_groups, int n_pairs,
                  int n_opacities, long long n_px, double* grad_cover, double* grad_paints, double* grad_m6, double* grad_geom, double* grad_pos,
                  double* grad_rgba, double* grad_opacity) {
    const Scene s = {cover, paints, desc, m6, geom, pos, rgba, view, items, clip_off, clip_planes, opacity, n_px};
    for (int j = 0; j < 4 * n_paths; ++j) grad_paints[j] = grad_geom[j] = 0.0;
    for (int j = 0; j < 6 * n_paths; ++j) grad_m6[j] = 0.0;
    for (int j = 0; j < n_stops; ++j) grad_pos[j] = 0.0;
    for (int j = 0; j < 4 * n_stops; ++j) grad_rgba[j] = 0.0;
    for (int j = 0; j < n_opacities; ++j) grad_opacity[j] = 0.0;
    std::vector<double> t_end((size_t)n_groups + 1), park(4 * (size_t)n_pairs + 4);
    for (long long i = 0; i < n_px; ++i) {
        if (n_walk0 > 0) {
            double X0[4] = {bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0};
            forward_px(s, n_walk0, i, X0, park.data());
        }
        double above = 1.0;
        for (int q = n_items - 1; q >= 0; --q) {
            const int* it = items + 4 * (size_t)q;
            const int op = mask_op(it[0]);
            if (op == GROUP_FILL) {
                const int p = it[1];
                const size_t at = (size_t)p * n_px + i;
                double col[4];
                GradPaintPx e;
                const double u = colour_of(s, p, i, col, e) ? gradpaint_through(cover[at], col, paints + 4 * (size_t)p)
                                                            : compose_through(cover[at], paints[4 * (size_t)p + 3]);
                grad_cover[at] = above;
                above = above * u;
            } else if (op == GROUP_END) {
                t_end[it[1]] = above;
                above = 1.0;
            } else if (op == MASK_END) {
                t_end[it[2]] = above;
                above = 1.0;
            } else if (op == MASK_HOLD) {
                above = 1.0;
            } else if (op == GROUP_BEGIN) {
                const double u = group_through(above, opacity_of(s, it[2]), mask_of(s, it[3], i));
                above = t_end[it[1]] * u;
            } else if (op == MASK_BEGIN_HELD) {
                const double u = mask_through(above, opacity_of(s, it[2]), mask_of(s, it[3], i), mask_value(&park[4 * (size_t)mask_pair(it[0])]));
                above = t_end[it[1]] * u;
            }
        }
        double X[GROUP_DEPTH + 1][4] = {{bg ? bg[0] : 0.0, bg ? bg[1] : 0.0, bg ? bg[2] : 0.0, bg ? bg[3] : 0.0}};
        double B[GROUP_DEPTH + 1][4], H[GROUP_DEPTH][4];
        double qok = 0.0;
        for (int k = 0; k < 4; ++k) B[0][k] = grad_image[4 * (size_t)i + k];
        int level = 0;
        for (int q = 0; q < n_items; ++q) {
            const int* it = items + 4 * (size_t)q;
            const int op = mask_op(it[0]);
            if (op == GROUP_FILL) {
                const int p = it[1];
                const int* d = desc + 4 * (size_t)p;
                const size_t at = (size_t)p * n_px + i;
                const double* paint = paints + 4 * (size_t)p;
                double* gp = grad_paints + 4 * (size_t)p;
                double col[4], P[4], t[4], dense[GRADPAINT_DENSE], lo[GRADPAINT_STOP], hi[GRADPAINT_STOP];
                GradPaintPx e;
                if (!colour_of(s, p, i, col, e)) {
                    grad_cover[at] = compose_vjp_step(X[level], grad_cover[at], B[level], cover[at], paint, t);
                    compose_step(X[level], cover[at], paint);
                    for (int k = 0; k < 4; ++k) gp[k] = gp[k] + t[k];
                    continue;
                }
                gradpaint_effective(col, paint, P);
                grad_cover[at] = compose_vjp_step(X[level], grad_cover[at], B[level], cover[at], P, t);
                gradpaint_vjp(d[0], geom + 4 * (size_t)p, pos + d[2], rgba + 4 * (size_t)d[2], col, paint, e, t, dense, lo, hi);
                gradpaint_step(X[level], cover[at], col, paint);
                for (int k = 0; k < 4; ++k) gp[k] = gp[k] + dense[k];
                for (int k = 0; k < 6; ++k) grad_m6[6 * (size_t)p + k] = grad_m6[6 * (size_t)p + k] + dense[4 + k];
                for (int k = 0; k < 4; ++k) grad_geom[4 * (size_t)p + k] = grad_geom[4 * (size_t)p + k] + dense[10 + k];
                if (e.lo < 0) continue;
                grad_pos[d[2] + e.lo] = grad_pos[d[2] + e.lo] + lo[0];
                for (int k = 0; k < 4; ++k) grad_rgba[4 * (size_t)(d[2] + e.lo) + k] = grad_rgba[4 * (size_t)(d[2] + e.lo) + k] + lo[1 + k];
                if (e.hi == e.lo) continue;
                grad_pos[d[2] + e.hi] = grad_pos[d[2] + e.hi] + hi[0];
                for (int k = 0; k < 4; ++k) grad_rgba[4 * (size_t)(d[2] + e.hi) + k] = grad_rgba[4 * (size_t)(d[2] + e.hi) + k] + hi[1 + k];
            } else if (op == GROUP_BEGIN || op == MASK_BEGIN_HELD) {
                double adj[4];
                group_adjoint(X[level], t_end[it[1]], B[level], adj);
                ++level;
                for (int k = 0; k < 4; ++k) X[level][k] = 0.0;
                if (op == GROUP_BEGIN) group_base(adj, opacity_of(s, it[2]), mask_of(s, it[3], i), B[level]);
                else mask_base(adj, opacity_of(s, it[2]), mask_of(s, it[3], i), mask_value(&park[4 * (size_t)mask_pair(it[0])]), B[level]);
            } else if (op == MASK_BEGIN_MASK) {
                ++level;
                for (int k = 0; k < 4; ++k) X[level][k] = 0.0;
                mask_base_of_mask(qok, &park[4 * (size_t)mask_pair(it[0])], B[level]);
            } else if (op == MASK_END) {
                --level;
                mask_step(X[level], H[level], mask_value(&park[4 * (size_t)mask_pair(it[0])]));
            } else {
                --level;
                const bool hold = op == MASK_HOLD;
                const double* G = X[level + 1];
                const double o = opacity_of(s, it[2]);
                double adj[4];
                group_adjoint(X[level], t_end[it[1]], B[level], adj);
                const double qd = compose_dot(adj, G);
                const double km = hold ? mask_value(&park[4 * (size_t)mask_pair(it[0])]) : 1.0;
                const double dk = hold ? mask_clip_term(qd, o, km) : qd * o;
                double k = 1.0;
                if (it[3] >= 0) {
                    const int a0 = clip_off[it[3]], a1 = clip_off[it[3] + 1];
                    double suffix = 1.0;
                    for (int a = a1 - 1; a >= a0; --a) {
                        const size_t at = (size_t)clip_planes[a] * n_px + i;
                        grad_cover[at] = suffix;
                        suffix = suffix * (1.0 - cover[at]);
                    }
                    k = 0.0;
                    for (int a = a0; a < a1; ++a) {
                        const size_t at = (size_t)clip_planes[a] * n_px + i;
                        grad_cover[at] = group_clip_vjp(dk, a == a0, k, grad_cover[at]);
                        k = group_mask_step(k, cover[at], a == a0);
                    }
                }
                if (it[2] >= 0) grad_opacity[it[2]] = grad_opacity[it[2]] + (hold ? mask_opacity_term(qd, k, km) : qd * k);
                if (hold) {
                    qok = mask_held_dot(qd, o, k);
                    mask_hold(G, o, k, H[level]);
                } else {
                    group_step(X[level], G, o, k);
                }
            }
        }
    }
}

}  // extern "C"
