// svgr_compose.h -- per-pixel arithmetic of differentiable compositing: solid fills painted source-over in paint order (forward),
// and the derivative of sum(grad_image * image) with respect to every coverage value and every paint (backward).
//
// Everything here is plain double arithmetic, compilable for the host (the CPU harness of tests/compose_harness.cpp) and for the
// device (k_compose_over, k_compose_vjp of svgr_hip.hip).  Both sides are compiled with -ffp-contract=off and nothing below is a
// fused multiply-add: every product and every sum is rounded on its own, in the order written.  DESIGN.md 7x has the derivation;
// tests/compose_ref.py restates it in numpy.
//
//   forward   C = bg; for p = 0 .. n_paths - 1:  s_k = m_p paint_p[k],  C_k = s_k + C_k (1 - s_3)       (compose_step)
//             the fill is the oracle's orc_fill_solid (mask * paint), the step over_px (src + dst * (1 - src_a)): no clamp
//   backward  u_p = 1 - m_p a_p,  T_p = prod_{q > p} u_q,  C_{p-1} the canvas under path p,  g = T_p grad_image:
//               d / d m_p          = g . paint_p - a_p (g . C_{p-1})
//               d / d paint_p[k<3] = sum over pixels of m_p g_k
//               d / d paint_p[3]   = sum over pixels of m_p (g_3 - g . C_{p-1})
//             walk 1 (compose_through) runs from the top path down and leaves T_p; walk 2 (compose_vjp_step, then compose_step)
//             runs from the bottom up and carries C_{p-1} as the forward does.  Nothing is divided: C_{p-1} = (C_p - s) / u_p has
//             u_p == 0 under an opaque paint on a covered pixel.
//   dots      g . x = ((g_0 x_0 + g_1 x_1) + g_2 x_2) + g_3 x_3
#pragma once
#include "svgr_core.h"

namespace svgr {

// one solid fill source-over the canvas: C <- m paint + C (1 - m paint[3])
SVGR_HD void compose_step(double* C, double m, const double* paint) {
    const double s0 = m * paint[0], s1 = m * paint[1], s2 = m * paint[2], s3 = m * paint[3];
    over_px(C, s0, s1, s2, s3);
}

// walk 1: what a path lets through of the paths under it, u = 1 - m a
SVGR_HD double compose_through(double m, double alpha) { return 1.0 - m * alpha; }

SVGR_HD double compose_dot(const double* g, const double* x) { return ((g[0] * x[0] + g[1] * x[1]) + g[2] * x[2]) + g[3] * x[3]; }

// walk 2 at path p of one pixel: C is the canvas UNDER the path, T = T_p, gi the pixel of grad_image.  Returns d / d m_p;
// t[0..3] are the pixel's terms of d / d paint_p.
SVGR_HD double compose_vjp_step(const double* C, double T, const double* gi, double m, const double* paint, double* t) {
    const double g[4] = {T * gi[0], T * gi[1], T * gi[2], T * gi[3]};
    const double gc = compose_dot(g, C);
    const double gp = compose_dot(g, paint);
    t[0] = m * g[0];
    t[1] = m * g[1];
    t[2] = m * g[2];
    t[3] = m * (g[3] - gc);
    return gp - paint[3] * gc;
}

}  // namespace svgr
