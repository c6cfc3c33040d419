// svgr_box.h -- the box of a layer in device coordinates, and the three questions the layer, filter and paint kernels ask of it:
// which device pixel is lane i, does a device pixel lie in that other box (and where), and where do two boxes meet.
//
// Plain integer arithmetic, compilable for the host (tests/box_harness.cpp) and for the device (the layer and paint kernels of
// svgr_hip.hip).  DESIGN.md 7c-box has the definitions.
//
//   Box       rows r0 .. r0 + rows - 1 and columns c0 .. c0 + cols - 1; a layer over it is row-major, pixel (R, C) at index
//             (R - r0) * cols + (C - c0).  Empty when rows == 0 or cols == 0.
//   admitted  box_of is the one door from the ABI's int64_t[4]: origins inside +-2^30, extents in [0, 2^30).  Every pixel of
//             an admitted box, and its one-pixel halo, therefore has coordinates in (-2^30 - 1, 2^31 - 1): ints.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "svgr_core.h"

namespace svgr {

struct Box {
    int r0, c0, rows, cols;
};

// what the ABI's entries accept as a box: the checks, and the narrowing, once
SVGR_HD bool box_of(const int64_t* bb, Box& out) {
    const int64_t lim = (int64_t)1 << 30;
    if (!bb || bb[2] < 0 || bb[3] < 0 || bb[2] >= lim || bb[3] >= lim || bb[0] <= -lim || bb[0] >= lim || bb[1] <= -lim || bb[1] >= lim)
        return false;
    out = Box{(int)bb[0], (int)bb[1], (int)bb[2], (int)bb[3]};
    return true;
}

SVGR_HD size_t box_px(const Box& b) { return (size_t)b.rows * (size_t)b.cols; }

// the device row and column of the box's pixel i (row-major, i < box_px(b))
SVGR_HD void box_cell(const Box& b, size_t i, int& R, int& C) {
    R = b.r0 + (int)(i / b.cols);
    C = b.c0 + (int)(i % b.cols);
}

// Does device pixel (R, C) lie in b?  Then `at` is its index in a layer over b.
// One unsigned compare per axis.  With d = R - r0 as an integer, R a pixel (or halo pixel) of an admitted box and b admitted,
// -2^31 < d < 3 * 2^30, so the 32-bit unsigned difference is d itself when d >= 0 and d + 2^32 > 2^31 when d < 0: it is below
// rows (< 2^30) exactly when 0 <= d < rows.  The signed subtraction R - r0 could overflow an int there; the unsigned one wraps
// by definition and the compare reads the wrap as "outside".
SVGR_HD bool box_find(const Box& b, int R, int C, size_t& at) {
    const unsigned r = (unsigned)R - (unsigned)b.r0, c = (unsigned)C - (unsigned)b.c0;
    if (r >= (unsigned)b.rows || c >= (unsigned)b.cols) return false;
    at = (size_t)r * (size_t)b.cols + c;
    return true;
}

// the intersection of two admitted boxes; rows == 0 or cols == 0 (or both) when they are disjoint or one is empty
// (origin and end of admitted boxes lie inside +-2^31: the int sums below do not overflow)
SVGR_HD Box box_meet(const Box& a, const Box& b) {
    const int r0 = a.r0 > b.r0 ? a.r0 : b.r0, c0 = a.c0 > b.c0 ? a.c0 : b.c0;
    const int r1 = a.r0 + a.rows < b.r0 + b.rows ? a.r0 + a.rows : b.r0 + b.rows;
    const int c1 = a.c0 + a.cols < b.c0 + b.cols ? a.c0 + a.cols : b.c0 + b.cols;
    return Box{r0, c0, r1 > r0 ? r1 - r0 : 0, c1 > c0 ? c1 - c0 : 0};
}

}  // namespace svgr
