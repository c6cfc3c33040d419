// Host build of svgrasterize.py_amd/csrc/svgr_box.h (Box, box_of, box_px, box_cell, box_find, box_meet): the box arithmetic of
// the layer, filter and paint kernels.  For CPU-side unit tests only (tests/test_box_host.py).  NOT a CPU fallback of the
// product: the package never loads it.
#include "../svgrasterize.py_amd/csrc/svgr_box.h"

using namespace svgr;

static Box box(const int* b) { return Box{b[0], b[1], b[2], b[3]}; }

extern "C" {

// box_of on bb (or on a null pointer when is_null): 1 and out = {r0, c0, rows, cols} when admitted, else 0 and out untouched
int bx_of(const int64_t* bb, int is_null, int* out) {
    Box b;
    if (!box_of(is_null ? nullptr : bb, b)) return 0;
    out[0] = b.r0; out[1] = b.c0; out[2] = b.rows; out[3] = b.cols;
    return 1;
}

unsigned long long bx_px(const int* b) { return (unsigned long long)box_px(box(b)); }

// rc[2 k ..] = the device row and column of the box's pixel i[k]
void bx_cell(const int* b, long n, const unsigned long long* i, int* rc) {
    for (long k = 0; k < n; ++k) box_cell(box(b), (size_t)i[k], rc[2 * k], rc[2 * k + 1]);
}

// ok[k] = is device pixel rc[2 k ..] in the box; at[k] = its index then, untouched otherwise
void bx_find(const int* b, long n, const int* rc, unsigned char* ok, unsigned long long* at) {
    for (long k = 0; k < n; ++k) {
        size_t a;
        ok[k] = box_find(box(b), rc[2 * k], rc[2 * k + 1], a) ? 1 : 0;
        if (ok[k]) at[k] = (unsigned long long)a;
    }
}

void bx_meet(const int* a, const int* b, int* out) {
    const Box m = box_meet(box(a), box(b));
    out[0] = m.r0; out[1] = m.c0; out[2] = m.rows; out[3] = m.cols;
}

}  // extern "C"
