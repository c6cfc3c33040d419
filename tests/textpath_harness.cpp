// textpath_harness.cpp -- the text-on-a-path per-lane header (csrc/svgr_textpath.h) compiled for the host, for
// tests/test_textpath_host.py (g++ -ffp-contract=off): the lanes of the two kernels run one after the other, the measure as
// the dasher's sequential table, the scan in between as a plain running sum.  With TEXTPATH_HARNESS_MAIN it is a program of
// its own (a sanitizer build runs that).
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_textpath.h"

namespace {
struct Measured {
    std::vector<double> len, tab, inc;
};
void measure(const int* types, const double* params, int n, Measured& m) {
    m.len.assign((size_t)n, 0.0);
    m.tab.assign((size_t)n * DASH_SUB, 0.0);
    m.inc.assign((size_t)n, 0.0);
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        const double* c = params + (size_t)i * 8;
        if (types[i] == SVGR_PATH_CUBIC) {
            dash_cubic_table(c, &m.tab[(size_t)i * DASH_SUB]);
            m.len[(size_t)i] = m.tab[(size_t)i * DASH_SUB + DASH_SUB - 1];
        } else if (types[i] != SVGR_PATH_UNCLOSED) {
            m.len[(size_t)i] = dash_line_length(c);
        }
        acc += m.len[(size_t)i];
        m.inc[(size_t)i] = acc;
    }
}
}  // namespace

extern "C" {

int th_count(const double* a, int n, double s, int strict) { return textpath_count(a, n, s, strict != 0); }
int th_owner(const int* off, int n, int j) { return textpath_owner(off, n, j); }
void th_place(const double* frame4, double h, double dy, double x, double y, double* out2) {
    const TextFrame f{frame4[0], frame4[1], frame4[2], frame4[3]};
    textpath_place(f, h, dy, x, y, out2[0], out2[1]);
}

// svgr_path_sample over n >= 1 segments: xyuv 4 per query, inside; returns the total length.
double th_sample(const int* types, const double* params, int n, const double* s, int nq, double* xyuv, int* inside) {
    Measured m;
    measure(types, params, n, m);
    const TextPathView v{types, params, m.len.data(), m.tab.data(), m.inc.data(), n};
    for (int q = 0; q < nq; ++q) {
        TextFrame f;
        inside[q] = textpath_locate(v, s[q], f);
        xyuv[4 * q] = f.x; xyuv[4 * q + 1] = f.y; xyuv[4 * q + 2] = f.ux; xyuv[4 * q + 3] = f.uy;
    }
    return m.inc[(size_t)n - 1];
}

// svgr_path_place_glyphs: inst_off (n_inst + 1) as the library's host side builds it; returns 0, or -1 when a lane met a slot
// outside the result.
int th_place_glyphs(const int* types, const double* params, int n, const int* atlas_types, const double* atlas_params, int n_atlas,
                    const int* glyph_seg_off, const int* inst_glyph, const int* inst_off, const double* s_mid, const double* half,
                    const double* dy, int n_inst, double* out, int* visible) {
    std::vector<double> frames((size_t)n_inst * 4 + 4);
    th_sample(types, params, n, s_mid, n_inst, frames.data(), visible);
    const TextEmitView v{atlas_types, atlas_params, glyph_seg_off, inst_glyph, inst_off, half, dy, frames.data(), visible, n_inst, n_atlas};
    bool ok = true;
    for (int j = 0; j < inst_off[n_inst]; ++j) ok = textpath_emit(v, j, out + (size_t)j * 8) && ok;
    return ok ? 0 : -1;
}

}  // extern "C"

#if defined(TEXTPATH_HARNESS_MAIN)
#include <cstdio>
int main() {
    const int types[3] = {SVGR_PATH_LINE, SVGR_PATH_CUBIC, SVGR_PATH_UNCLOSED};
    const double params[24] = {0, 0, 10, 0, 0, 0, 0, 0, 10, 0, 20, 0, 30, 10, 30, 20, 30, 20, 0, 0, 0, 0, 0, 0};
    const int a_types[2] = {SVGR_PATH_LINE, SVGR_PATH_CUBIC};
    const double a_params[16] = {0, 0, 4, -6, 0, 0, 0, 0, 4, -6, 5, -2, 6, -1, 8, 0};
    const int g_off[3] = {0, 2, 2}, glyph[4] = {0, 1, 0, 0}, i_off[5] = {0, 2, 2, 4, 6};
    const double s_mid[4] = {-1.0, 3.0, 12.0, 25.0}, half[4] = {4, 2, 4, 4}, dy[4] = {0, 0, 1, -1};
    double out[48];
    int visible[4];
    const int rc = th_place_glyphs(types, params, 3, a_types, a_params, 2, g_off, glyph, i_off, s_mid, half, dy, 4, out, visible);
    std::printf("%d %d%d%d%d %.17g\n", rc, visible[0], visible[1], visible[2], visible[3], out[47]);
    return rc;
}
#endif
