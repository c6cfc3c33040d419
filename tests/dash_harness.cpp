// dash_harness.cpp -- the dasher's per-lane header (csrc/svgr_dash.h) compiled for the host, for tests/test_dash_host.py
// (built by tests/util.py: host_build): sub-interval lengths, inversion, split and the piece counts of a segment range, one C entry each.
#include "../svgrasterize.py_amd/csrc/svgr_dash.h"

extern "C" {

void dh_sub_lengths(const double* c, double* out32) {
    for (int i = 0; i < DASH_SUB; ++i) out32[i] = dash_sub_length(c, i);
}
void dh_table(const double* c, double* tab32) { dash_cubic_table(c, tab32); }
double dh_line_length(const double* q) { return dash_line_length(q); }
double dh_invert(const double* c, double s) {
    double tab[DASH_SUB];
    dash_cubic_table(c, tab);
    return dash_invert(c, tab, s);
}
void dh_split(const double* c, double ta, double tb, double* out8) { dash_split(c, ta, tb, out8); }

// pieces and started dashes of a segment of length s1 - s0 that owns [s0, s1) of a subpath in mode `mode`; out = {pieces, starts}
void dh_count(const double* dashes, int n, double offset, double scale, int type, double s0, double s1, int mode, long long* out) {
    DashPat pat;
    dash_build_pattern(dashes, n, offset, scale, pat);
    DashSeg g;
    dash_seg_pieces(pat, type, s1 - s0, s0, s1, mode, g);
    out[0] = g.cnt;
    out[1] = g.cnt - g.cont;
}
int dh_mode(const double* dashes, int n, double offset, double scale, double L, int closed) {
    DashPat pat;
    dash_build_pattern(dashes, n, offset, scale, pat);
    return dash_sub_mode(pat, L, closed != 0);
}
// piece q of a lone segment (type 0 line / 2 cubic) that begins its subpath: out8 control points; returns the output type
int dh_piece(const double* dashes, int n, double offset, int type, const double* c, long long q, double* out8) {
    DashPat pat;
    dash_build_pattern(dashes, n, offset, 1.0, pat);
    double tab[DASH_SUB] = {0};
    double len;
    if (type == 2) { dash_cubic_table(c, tab); len = tab[DASH_SUB - 1]; }
    else len = dash_line_length(c);
    DashSeg g;
    dash_seg_pieces(pat, type, len, 0.0, len, DASH_NORMAL, g);
    if (q < 0 || q >= g.cnt) return -1;
    long long k;
    int j;
    return dash_piece(pat, g, type, c, tab, len, DASH_NORMAL, q, k, j, out8);
}

}  // extern "C"
