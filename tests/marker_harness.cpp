// marker_harness.cpp -- the marker pass's per-lane header (csrc/svgr_marker.h) compiled for the host, for
// tests/test_marker_host.py (g++ -ffp-contract=off): the lanes of the three kernels run one after the other, the scan in
// between as a plain running sum.
#include <vector>

#include "../svgrasterize.py_amd/csrc/svgr_marker.h"

extern "C" {

int mh_unit(double dx, double dy, double* out2) { return marker_unit(dx, dy, out2[0], out2[1]) ? 1 : 0; }
int mh_seg_dirs(int type, const double* c, double* out4) {
    MarkerDirs d{0.0, 0.0, 0.0, 0.0};
    const bool ok = marker_seg_dirs(type, c, d);
    out4[0] = d.sx; out4[1] = d.sy; out4[2] = d.ex; out4[3] = d.ey;
    return ok ? 1 : 0;
}
void mh_bisect(const double* in2, const double* out2, double* u2) { marker_bisect(in2[0], in2[1], out2[0], out2[1], u2[0], u2[1]); }

// The whole pass over n segments in n_sub non-empty subpaths (sub_off: n_sub + 1 entries): returns the vertex count, -1 when a
// lane met a slot outside [0, cap).  xyuv: 4 * cap doubles, kind: cap ints.
long long mh_path(const int* types, const double* params, const int* seg_vertex, const int* sub_off, int n_sub, long long cap,
                  double* xyuv, int* kind) {
    const int n = sub_off[n_sub];
    if (n == 0) return 0;
    std::vector<int> seg_sub((size_t)n), flags((size_t)n), tab((size_t)n, -1);
    std::vector<MarkerDirs> dirs((size_t)n);
    std::vector<MarkerCnt> cnt((size_t)n);
    for (int s = 0; s < n_sub; ++s)
        for (int i = sub_off[s]; i < sub_off[s + 1]; ++i) seg_sub[(size_t)i] = s;
    for (int i = 0; i < n; ++i) {
        MarkerDirs d{0.0, 0.0, 0.0, 0.0};
        flags[(size_t)i] = marker_classify(types, seg_sub.data(), sub_off, seg_vertex, i, params + (size_t)i * 8, d, cnt[(size_t)i]);
        dirs[(size_t)i] = d;
    }
    for (int i = 1; i < n; ++i) {
        cnt[(size_t)i].nd += cnt[(size_t)i - 1].nd;
        cnt[(size_t)i].v += cnt[(size_t)i - 1].v;
    }
    for (int i = 0; i < n; ++i)
        if (flags[(size_t)i] & MARKER_F_DIR) tab[(size_t)(cnt[(size_t)i].nd - 1)] = i;
    const long long n_vert = cnt[(size_t)n - 1].v;
    if (n_vert > cap) return -1;
    const MarkerView v{types, params, seg_sub.data(), sub_off, flags.data(), dirs.data(), cnt.data(), tab.data(), n};
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = marker_emit(v, i, n_vert, xyuv, kind) && ok;
    return ok ? n_vert : -1;
}

}  // extern "C"
