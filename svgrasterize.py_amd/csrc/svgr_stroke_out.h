// svgr_stroke_out.h -- the path a stroke-side entry point hands back (svgr_path_stroke, svgr_path_dash): flat arrays in the
// layout of Path.from_segments, read with svgr_stroke_out_counts / _copy and released with svgr_stroke_out_free.
#pragma once
#include <cstdint>
#include <vector>

struct svgr_stroke_out {
    std::vector<int32_t> types;
    std::vector<double> params;  // 8 per segment
    std::vector<int32_t> sizes;
};
