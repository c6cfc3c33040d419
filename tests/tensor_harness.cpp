// CPU harness for tensor output: csrc/svgr_tensor.h driven serially on the host -- one loop iteration where k_tensor_pack and
// k_tensor_unpack of svgr_hip.hip have one lane.  The arithmetic is the header's own, so the elements this writes are the
// device's bit for bit; where an element goes is restated here from the description's strides, one element at a time.
// tests/test_tensor_host.py holds it against tests/tensor_ref.py, numpy and torch; with -DTENSOR_HARNESS_MAIN it is a stand-alone
// program (for a run under a sanitizer).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/svgr.h"
#include "../svgrasterize.py_amd/csrc/svgr_tensor.h"

namespace {

TensorOp op_of(const svgr_tensor_desc* d) {
    TensorOp op;
    memset(&op, 0, sizeof op);
    op.dtype = d->dtype; op.channels = d->channels; op.has_bg = d->has_bg;
    const int n = tensor_n_channels(d->channels);
    for (int k = 0; k < 4; ++k) {
        op.scale[k] = d->scale[k]; op.bias[k] = d->bias[k];
        if (k < n && (d->scale[k] != 1.0 || d->bias[k] != 0.0)) op.affine = 1;   // (svgr_layer_to_tensor's rule)
        if (k < 3) op.bg[k] = d->bg[k];
    }
    return op;
}

void put(void* dst, int dtype, int64_t at, uint32_t bits) {
    if (dtype == TENSOR_F32) ((uint32_t*)dst)[at] = bits;
    else if (dtype == TENSOR_U8) ((uint8_t*)dst)[at] = (uint8_t)bits;
    else ((uint16_t*)dst)[at] = (uint16_t)bits;
}
uint32_t get(const void* src, int dtype, int64_t at) {
    if (dtype == TENSOR_F32) return ((const uint32_t*)src)[at];
    if (dtype == TENSOR_U8) return ((const uint8_t*)src)[at];
    return ((const uint16_t*)src)[at];
}

}  // namespace

extern "C" {

uint32_t h_encode(int dtype, double y) { return tensor_encode(dtype, y); }
double h_decode(int dtype, uint32_t bits) { return tensor_decode(dtype, bits); }
uint32_t h_f16_bits(uint32_t f32_bits) { return tensor_f16_bits(f32_bits); }
uint32_t h_bf16_bits(uint32_t f32_bits) { return tensor_bf16_bits(f32_bits); }
uint32_t h_f16_widen(uint32_t h) { return tensor_f16_widen(h); }

void h_encode_many(int dtype, const double* y, int64_t n, uint32_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = tensor_encode(dtype, y[i]);
}

// svgr_layer_to_tensor without its checks: every element of the plane, nothing else of dst
void h_pack(const svgr_tensor_desc* d, const void* src, const int64_t* bb, void* dst) {
    const TensorOp op = op_of(d);
    for (int64_t r = 0; r < d->rows; ++r)
        for (int64_t c = 0; c < d->cols; ++c) {
            double px[4], y[4];
            tensor_load_px(src, d->source, r, c, bb[0], bb[1], bb[2], bb[3], px);
            const int n = tensor_px(op, px[0], px[1], px[2], px[3], y);
            for (int k = 0; k < n; ++k)
                put(dst, d->dtype, d->offset + k * d->stride_c + r * d->stride_h + c * d->stride_w, tensor_encode(d->dtype, y[k]));
        }
}

// svgr_tensor_to_layer without its checks
void h_unpack(const svgr_tensor_desc* d, const void* src, double* dst) {
    const int n_in = tensor_n_channels(d->channels);
    for (int64_t r = 0; r < d->rows; ++r)
        for (int64_t c = 0; c < d->cols; ++c) {
            double v[4], px[4];
            for (int k = 0; k < n_in; ++k) v[k] = tensor_decode(d->dtype, get(src, d->dtype, d->offset + k * d->stride_c + r * d->stride_h + c * d->stride_w));
            const int n = tensor_unpack_px(d->channels, v, px);
            for (int k = 0; k < n; ++k) dst[(r * d->cols + c) * n + k] = px[k];
        }
}

}  // extern "C"

#ifdef TENSOR_HARNESS_MAIN
int main() {
    // a 3 x 5 plane, a 2 x 4 layer hanging over its top left corner, every dtype and channel selection, both layouts
    std::vector<double> src(2 * 4 * 4);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (double)i / 31.0;
    const int64_t bb[4] = {-1, -1, 2, 4};
    unsigned long long sum = 0;
    for (int dtype = 0; dtype < TENSOR_DTYPES; ++dtype)
        for (int ch = 0; ch < TENSOR_CHANNEL_KINDS; ++ch)
            for (int hwc = 0; hwc < 2; ++hwc) {
                svgr_tensor_desc d;
                memset(&d, 0, sizeof d);
                const int n = tensor_n_channels(ch);
                d.source = TENSOR_SRC_RGBA_F64; d.dtype = dtype; d.channels = ch; d.has_bg = 1;
                for (int k = 0; k < 4; ++k) { d.scale[k] = 2.0; d.bias[k] = -0.5; }
                d.bg[0] = 0.25; d.bg[1] = 0.5; d.bg[2] = 0.75;
                d.rows = 3; d.cols = 5;
                d.stride_c = hwc ? 1 : 3 * 7; d.stride_h = hwc ? 5 * n + 2 : 7; d.stride_w = hwc ? n : 1; d.offset = 3;
                std::vector<uint8_t> dst((size_t)(3 + 4 * 3 * 7 + 3 * (5 * 4 + 2)) * 4, 0);
                h_pack(&d, src.data(), bb, dst.data());
                std::vector<double> back((size_t)3 * 5 * 4);
                h_unpack(&d, dst.data(), back.data());
                for (uint8_t b : dst) sum += b;
            }
    printf("tensor harness ok: %llu\n", sum);
    return 0;
}
#endif
