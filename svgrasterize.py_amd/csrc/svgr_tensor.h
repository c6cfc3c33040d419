// svgr_tensor.h -- tensor output (svgr_layer_to_tensor / svgr_tensor_to_layer): what one lane does to one pixel.
//
// Everything here is per pixel, in double, every operation rounded on its own (no contraction: -ffp-contract=off, the one fma
// is spelled out), compilable for the host (the CPU harness of tests/tensor_harness.cpp) and for the device (k_tensor_pack and
// k_tensor_unpack of svgr_hip.hip).  DESIGN.md 7p has the definitions; tests/tensor_ref.py restates them in numpy.
//
//   pixel       RGBA as the caller prepared it (colour space and alpha state are Layer.convert's business: no pow and no
//               division here); a float32 canvas is widened exactly, a 1-channel mask is broadcast to all four channels
//               (Layer.compose's rule), a pixel outside the source's box is (0, 0, 0, 0)
//   background  optional, premultiplied input only: c = c + bg_c * (1 - a) for the three colours, then a = 1
//   channels    RGBA (4), RGB (3), ALPHA (1) or LUMA (1: fma(b, 0.072, fma(g, 0.7154, r * 0.2125)), svgr_layer_luminance's weights
//               and order without its multiplication by alpha)
//   affine      y = v * scale[k] + bias[k] per output channel; skipped altogether when every scale is 1 and every bias 0 (so a
//               -0.0 stays -0.0)
//   element     F32: y rounded to nearest-even.  F16 / BF16: that float32 rounded to nearest-even again (the two steps of
//               tensor.float().half()), by integer arithmetic on the bits: overflow gives infinity, subnormal results are kept.
//               U8: rint(y * 255) saturated to [0, 255], NaN gives 0.  Every NaN leaves as THE quiet NaN of its type (7fc00000,
//               7e00, 7fc0), whatever its sign and payload were: the host and the device cannot differ in it
//   inverse     element -> double, exact: U8 is v / 255, the halves are widened
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define TENSOR_HD __host__ __device__ inline
#else
#define TENSOR_HD inline
#endif

constexpr int TENSOR_SRC_RGBA_F64 = 0, TENSOR_SRC_RGBA_F32 = 1, TENSOR_SRC_MASK_F64 = 2, TENSOR_SRC_KINDS = 3;
constexpr int TENSOR_F32 = 0, TENSOR_F16 = 1, TENSOR_BF16 = 2, TENSOR_U8 = 3, TENSOR_DTYPES = 4;
constexpr int TENSOR_RGBA = 0, TENSOR_RGB = 1, TENSOR_ALPHA = 2, TENSOR_LUMA = 3, TENSOR_CHANNEL_KINDS = 4;

// what the launch passes to every lane
struct TensorOp {
    int dtype, channels, has_bg, affine;
    double bg[3];
    double scale[4], bias[4];
};

TENSOR_HD int tensor_n_channels(int channels) { return channels == TENSOR_RGBA ? 4 : channels == TENSOR_RGB ? 3 : 1; }
TENSOR_HD int tensor_elem_bytes(int dtype) { return dtype == TENSOR_F32 ? 4 : dtype == TENSOR_U8 ? 1 : 2; }

TENSOR_HD uint32_t tensor_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
TENSOR_HD float tensor_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// float32 bits -> float16 bits, round to nearest-even
TENSOR_HD uint32_t tensor_f16_bits(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a > 0x7f800000u) return 0x7e00u;
    const uint32_t e = a >> 23;
    if (e >= 113u) {   // a normal half, or beyond: the exponent rebiased by 127 - 15, the carry of the rounding runs into it
        const uint32_t v = a - 0x38000000u, rem = v & 0x1fffu;
        uint32_t r = v >> 13;
        if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
        return sign | (r > 0x7c00u ? 0x7c00u : r);
    }
    if (e < 102u) return sign;   // below 2^-25: zero
    // a subnormal half is a multiple of 2^-24: the 24-bit significand shifted down by 126 - e (14 .. 24)
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, s = 126u - e, rem = m & ((1u << s) - 1u), half = 1u << (s - 1u);
    uint32_t r = m >> s;
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return sign | r;
}
// float32 bits -> bfloat16 bits, round to nearest-even (the carry runs into the exponent and, at the top, into infinity)
TENSOR_HD uint32_t tensor_bf16_bits(uint32_t x) {
    if ((x & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    const uint32_t rem = x & 0xffffu;
    uint32_t r = x >> 16;
    if (rem > 0x8000u || (rem == 0x8000u && (r & 1u))) ++r;
    return r;
}
// float16 bits -> float32 bits, exact
TENSOR_HD uint32_t tensor_f16_widen(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return sign | 0x7f800000u | (m << 13);
    if (e) return sign | ((e + 112u) << 23) | (m << 13);
    if (!m) return sign;
    int k = 0;   // a subnormal: m * 2^-24, its leading bit moved up to bit 10
    uint32_t n = m;
    while (!(n & 0x400u)) { n <<= 1; ++k; }
    return sign | ((uint32_t)(113 - k) << 23) | ((n & 0x3ffu) << 13);
}

// One value to its element's bits (in the low 32, 16 or 8 bits).
TENSOR_HD uint32_t tensor_encode(int dtype, double y) {
    if (dtype == TENSOR_U8) {
        const double r = rint(y * 255.0);
        return !(r >= 0.0) ? 0u : r > 255.0 ? 255u : (uint32_t)(int)r;   // (NaN -> 0)
    }
    if (y != y) return dtype == TENSOR_F32 ? 0x7fc00000u : dtype == TENSOR_F16 ? 0x7e00u : 0x7fc0u;
    const uint32_t f = tensor_f32_bits((float)y);
    return dtype == TENSOR_F32 ? f : dtype == TENSOR_F16 ? tensor_f16_bits(f) : tensor_bf16_bits(f);
}
// The inverse: an element's bits to double.
TENSOR_HD double tensor_decode(int dtype, uint32_t bits) {
    if (dtype == TENSOR_U8) return (double)(bits & 255u) / 255.0;
    if (dtype == TENSOR_F32) return (double)tensor_bits_f32(bits);
    return (double)tensor_bits_f32(dtype == TENSOR_F16 ? tensor_f16_widen(bits & 0xffffu) : (bits & 0xffffu) << 16);
}

// One pixel through background, channel selection and affine: y[0 .. n), n = tensor_n_channels(op.channels).
TENSOR_HD int tensor_px(const TensorOp& op, double r, double g, double b, double a, double* y) {
    if (op.has_bg) {
        const double t = 1.0 - a;
        r = r + op.bg[0] * t;
        g = g + op.bg[1] * t;
        b = b + op.bg[2] * t;
        a = 1.0;
    }
    int n;
    if (op.channels == TENSOR_RGBA) { y[0] = r; y[1] = g; y[2] = b; y[3] = a; n = 4; }
    else if (op.channels == TENSOR_RGB) { y[0] = r; y[1] = g; y[2] = b; n = 3; }
    else if (op.channels == TENSOR_ALPHA) { y[0] = a; n = 1; }
    else { y[0] = fma(b, 0.072, fma(g, 0.7154, r * 0.2125)); n = 1; }
    if (op.affine)
        for (int k = 0; k < n; ++k) y[k] = y[k] * op.scale[k] + op.bias[k];
    return n;
}

// The pixel (row, col) of the plane out of a source over the box {s0, s1, srows, scols}: zero outside it.
TENSOR_HD void tensor_load_px(const void* src, int kind, int64_t row, int64_t col, int64_t s0, int64_t s1, int64_t srows, int64_t scols,
                              double* px) {
    const int64_t r = row - s0, c = col - s1;
    if (r < 0 || c < 0 || r >= srows || c >= scols) { px[0] = px[1] = px[2] = px[3] = 0.0; return; }
    const int64_t i = r * scols + c;
    if (kind == TENSOR_SRC_RGBA_F64) {
#if defined(__HIP_DEVICE_COMPILE__)
        const double4 v = ((const double4*)src)[i];   // (one pixel, two 16-byte loads)
        px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
#else
        const double* p = (const double*)src + 4 * i;
        px[0] = p[0]; px[1] = p[1]; px[2] = p[2]; px[3] = p[3];
#endif
    } else if (kind == TENSOR_SRC_RGBA_F32) {
#if defined(__HIP_DEVICE_COMPILE__)
        const float4 v = ((const float4*)src)[i];
        px[0] = (double)v.x; px[1] = (double)v.y; px[2] = (double)v.z; px[3] = (double)v.w;
#else
        const float* p = (const float*)src + 4 * i;
        px[0] = (double)p[0]; px[1] = (double)p[1]; px[2] = (double)p[2]; px[3] = (double)p[3];
#endif
    } else {
        px[0] = px[1] = px[2] = px[3] = ((const double*)src)[i];
    }
}

// The inverse of the channel selection: n elements of a pixel to the layer's 4 (RGBA, RGB: a = 1) or 1 (ALPHA, LUMA) values.
TENSOR_HD int tensor_unpack_px(int channels, const double* v, double* px) {
    if (channels == TENSOR_RGBA) { px[0] = v[0]; px[1] = v[1]; px[2] = v[2]; px[3] = v[3]; return 4; }
    if (channels == TENSOR_RGB) { px[0] = v[0]; px[1] = v[1]; px[2] = v[2]; px[3] = 1.0; return 4; }
    px[0] = v[0];
    return 1;
}
