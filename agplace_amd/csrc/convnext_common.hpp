// Shared by convnext.hip (forward) and convnext_bwd.hip (backward): tile constants, wave reductions, the three-product MFMA, and the
// one-product fp16 MFMA with its conversion (the forward's precision 4).
#pragma once
#include "common.hpp"

namespace {

constexpr int CNX_TP = 32;         // pixels per tile of the matrix kernels (one MFMA column block)
constexpr int CNX_KPAD = 8;        // bf16 elements of padding per LDS operand row (16 B: spreads the rows over the banks)

// sum over the 32 lanes of a half wave (lanes that share lane >> 5)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over 8 consecutive lanes
__device__ __forceinline__ float oct_sum(float v) {
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

__device__ __forceinline__ void mfma3(f32x16& acc, const bf16x8& wh, const bf16x8& wl, const bf16x8& xh, const bf16x8& xl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh, acc, 0, 0, 0);
}

// ---- precision 4 of the inference kernels (convnext.hip, PREC = 4): fp16 operands, ONE product per MFMA.  The fragments travel
// in the bf16 fragment type (8 x 16 bits) so that both precisions share loads, stores and signatures.
__device__ __forceinline__ void mfma1h(f32x16& acc, const bf16x8& w, const bf16x8& x) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x), acc, 0, 0, 0);
}
// two fp32 -> one packed fp16 pair (a in the low half): round to nearest even, saturating at +-65504, NaN kept (the clamp alone
// would turn a NaN into -65504: v_med3_f32 returns the minimum of its operands when one is NaN)
__device__ __forceinline__ uint32_t cnx_h2(float a, float b) {
    const float ca = __builtin_amdgcn_fmed3f(a, -65504.f, 65504.f), cb = __builtin_amdgcn_fmed3f(b, -65504.f, 65504.f);
    const f32x2v v = {a != a ? a : ca, b != b ? b : cb};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ bf16_t cnx_h1(float a) { return (bf16_t)(cnx_h2(a, 0.f) & 0xffffu); }

// feature row (inside a 32-row block) of accumulator register `reg` of a lane in half `h`
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---- the stem's two image sources (cnx_stem_kernel, cnx_stem_bwd_kernel: templated on the loader).  A loader returns element
// (image, channel, row y, panorama column X) of the logical fp32 image [n][3][h][W]; everything after the load is shared.
struct CnxLoadF32 {            // fp32 [n][3][h][W] with element strides
    const float* x;
    long long sn, sc, sh, sw;
    __device__ __forceinline__ float operator()(long long img, int ci, int y, int X) const {
        return x[img * sn + ci * sc + (long long)y * sh + (long long)X * sw];
    }
};
// ToTensor + Normalize of one byte: pack_u8_cams_kernel's expression (pack.hip).  The ONE definition behind agp_normalize_u8_cams
// and the uint8 stems, so the three give the same bits.
__device__ __forceinline__ float cnx_norm_u8(uint8_t u, float mean, float stdv) { return ((float)u / 255.f - mean) / stdv; }
struct CnxLoadU8 {             // uint8 camera tiles [n][ncam][h][w][3]; the image is the panorama [n][3][h][ncam * w]
    const uint8_t* t;
    int ncam, h, w;
    float m0, m1, m2, s0, s1, s2;
    // one byte per load, addressed per element by panorama column (a 4x4 patch may straddle cameras): cam < ncam, x < w, y < h
    // for every (y, X) inside the panorama, so no load leaves the n * ncam * h * w * 3 bytes
    __device__ __forceinline__ float operator()(long long img, int ci, int y, int X) const {
        const int cam = X / w, x = X - cam * w;
        const uint8_t u = t[((((long long)img * ncam + cam) * h + y) * w + x) * 3 + ci];
        return cnx_norm_u8(u, ci == 0 ? m0 : ci == 1 ? m1 : m2, ci == 0 ? s0 : ci == 1 ? s1 : s2);
    }
};

inline long long cnx_pad(long long P) { return (P + CNX_TP - 1) / CNX_TP * CNX_TP; }
inline bool cnx_c_host_ok(int C) { return C == 96 || C == 192 || C == 384; }
inline bool cnx_map_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (long long)n * h * w < (1ll << 31) / 32; }

}  // namespace
