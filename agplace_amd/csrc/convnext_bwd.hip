// ConvNeXt-tiny backward kernels (agplace_amd/convnext.py: the opt-in training path).  First versions: correct, deterministic,
// not tuned.
//
// Arithmetic as in convnext.hip: every MFMA operand is a bf16 (hi, lo) pair, a product is hi*hi + hi*lo + lo*hi accumulated in
// fp32; LayerNorm, GELU' and all sums are fp32.  There is NO atomic in this file: every sum over pixels or workgroups is a
// register / LDS sum in a fixed order, or a per-slice partial plane that a following kernel adds in slice order, so two runs
// give the same bits.  Every entry accumulates (+=) into caller-owned fp32 gradient buffers in the parameters' own layouts.
//
// One block's backward, with xn the operand agp_cnx_dwconv_ln_fwd recomputes from the saved block input, gs = row_scale * gy:
//   cnx_mlp_dgrad_kernel   pixel-parallel (the forward's structure): h = W1 xn + b1, ga = (ls W2)^T gs, gh = ga GELU'(h),
//                          gxn = W1^T gh.  The hidden quantities live in accumulators only.
//   cnx_mlp_wgrad_kernel   hidden-parallel: a workgroup owns one 32-wide hidden block and a slice of CNX_SLICE_TILES pixel
//                          tiles; it recomputes h^T, ga^T (pixel on the accumulator row) and keeps gW1^T and
//                          G[c][j] = sum_p gs[p][c] a[p][j] of its block in accumulators across the sweep (K = pixels).
//   cnx_mlp_finish_kernel  gW2 += ls G, g_layer_scale[c] += sum_j W2[c][j] G[c][j] + b2[c] sum_p gs[p][c] (= sum_p gs m, without
//                          forming m from out - resid), gb2 += ls sum_p gs.
//   cnx_dwln_gz_kernel     recomputes the depthwise conv and the LayerNorm statistics, LayerNorm backward -> gz, g_gamma, g_beta,
//                          g_dwbias partials.
//   cnx_dw_bwd_kernel      gx = gy + transposed depthwise conv of gz; g_dw partials.
#include "convnext_common.hpp"

namespace {

constexpr int CNX_SLICE_TILES = 32;                          // 32-pixel tiles per pixel slice of the weight-gradient sweeps
constexpr int CNX_SLICE_PIXELS = CNX_SLICE_TILES * CNX_TP;   // 1024
constexpr int CNX_DW_TILES = 8;                              // 4 x 8 tiles per workgroup of cnx_dw_bwd_kernel
constexpr int CNX_STEM_TILES = 8;                            // 32-pixel tiles per workgroup of cnx_stem_bwd_kernel
constexpr int CNX_STEM_PART = 96 * 48 + 3 * 96;              // floats of one stem partial: gW, g_bias, g_gamma, g_beta
constexpr int CNX_REDUCE_GROUP = 16;                         // partials one thread adds per level of the final sums

// d/dx GELU(x) = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

// the operand planes of 32 pixels -> LDS [32][C + 8] (zeros beyond P)
template <int C, int NTHR>
__device__ __forceinline__ void load_planes(const bf16_t* __restrict__ x_hi, const bf16_t* __restrict__ x_lo, long long p0, long long P,
                                            bf16_t* sx_hi, bf16_t* sx_lo, int t) {
    constexpr int LD = C + CNX_KPAD, VR = C / 8;
    for (int e = t; e < CNX_TP * VR; e += NTHR) {
        const int row = e / VR, v = e - row * VR;
        u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
        if (p0 + row < P) {
            vh = *(const u32x4*)(x_hi + (size_t)(p0 + row) * C + v * 8);
            vl = *(const u32x4*)(x_lo + (size_t)(p0 + row) * C + v * 8);
        }
        *(u32x4*)(sx_hi + row * LD + v * 8) = vh;
        *(u32x4*)(sx_lo + row * LD + v * 8) = vl;
    }
}

// fp32 rows [P][ldg] (columns c0 .. c0 + W), times the row's image factor -> split planes in LDS [32][W + 8] (zeros beyond P)
template <int W, int NTHR>
__device__ __forceinline__ void load_rows_split(const float* __restrict__ g, int ldg, int c0, const float* __restrict__ row_scale,
                                                long long ppi, long long p0, long long P, bf16_t* s_hi, bf16_t* s_lo, int t) {
    constexpr int LD = W + CNX_KPAD, VR = W / 4;
    for (int e = t; e < CNX_TP * VR; e += NTHR) {
        const int row = e / VR, v = e - row * VR;
        f32x4 f = {0.f, 0.f, 0.f, 0.f};
        if (p0 + row < P) {
            f = *(const f32x4*)(g + (size_t)(p0 + row) * ldg + c0 + v * 4);
            if (row_scale) f *= row_scale[(p0 + row) / ppi];
        }
        bf16_t hi[4], lo[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split_bf16(f[i], hi[i], lo[i]);
        *(u32x2*)(s_hi + row * LD + v * 4) = u32x2{pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
        *(u32x2*)(s_lo + row * LD + v * 4) = u32x2{pack2(lo[0], lo[1]), pack2(lo[2], lo[3])};
    }
}

// A / B fragment with the PIXEL on the k slots: element e = LDS[pixel(e)][col].  ACC: the pixel order of an accumulator's
// registers 8 tt .. 8 tt + 7 (acc_row), the partner of an operand taken from an accumulator; else the natural order 16 tt + 8 h + e.
template <bool ACC>
__device__ __forceinline__ bf16x8 gather_px(const bf16_t* s, int ld, int col, int tt, int h) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (short)s[(ACC ? acc_row(8 * tt + e, h) : 16 * tt + 8 * h + e) * ld + col];
    return v;
}

// ------------------------------------------------------------------------------------------------- MLP: data gradient
//   w1 planes : [4C/32][C/16][64][8]      lane (r, h): W1[jb*32 + r][kk*16 + 8h + e]              (the forward's)
//   w2t planes: [4C/32][C/16][64][8]      lane (r, h): ls[c] W2[c][jb*32 + r], c = kk*16 + 8h + e
//   w1t planes: [4C/32][2][C/32][64][8]   lane (r, h): W1[jb*32 + acc_row(8t + e, h)][ct*32 + r]
template <int C>
__global__ __launch_bounds__(256) void cnx_mlp_dgrad_kernel(const bf16_t* __restrict__ x_hi, const bf16_t* __restrict__ x_lo,
                                                            const float* __restrict__ gy, const float* __restrict__ row_scale,
                                                            long long ppi, long long P, const bf16x8* __restrict__ w1_hi,
                                                            const bf16x8* __restrict__ w1_lo, const float* __restrict__ b1,
                                                            const bf16x8* __restrict__ w2t_hi, const bf16x8* __restrict__ w2t_lo,
                                                            const bf16x8* __restrict__ w1t_hi, const bf16x8* __restrict__ w1t_lo,
                                                            float* __restrict__ gxn) {
    constexpr int LD = C + CNX_KPAD, KK = C / 16, CT = C / 32, JB = C / 8;
    __shared__ __attribute__((aligned(16))) bf16_t smem[4 * CNX_TP * LD];
    static_assert(4 * CNX_TP * LD * 2 >= 4 * 32 * 36 * 4, "the reduction buffer reuses the operand planes");
    bf16_t* const sx_hi = smem;
    bf16_t* const sx_lo = sx_hi + CNX_TP * LD;
    bf16_t* const sg_hi = sx_lo + CNX_TP * LD;
    bf16_t* const sg_lo = sg_hi + CNX_TP * LD;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
    const long long p0 = (long long)blockIdx.x * CNX_TP;
    load_planes<C, 256>(x_hi, x_lo, p0, P, sx_hi, sx_lo, t);
    load_rows_split<C, 256>(gy, C, 0, row_scale, ppi, p0, P, sg_hi, sg_lo, t);
    __syncthreads();
    f32x16 y[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) y[ct][i] = 0.f;
    const int boff = r * LD + 8 * h;
#pragma unroll 1
    for (int jb = wave; jb < JB; jb += 4) {
        f32x16 hacc, ga;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bv = *(const f32x4*)(b1 + jb * 32 + 8 * q + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                hacc[4 * q + i] = bv[i];
                ga[4 * q + i] = 0.f;
            }
        }
        const size_t woff = (size_t)jb * KK * 64 + lane;
#pragma unroll 4
        for (int kk = 0; kk < KK; ++kk)
            mfma3(hacc, w1_hi[woff + kk * 64], w1_lo[woff + kk * 64], *(const bf16x8*)(sx_hi + boff + kk * 16),
                  *(const bf16x8*)(sx_lo + boff + kk * 16));
#pragma unroll 4
        for (int kk = 0; kk < KK; ++kk)
            mfma3(ga, w2t_hi[woff + kk * 64], w2t_lo[woff + kk * 64], *(const bf16x8*)(sg_hi + boff + kk * 16),
                  *(const bf16x8*)(sg_lo + boff + kk * 16));
        bf16x8 g_hi[2], g_lo[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            bf16_t hi, lo;
            split_bf16(ga[i] * gelu_grad(hacc[i]), hi, lo);
            g_hi[i >> 3][i & 7] = (short)hi;
            g_lo[i >> 3][i & 7] = (short)lo;
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const size_t coff = ((size_t)(jb * 2 + tt) * CT) * 64 + lane;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) mfma3(y[ct], w1t_hi[coff + ct * 64], w1t_lo[coff + ct * 64], g_hi[tt], g_lo[tt]);
        }
    }
    float* const red = (float*)smem;       // [4 waves][32 pixels][36]
    const int epx = t >> 3, ec = (t & 7) * 4;
    const long long ep = p0 + epx;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = {y[ct][4 * q], y[ct][4 * q + 1], y[ct][4 * q + 2], y[ct][4 * q + 3]};
            *(f32x4*)(red + (wave * 32 + r) * 36 + 8 * q + 4 * h) = v;
        }
        __syncthreads();
        if (ep < P) {
            const f32x4 s0 = *(const f32x4*)(red + (0 * 32 + epx) * 36 + ec), s1 = *(const f32x4*)(red + (1 * 32 + epx) * 36 + ec);
            const f32x4 s2 = *(const f32x4*)(red + (2 * 32 + epx) * 36 + ec), s3 = *(const f32x4*)(red + (3 * 32 + epx) * 36 + ec);
            *(f32x4*)(gxn + (size_t)ep * C + ct * 32 + ec) = ((s0 + s1) + s2) + s3;
        }
    }
}

// ----------------------------------------------------------------------------------------------- MLP: weight gradients
// grid (4C / 32 hidden blocks, pixel slices), 192 threads: the three waves recompute the block's h^T and ga^T each (pixel on
// the accumulator row, hidden feature on the lane) and split the C / 32 channel tiles of the two K = pixels products:
//   gW1^T[k][j] += sum_p xn[p][k] gh[p][j]      A = xn^T gathered from LDS in acc_row pixel order, B = gh^T's registers
//   G[c][j]     += sum_p gs[p][c] a[p][j]       A = gs^T gathered likewise,                          B = a^T's registers
// Partials per slice s: pw1 [S][4C][C], pg [S][C][4C], pb1 [S][4C].
template <int C>
__global__ __launch_bounds__(192, (C <= 192 ? 2 : 1)) void cnx_mlp_wgrad_kernel(const bf16_t* __restrict__ x_hi, const bf16_t* __restrict__ x_lo,
                                                            const float* __restrict__ gy, const float* __restrict__ row_scale,
                                                            long long ppi, long long P, const bf16x8* __restrict__ w1_hi,
                                                            const bf16x8* __restrict__ w1_lo, const float* __restrict__ b1,
                                                            const bf16x8* __restrict__ w2t_hi, const bf16x8* __restrict__ w2t_lo,
                                                            float* __restrict__ pw1, float* __restrict__ pg, float* __restrict__ pb1) {
    constexpr int LD = C + CNX_KPAD, KK = C / 16, CT = C / 32, NCT = CT / 3, H4 = 4 * C;
    __shared__ __attribute__((aligned(16))) bf16_t smem[4 * CNX_TP * LD];
    bf16_t* const sx_hi = smem;
    bf16_t* const sx_lo = sx_hi + CNX_TP * LD;
    bf16_t* const sg_hi = sx_lo + CNX_TP * LD;
    bf16_t* const sg_lo = sg_hi + CNX_TP * LD;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
    const int jb = blockIdx.x, s = blockIdx.y;
    const long long ntiles = (P + CNX_TP - 1) / CNX_TP;
    const long long tile0 = (long long)s * CNX_SLICE_TILES;
    const long long tile1 = tile0 + CNX_SLICE_TILES < ntiles ? tile0 + CNX_SLICE_TILES : ntiles;
    f32x16 aw1[NCT], ag[NCT];
#pragma unroll
    for (int n = 0; n < NCT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            aw1[n][i] = 0.f;
            ag[n][i] = 0.f;
        }
    float sb1 = 0.f;
    const float bj = b1[jb * 32 + r];
    const int aoff = r * LD + 8 * h;
    const size_t woff = (size_t)jb * KK * 64 + lane;
#pragma unroll 1
    for (long long tile = tile0; tile < tile1; ++tile) {
        const long long p0 = tile * CNX_TP;
        __syncthreads();                   // the previous tile's planes have been read
        load_planes<C, 192>(x_hi, x_lo, p0, P, sx_hi, sx_lo, t);
        load_rows_split<C, 192>(gy, C, 0, row_scale, ppi, p0, P, sg_hi, sg_lo, t);
        __syncthreads();
        f32x16 hT, gaT;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            hT[i] = bj;
            gaT[i] = 0.f;
        }
#pragma unroll 4
        for (int kk = 0; kk < KK; ++kk)
            mfma3(hT, *(const bf16x8*)(sx_hi + aoff + kk * 16), *(const bf16x8*)(sx_lo + aoff + kk * 16), w1_hi[woff + kk * 64],
                  w1_lo[woff + kk * 64]);
#pragma unroll 4
        for (int kk = 0; kk < KK; ++kk)
            mfma3(gaT, *(const bf16x8*)(sg_hi + aoff + kk * 16), *(const bf16x8*)(sg_lo + aoff + kk * 16), w2t_hi[woff + kk * 64],
                  w2t_lo[woff + kk * 64]);
        bf16x8 a_hi[2], a_lo[2], g_hi[2], g_lo[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float hv = hT[i];
            const float phi = 0.5f * (1.f + erff(hv * 0.70710678118654752440f));      // one erf serves GELU and GELU'
            const float gh = gaT[i] * (phi + hv * 0.39894228040143267794f * expf(-0.5f * hv * hv));
            sb1 += gh;
            bf16_t hi, lo;
            split_bf16(gh, hi, lo);
            g_hi[i >> 3][i & 7] = (short)hi;
            g_lo[i >> 3][i & 7] = (short)lo;
            split_bf16(hv * phi, hi, lo);
            a_hi[i >> 3][i & 7] = (short)hi;
            a_lo[i >> 3][i & 7] = (short)lo;
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int n = 0; n < NCT; ++n) {
                const int col = (wave + 3 * n) * 32 + r;
                mfma3(aw1[n], gather_px<true>(sx_hi, LD, col, tt, h), gather_px<true>(sx_lo, LD, col, tt, h), g_hi[tt], g_lo[tt]);
                mfma3(ag[n], gather_px<true>(sg_hi, LD, col, tt, h), gather_px<true>(sg_lo, LD, col, tt, h), a_hi[tt], a_lo[tt]);
            }
    }
    const int j = jb * 32 + r;
#pragma unroll
    for (int n = 0; n < NCT; ++n) {
        const int c0 = (wave + 3 * n) * 32;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = {aw1[n][4 * q], aw1[n][4 * q + 1], aw1[n][4 * q + 2], aw1[n][4 * q + 3]};
            *(f32x4*)(pw1 + ((size_t)s * H4 + j) * C + c0 + 8 * q + 4 * h) = v;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) pg[((size_t)s * C + c0 + acc_row(i, h)) * H4 + j] = ag[n][i];
    }
    const float tot = sb1 + __shfl_xor(sb1, 32, 64);
    if (wave == 0 && h == 0) pb1[(size_t)s * H4 + j] = tot;
}

// part[s][c] = sum over the pixels p of slice s of g[p][c] * row_scale[p / ppi]; grid (slices, width / 32).  Thread (cl, q = t >> 5)
// adds the pixels q, q + 8, ... of the slice for column cl of the chunk; the eight sums are then added in q order.
__global__ __launch_bounds__(256) void cnx_colsum_kernel(const float* __restrict__ g, int width, const float* __restrict__ row_scale,
                                                         long long ppi, long long P, float* __restrict__ part) {
    __shared__ float red[8][32];
    const int cl = threadIdx.x & 31, q = threadIdx.x >> 5, c = blockIdx.y * 32 + cl;
    const long long pa = (long long)blockIdx.x * CNX_SLICE_PIXELS;
    const long long pb = pa + CNX_SLICE_PIXELS < P ? pa + CNX_SLICE_PIXELS : P;
    float s = 0.f;
    for (long long p = pa + q; p < pb; p += 8) {
        float v = g[(size_t)p * width + c];
        if (row_scale) v *= row_scale[p / ppi];
        s += v;
    }
    red[q][cl] = s;
    __syncthreads();
    if (q == 0) {
        float a = red[0][cl];
#pragma unroll
        for (int i = 1; i < 8; ++i) a += red[i][cl];
        part[(size_t)blockIdx.x * width + c] = a;
    }
}

// Many partials are first summed in groups of CNX_REDUCE_GROUP consecutive ones, in place: group g leaves its sum (parts in
// order) in its first slot.  reduce_into repeats this until at most CNX_REDUCE_GROUP remain; the order is fixed by the count.
__global__ __launch_bounds__(256) void cnx_group_sum_kernel(float* __restrict__ part, int nparts, long long pstride, long long n,
                                                            int group) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int q0 = blockIdx.y * group, q1 = q0 + group < nparts ? q0 + group : nparts;
    float s = 0.f;
    for (int q = q0; q < q1; ++q) s += part[(size_t)q * pstride + i];
    part[(size_t)q0 * pstride + i] = s;
}

// dst[perm(i)] += sum_q part[q * pstride + i], q in order.  perm 0: i.  perm 1: [rows][cols] -> [cols][rows] (pa = rows,
// pb = cols).  perm 2: the downsample weight, [2C][(kp, c)] -> Conv2d's [2C][c][kp] (pa = C).
__global__ __launch_bounds__(256) void cnx_reduce_kernel(const float* __restrict__ part, int nparts, long long pstride, long long n,
                                                         float* __restrict__ dst, int perm, int pa, int pb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int q = 0; q < nparts; ++q) s += part[(size_t)q * pstride + i];
    long long d = i;
    if (perm == 1) d = (i % pb) * pa + i / pb;
    else if (perm == 2) {
        const long long o = i / (4 * pa), k = i % (4 * pa);
        d = o * 4 * pa + (k % pa) * 4 + k / pa;
    }
    dst[d] += s;
}

// One workgroup per channel c: gW2[c][:] += ls[c] G[c][:], g_ls[c] += sum_j W2[c][j] G[c][j] + b2[c] cs[c], gb2[c] += ls[c] cs[c]
__global__ __launch_bounds__(256) void cnx_mlp_finish_kernel(const float* __restrict__ pg, const float* __restrict__ pcs, int S, int C,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             const float* __restrict__ ls, float* __restrict__ gw2,
                                                             float* __restrict__ gb2, float* __restrict__ gls) {
    __shared__ float red[256];
    const int c = blockIdx.x, t = threadIdx.x, H4 = 4 * C;
    const float lsc = ls[c];
    float dot = 0.f;
    for (int j = t; j < H4; j += 256) {
        float g = 0.f;
        for (int s = 0; s < S; ++s) g += pg[((size_t)s * C + c) * H4 + j];
        gw2[(size_t)c * H4 + j] += lsc * g;
        dot = fmaf(w2[(size_t)c * H4 + j], g, dot);
    }
    red[t] = dot;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        float cs = 0.f;
        for (int s = 0; s < S; ++s) cs += pcs[(size_t)s * C + c];
        gls[c] += red[0] + b2[c] * cs;
        gb2[c] += lsc * cs;
    }
}

// --------------------------------------------------------------------------- LayerNorm backward behind the depthwise conv
// The forward kernel's conv and statistics, recomputed from the block input; then per pixel
//   gxh = gxn gamma, gz = rstd (gxh - mean_c gxh - xhat mean_c(gxh xhat)).
// Partials per workgroup: pln [blocks][3][C] = g_gamma (sum gxn xhat), g_beta (sum gxn), g_dwbias (sum gz), summed over the
// workgroup's pixels in a fixed order.
template <int C>
__global__ __launch_bounds__(256) void cnx_dwln_gz_kernel(const float* __restrict__ x, const float* __restrict__ gxn, int h, int w,
                                                          int tiles_y, int tiles_x, const float* __restrict__ wt,
                                                          const float* __restrict__ bias, const float* __restrict__ g, float eps,
                                                          float* __restrict__ gz, float* __restrict__ pln) {
    constexpr int NK = C / 32;
    __shared__ __attribute__((aligned(16))) float tile[10][14][32];
    __shared__ float wl[49][32];
    __shared__ float red[8][3][C];
    const int t = threadIdx.x, cl = t & 31, col = t >> 5;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y, img = bid / tiles_y;
    const int y0 = ty * 4, x0 = tx * 8;
    const float* ximg = x + (size_t)img * h * w * C;
    float conv[4][NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        __syncthreads();
        for (int e = t; e < 140 * 8; e += 256) {
            const int q = e & 7, pxi = e >> 3, yy = pxi / 14, xx = pxi - yy * 14;
            const int gy = y0 + yy - 3, gx = x0 + xx - 3;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = *(const f32x4*)(ximg + ((size_t)gy * w + gx) * C + k * 32 + q * 4);
            *(f32x4*)&tile[yy][xx][q * 4] = v;
        }
        for (int e = t; e < 49 * 32; e += 256) wl[e >> 5][e & 31] = wt[(e >> 5) * C + k * 32 + (e & 31)];
        __syncthreads();
        float acc[4];
        const float bv = bias[k * 32 + cl];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = bv;
#pragma unroll 1
        for (int kx = 0; kx < 7; ++kx) {
            float v[10];
#pragma unroll
            for (int rr = 0; rr < 10; ++rr) v[rr] = tile[rr][col + kx][cl];
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                const float wv = wl[ky * 7 + kx][cl];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(wv, v[i + ky], acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) conv[i][k] = acc[i];
    }
    float sgam[NK], sbet[NK], sdb[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) sgam[k] = sbet[k] = sdb[k] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) s += conv[i][k];
        const float mean = half_sum(s) * (1.f / C);
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            conv[i][k] -= mean;
            q = fmaf(conv[i][k], conv[i][k], q);
        }
        const float rstd = 1.f / sqrtf(half_sum(q) * (1.f / C) + eps);
        const int py = y0 + i, px = x0 + col;
        const bool ok = py < h && px < w;
        const size_t p = ((size_t)img * h + (ok ? py : 0)) * w + (ok ? px : 0);
        float gv[NK], m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = k * 32 + cl;
            conv[i][k] *= rstd;                                   // xhat
            gv[k] = ok ? gxn[p * C + c] : 0.f;
            const float gxh = gv[k] * g[c];
            m1 += gxh;
            m2 = fmaf(gxh, conv[i][k], m2);
        }
        m1 = half_sum(m1) * (1.f / C);
        m2 = half_sum(m2) * (1.f / C);
        if (ok) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int c = k * 32 + cl;
                const float z = rstd * (gv[k] * g[c] - m1 - conv[i][k] * m2);
                gz[p * C + c] = z;
                sgam[k] = fmaf(gv[k], conv[i][k], sgam[k]);
                sbet[k] += gv[k];
                sdb[k] += z;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        red[col][0][k * 32 + cl] = sgam[k];
        red[col][1][k * 32 + cl] = sbet[k];
        red[col][2][k * 32 + cl] = sdb[k];
    }
    __syncthreads();
    for (int e = t; e < 3 * C; e += 256) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += (&red[q][0][0])[e];
        pln[(size_t)blockIdx.x * 3 * C + e] = s;
    }
}

// ------------------------------------------------------------------------ depthwise 7x7: data and weight gradients
// gx = gy + sum_tap gz[p - tap] dw[tap] (the forward's conv on gz with the taps flipped) and the partials of
// g_dw[tap][c] = sum_p gz[p][c] x[p + tap][c].  A workgroup walks the channel chunks; per chunk it sweeps its CNX_DW_TILES
// consecutive 4 x 8 tiles with the x and gz windows (addressed by (image, y, x), zeros outside the image) in LDS.  Phase 1:
// thread (cl, col) computes the 4 gx of its column.  Phase 2: thread (cl, ky = t >> 5 < 7) adds the tile's 32 pixels into its
// 7 taps of row ky.  pdw: [workgroups][49][C].
template <int C>
__global__ __launch_bounds__(256) void cnx_dw_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gz,
                                                         const float* __restrict__ gy, int h, int w, int tiles_y, int tiles_x,
                                                         long long ntiles, const float* __restrict__ wt, float* __restrict__ gx,
                                                         float* __restrict__ pdw) {
    constexpr int NK = C / 32;
    __shared__ __attribute__((aligned(16))) float tx_[10][14][32];
    __shared__ __attribute__((aligned(16))) float tg_[10][14][32];
    __shared__ float wl[49][32];
    const int t = threadIdx.x, cl = t & 31, col = t >> 5;
    const long long tile0 = (long long)blockIdx.x * CNX_DW_TILES;
    const long long tile1 = tile0 + CNX_DW_TILES < ntiles ? tile0 + CNX_DW_TILES : ntiles;
#pragma unroll 1
    for (int k = 0; k < NK; ++k) {
        float dacc[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) dacc[i] = 0.f;
        __syncthreads();
        for (int e = t; e < 49 * 32; e += 256) wl[e >> 5][e & 31] = wt[(e >> 5) * C + k * 32 + (e & 31)];
#pragma unroll 1
        for (long long tile = tile0; tile < tile1; ++tile) {
            long long bid = tile;
            const int txi = (int)(bid % tiles_x);
            bid /= tiles_x;
            const int tyi = (int)(bid % tiles_y), img = (int)(bid / tiles_y);
            const int y0 = tyi * 4, x0 = txi * 8;
            const size_t ibase = (size_t)img * h * w;
            __syncthreads();
            for (int e = t; e < 140 * 8; e += 256) {
                const int q = e & 7, pxi = e >> 3, yy = pxi / 14, xx = pxi - yy * 14;
                const int py = y0 + yy - 3, px = x0 + xx - 3;
                f32x4 v = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
                if (py >= 0 && py < h && px >= 0 && px < w) {
                    const size_t off = (ibase + (size_t)py * w + px) * C + k * 32 + q * 4;
                    v = *(const f32x4*)(x + off);
                    u = *(const f32x4*)(gz + off);
                }
                *(f32x4*)&tx_[yy][xx][q * 4] = v;
                *(f32x4*)&tg_[yy][xx][q * 4] = u;
            }
            __syncthreads();
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int kx = 0; kx < 7; ++kx) {
                float v[10];
#pragma unroll
                for (int rr = 0; rr < 10; ++rr) v[rr] = tg_[rr][col + kx][cl];
#pragma unroll
                for (int ky = 0; ky < 7; ++ky) {
                    const float wv = wl[48 - (ky * 7 + kx)][cl];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = fmaf(wv, v[i + ky], acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int py = y0 + i, px = x0 + col;
                if (py < h && px < w) {
                    const size_t off = (ibase + (size_t)py * w + px) * C + k * 32 + cl;
                    gx[off] = gy[off] + acc[i];
                }
            }
            if (col < 7) {                 // col is this thread's tap row ky in phase 2
#pragma unroll 1
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c8 = 0; c8 < 8; ++c8) {
                        const float gzv = tg_[3 + i][3 + c8][cl];
#pragma unroll
                        for (int kx = 0; kx < 7; ++kx) dacc[kx] = fmaf(gzv, tx_[i + col][c8 + kx][cl], dacc[kx]);
                    }
            }
        }
        if (col < 7) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) pdw[((size_t)blockIdx.x * 49 + col * 7 + kx) * C + k * 32 + cl] = dacc[kx];
        }
    }
}

// ------------------------------------------------------------------------------------------------ plain LayerNorm backward
// Eight lanes per pixel, 32 pixels per workgroup (the downsample forward's arrangement).  gx may alias gxn.  A pixel outside the
// covered area (y >= hc or x >= wc: the odd last row / column a stride-2 conv drops) gets gx = 0 exactly and contributes
// nothing.  pln: [workgroups][2][C] = g_gamma, g_beta.
template <int C>
__global__ __launch_bounds__(256) void cnx_ln_bwd_kernel(const float* __restrict__ x, const float* gxn, int h, int w, int hc, int wc,
                                                         long long P, const float* __restrict__ g, float eps, float* gx,
                                                         float* __restrict__ pln) {
    constexpr int NV = C / 32;
    __shared__ float red[32][C + 1];
    const int t = threadIdx.x, lpx = t >> 3, sl = t & 7;
    const long long p = (long long)blockIdx.x * 32 + lpx;
    bool ok = p < P;
    if (ok) {
        const int rem = (int)(p % ((long long)h * w));
        ok = rem / w < hc && rem % w < wc;
    }
    f32x4 v[NV], gv[NV];
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
        v[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        gv[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) {
            v[m] = *(const f32x4*)(x + (size_t)p * C + (sl + 8 * m) * 4);
            gv[m] = *(const f32x4*)(gxn + (size_t)p * C + (sl + 8 * m) * 4);
        }
        s += (v[m][0] + v[m][1]) + (v[m][2] + v[m][3]);
    }
    const float mean = oct_sum(s) * (1.f / C);
    float q = 0.f;
#pragma unroll
    for (int m = 0; m < NV; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[m][i] -= mean;
            q = fmaf(v[m][i], v[m][i], q);
        }
    const float rstd = 1.f / sqrtf(oct_sum(q) * (1.f / C) + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
        const f32x4 gam = *(const f32x4*)(g + (sl + 8 * m) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[m][i] *= rstd;                                      // xhat
            const float gxh = gv[m][i] * gam[i];
            m1 += gxh;
            m2 = fmaf(gxh, v[m][i], m2);
        }
    }
    m1 = oct_sum(m1) * (1.f / C);
    m2 = oct_sum(m2) * (1.f / C);
    if (p < P) {
#pragma unroll
        for (int m = 0; m < NV; ++m) {
            const f32x4 gam = *(const f32x4*)(g + (sl + 8 * m) * 4);
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = rstd * (gv[m][i] * gam[i] - m1 - v[m][i] * m2);
            }
            *(f32x4*)(gx + (size_t)p * C + (sl + 8 * m) * 4) = o;
        }
    }
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < NV; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[lpx][(sl + 8 * m) * 4 + i] = which == 0 ? gv[m][i] * v[m][i] : gv[m][i];
        __syncthreads();
        for (int c = t; c < C; c += 256) {
            float a = 0.f;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) a += red[r][c];
            pln[((size_t)blockIdx.x * 2 + which) * C + c] = a;
        }
    }
}

// ------------------------------------------------------------------------------------------ downsample: data gradient
// gxn_patch[k][p] = sum_o W[o][k] gout[p][o] per 32 output pixels: A = W^T in fragment order ([4C / 32][2C / 16][64][8]), B = the
// gout tile's split planes in LDS.  The k block kb is 32 channels of input pixel (2 oy + ky, 2 ox + kx), kp = ky * 2 + kx =
// kb / (C / 32); the result goes straight to that pixel of gxin [n][h][w][C].
template <int C>
__global__ __launch_bounds__(256) void cnx_down_dgrad_kernel(const float* __restrict__ gout, int h, int w, int ho, int wo, long long P,
                                                             const bf16x8* __restrict__ wt_hi, const bf16x8* __restrict__ wt_lo,
                                                             float* __restrict__ gxin) {
    constexpr int N2 = 2 * C, LD = N2 + CNX_KPAD, KK = N2 / 16, KB = 4 * C / 32, CB = C / 32;
    __shared__ __attribute__((aligned(16))) bf16_t sg_hi[CNX_TP * LD];
    __shared__ __attribute__((aligned(16))) bf16_t sg_lo[CNX_TP * LD];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, hh = lane >> 5;
    const long long p0 = (long long)blockIdx.x * CNX_TP;
    load_rows_split<N2, 256>(gout, N2, 0, nullptr, 1, p0, P, sg_hi, sg_lo, t);
    __syncthreads();
    const long long op = p0 + r;
    long long img = 0;
    int oy = 0, ox = 0;
    if (op < P) {
        img = op / ((long long)ho * wo);
        const int rem = (int)(op - img * ho * wo);
        oy = rem / wo;
        ox = rem - oy * wo;
    }
    const int boff = r * LD + 8 * hh;
#pragma unroll 1
    for (int kb = wave; kb < KB; kb += 4) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const size_t woff = (size_t)kb * KK * 64 + lane;
#pragma unroll 4
        for (int kk = 0; kk < KK; ++kk)
            mfma3(acc, wt_hi[woff + kk * 64], wt_lo[woff + kk * 64], *(const bf16x8*)(sg_hi + boff + kk * 16),
                  *(const bf16x8*)(sg_lo + boff + kk * 16));
        if (op < P) {
            const int kp = kb / CB, c0 = (kb - kp * CB) * 32;
            float* dst = gxin + (((size_t)img * h + (2 * oy + (kp >> 1))) * w + (2 * ox + (kp & 1))) * C + c0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                *(f32x4*)(dst + 8 * q + 4 * hh) = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- downsample: weight gradient
// gW[o][k] += sum_P gout[P][o] xn_patch[P][k], K = output pixels.  grid (2C / 32 output blocks, 4C / 384 K chunks, pixel slices).
// Per tile the chunk is normalised into LDS as in the forward; both operands are gathered with the pixel on the k slots.
// pw: [slices][2C][4C] with k = (ky * 2 + kx) * C + c.
template <int C>
__global__ __launch_bounds__(256) void cnx_down_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gout, int h, int w,
                                                             int ho, int wo, long long P, const float* __restrict__ g,
                                                             const float* __restrict__ b, float eps, float* __restrict__ pw) {
    constexpr int KC = 384, LD = KC + CNX_KPAD, IPP = KC / C, NV = C / 32, LDG = 32 + CNX_KPAD;
    __shared__ __attribute__((aligned(16))) bf16_t sx_hi[CNX_TP * LD];
    __shared__ __attribute__((aligned(16))) bf16_t sx_lo[CNX_TP * LD];
    __shared__ __attribute__((aligned(16))) bf16_t so_hi[CNX_TP * LDG];
    __shared__ __attribute__((aligned(16))) bf16_t so_lo[CNX_TP * LDG];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, hh = lane >> 5;
    const int nt = blockIdx.x, ch = blockIdx.y, s = blockIdx.z;
    const int lpx = t >> 3, sl = t & 7;
    const long long ntiles = (P + CNX_TP - 1) / CNX_TP;
    const long long tile0 = (long long)s * CNX_SLICE_TILES;
    const long long tile1 = tile0 + CNX_SLICE_TILES < ntiles ? tile0 + CNX_SLICE_TILES : ntiles;
    f32x16 acc[3];
#pragma unroll
    for (int n = 0; n < 3; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 1
    for (long long tile = tile0; tile < tile1; ++tile) {
        const long long p0 = tile * CNX_TP, lp = p0 + lpx;
        long long img = 0;
        int oy = 0, ox = 0;
        if (lp < P) {
            img = lp / ((long long)ho * wo);
            const int rem = (int)(lp - img * ho * wo);
            oy = rem / wo;
            ox = rem - oy * wo;
        }
        __syncthreads();
        load_rows_split<32, 256>(gout, 2 * C, nt * 32, nullptr, 1, p0, P, so_hi, so_lo, t);
#pragma unroll 1
        for (int sub = 0; sub < IPP; ++sub) {
            const int kp = ch * IPP + sub, ky = kp >> 1, kx = kp & 1;
            f32x4 v[NV];
            float sum = 0.f;
            if (lp < P) {
                const float* src = x + (((size_t)img * h + (2 * oy + ky)) * w + (2 * ox + kx)) * C;
#pragma unroll
                for (int m = 0; m < NV; ++m) {
                    v[m] = *(const f32x4*)(src + (sl + 8 * m) * 4);
                    sum += (v[m][0] + v[m][1]) + (v[m][2] + v[m][3]);
                }
            } else {
#pragma unroll
                for (int m = 0; m < NV; ++m) v[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float mean = oct_sum(sum) * (1.f / C);
            float q = 0.f;
#pragma unroll
            for (int m = 0; m < NV; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[m][i] -= mean;
                    q = fmaf(v[m][i], v[m][i], q);
                }
            const float rstd = 1.f / sqrtf(oct_sum(q) * (1.f / C) + eps);
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const int c = (sl + 8 * m) * 4;
                const f32x4 gv = *(const f32x4*)(g + c), bv = *(const f32x4*)(b + c);
                bf16_t hi[4], lo[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) split_bf16(lp < P ? fmaf(v[m][i] * rstd, gv[i], bv[i]) : 0.f, hi[i], lo[i]);
                *(u32x2*)(sx_hi + lpx * LD + sub * C + c) = u32x2{pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
                *(u32x2*)(sx_lo + lpx * LD + sub * C + c) = u32x2{pack2(lo[0], lo[1]), pack2(lo[2], lo[3])};
            }
        }
        __syncthreads();
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const bf16x8 ah = gather_px<false>(so_hi, LDG, r, tt, hh), al = gather_px<false>(so_lo, LDG, r, tt, hh);
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int col = (wave + 4 * n) * 32 + r;
                mfma3(acc[n], ah, al, gather_px<false>(sx_hi, LD, col, tt, hh), gather_px<false>(sx_lo, LD, col, tt, hh));
            }
        }
    }
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        const int k = ch * KC + (wave + 4 * n) * 32 + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) pw[((size_t)s * 2 * C + nt * 32 + acc_row(i, hh)) * (4 * C) + k] = acc[n][i];
    }
}

// ------------------------------------------------------------------------------------------------------------------ stem
// The forward's conv and LayerNorm statistics recomputed per 32-pixel tile, LayerNorm backward -> gz (LDS), then
// gW[o][idx] += sum_px gz[px][o] patch[px][idx]: thread t owns the 18 outputs t + 256 u.  A workgroup sweeps CNX_STEM_TILES
// tiles and writes one partial: [96 x 48 gW][96 g_bias][96 g_gamma][96 g_beta].
// LOAD: the image source, as in cnx_stem_kernel (convnext_common.hpp).
template <class LOAD>
__global__ __launch_bounds__(256) void cnx_stem_bwd_kernel(const LOAD ld, int ho, int wo, long long P, const float* __restrict__ wt,
                                                           const float* __restrict__ bias, const float* __restrict__ g, float eps,
                                                           const float* __restrict__ gout, float* __restrict__ part) {
    __shared__ float xin[32][48];
    __shared__ float sgz[32][97];
    __shared__ float red[8][3][96];
    const int t = threadIdx.x, cl = t & 31, pg = t >> 5;
    const long long ntiles = (P + 31) / 32;
    const long long tile0 = (long long)blockIdx.x * CNX_STEM_TILES;
    const long long tile1 = tile0 + CNX_STEM_TILES < ntiles ? tile0 + CNX_STEM_TILES : ntiles;
    float aw[18];
#pragma unroll
    for (int u = 0; u < 18; ++u) aw[u] = 0.f;
    float sgam[3] = {0.f, 0.f, 0.f}, sbet[3] = {0.f, 0.f, 0.f}, sbi[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (long long tile = tile0; tile < tile1; ++tile) {
        const long long p0 = tile * 32;
        __syncthreads();
        for (int e = t; e < 32 * 48; e += 256) {
            const int px = e / 48, idx = e % 48;
            const long long p = p0 + px;
            float v = 0.f;
            if (p < P) {
                const int ci = idx >> 4, ky = (idx >> 2) & 3, kx = idx & 3;
                const long long img = p / ((long long)ho * wo);
                const int rem = (int)(p - img * ho * wo), oy = rem / wo, ox = rem - oy * wo;
                v = ld(img, ci, 4 * oy + ky, 4 * ox + kx);
            }
            xin[px][idx] = v;
        }
        __syncthreads();
        float acc[4][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float bv = bias[cl + 32 * k];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][k] = bv;
        }
        for (int idx = 0; idx < 48; ++idx) {
            float wv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) wv[k] = wt[idx * 96 + cl + 32 * k];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float xv = xin[pg * 4 + i][idx];
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[i][k] = fmaf(xv, wv[k], acc[i][k]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float mean = half_sum(acc[i][0] + acc[i][1] + acc[i][2]) * (1.f / 96.f);
            float d[3], q = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                d[k] = acc[i][k] - mean;
                q = fmaf(d[k], d[k], q);
            }
            const float rstd = 1.f / sqrtf(half_sum(q) * (1.f / 96.f) + eps);
            const long long p = p0 + pg * 4 + i;
            float gv[3], m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = cl + 32 * k;
                d[k] *= rstd;
                gv[k] = p < P ? gout[p * 96 + c] : 0.f;
                const float gxh = gv[k] * g[c];
                m1 += gxh;
                m2 = fmaf(gxh, d[k], m2);
            }
            m1 = half_sum(m1) * (1.f / 96.f);
            m2 = half_sum(m2) * (1.f / 96.f);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = cl + 32 * k;
                const float z = p < P ? rstd * (gv[k] * g[c] - m1 - d[k] * m2) : 0.f;
                sgz[pg * 4 + i][c] = z;
                sgam[k] = fmaf(gv[k], d[k], sgam[k]);
                sbet[k] += gv[k];
                sbi[k] += z;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 18; ++u) {
            const int e = t + 256 * u, o = e / 48, idx = e - o * 48;
            float a = aw[u];
            for (int px = 0; px < 32; ++px) a = fmaf(sgz[px][o], xin[px][idx], a);
            aw[u] = a;
        }
    }
    float* const dst = part + (size_t)blockIdx.x * CNX_STEM_PART;
#pragma unroll
    for (int u = 0; u < 18; ++u) dst[t + 256 * u] = aw[u];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        red[pg][0][cl + 32 * k] = sbi[k];
        red[pg][1][cl + 32 * k] = sgam[k];
        red[pg][2][cl + 32 * k] = sbet[k];
    }
    __syncthreads();
    for (int e = t; e < 3 * 96; e += 256) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += (&red[q][0][0])[e];
        dst[96 * 48 + e] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
inline long long slices_of(long long P) { return (cnx_pad(P) / CNX_TP + CNX_SLICE_TILES - 1) / CNX_SLICE_TILES; }
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
inline long long mlp_bwd_floats(long long P, int C) { return slices_of(P) * (8ll * C * C + 4 * C + C); }
inline long long dwln_tiles(int n, int h, int w) { return (long long)n * ((h + 3) / 4) * ((w + 7) / 8); }
inline long long dwln_bwd_floats(int n, int h, int w, int C) {
    const long long tiles = dwln_tiles(n, h, w);
    return (long long)n * h * w * C + tiles * 3 * C + ceil_div(tiles, CNX_DW_TILES) * 49 * C;
}
inline long long down_bwd_floats(int n, int h, int w, int C) {
    const long long Po = (long long)n * (h / 2) * (w / 2);
    if (Po <= 0) return 0;
    return slices_of(Po) * (8ll * C * C + 2 * C) + ceil_div((long long)n * h * w, 32) * 2 * C;
}
inline long long stem_bwd_floats(long long P) { return ceil_div(ceil_div(P, 32), CNX_STEM_TILES) * CNX_STEM_PART; }

inline void reduce_into(hipStream_t s, float* part, long long nparts, long long pstride, long long n, float* dst, int perm = 0,
                        int pa = 0, int pb = 0) {
    while (nparts > CNX_REDUCE_GROUP) {
        const long long groups = ceil_div(nparts, CNX_REDUCE_GROUP);
        hipLaunchKernelGGL(cnx_group_sum_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)groups), dim3(256), 0, s, part, (int)nparts,
                           pstride, n, CNX_REDUCE_GROUP);
        nparts = groups;
        pstride *= CNX_REDUCE_GROUP;
    }
    hipLaunchKernelGGL(cnx_reduce_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, part, (int)nparts, pstride, n, dst, perm,
                       pa, pb);
}

}  // namespace

extern "C" {

int64_t agp_cnx_bwd_slice_pixels(void) { return CNX_SLICE_PIXELS; }

int64_t agp_cnx_bwd_workspace_bytes(int n, int h, int w, int C) {
    if (!cnx_map_ok(n, h, w) || !cnx_c_host_ok(C)) return -1;
    long long f = mlp_bwd_floats((long long)n * h * w, C);
    const long long a = dwln_bwd_floats(n, h, w, C), b = down_bwd_floats(n, h, w, C);
    if (a > f) f = a;
    if (b > f) f = b;
    if (C == 96) {
        const long long c = stem_bwd_floats((long long)n * h * w);
        if (c > f) f = c;
    }
    return f * 4;
}

int agp_cnx_mlp_bwd(const void* workspace, int64_t workspace_bytes, int64_t P, int C, const float* gy, const float* row_scale,
                    int64_t pixels_per_image, const void* w1_hi, const void* w1_lo, const float* b1, const void* w2t_hi,
                    const void* w2t_lo, const void* w1t_hi, const void* w1t_lo, const float* w2, const float* b2,
                    const float* layer_scale, float* gxn, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_layer_scale,
                    void* bwd_workspace, int64_t bwd_workspace_bytes, void* stream) {
    if (!workspace || !gy || !w1_hi || !w1_lo || !b1 || !w2t_hi || !w2t_lo || !w1t_hi || !w1t_lo || !w2 || !b2 || !layer_scale || !gxn ||
        !g_w1 || !g_b1 || !g_w2 || !g_b2 || !g_layer_scale || !bwd_workspace)
        return AGP_E_BADARG;
    if (P <= 0 || P >= (1ll << 31) / 32 || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    if (row_scale && (pixels_per_image <= 0 || P % pixels_per_image)) return AGP_E_BADARG;
    if (workspace_bytes < 2 * cnx_pad(P) * C * 2 || ((uintptr_t)workspace & 15) || ((uintptr_t)bwd_workspace & 15)) return AGP_E_BADARG;
    if (bwd_workspace_bytes < mlp_bwd_floats(P, C) * 4) return AGP_E_BADARG;
    const bf16_t* const hi = (const bf16_t*)workspace;
    const bf16_t* const lo = hi + cnx_pad(P) * C;
    const long long S = slices_of(P), ppi = pixels_per_image;
    float* const pw1 = (float*)bwd_workspace;
    float* const pg = pw1 + S * 4 * C * C;
    float* const pb1 = pg + S * 4 * C * C;
    float* const pcs = pb1 + S * 4 * C;
    hipStream_t s = (hipStream_t)stream;
    const bf16x8 *a = (const bf16x8*)w1_hi, *b = (const bf16x8*)w1_lo, *c = (const bf16x8*)w2t_hi, *d = (const bf16x8*)w2t_lo;
    const bf16x8 *e = (const bf16x8*)w1t_hi, *f = (const bf16x8*)w1t_lo;
    const dim3 gd((unsigned)(cnx_pad(P) / CNX_TP)), gw((unsigned)(C / 8), (unsigned)S);
    (void)hipGetLastError();
#define CNX_MLPB(CC)                                                                                                                  \
    hipLaunchKernelGGL(cnx_mlp_dgrad_kernel<CC>, gd, dim3(256), 0, s, hi, lo, gy, row_scale, ppi, (long long)P, a, b, b1, c, d, e, f, gxn); \
    hipLaunchKernelGGL(cnx_mlp_wgrad_kernel<CC>, gw, dim3(192), 0, s, hi, lo, gy, row_scale, ppi, (long long)P, a, b, b1, c, d, pw1, pg, pb1)
    if (C == 96) { CNX_MLPB(96); } else if (C == 192) { CNX_MLPB(192); } else { CNX_MLPB(384); }
#undef CNX_MLPB
    hipLaunchKernelGGL(cnx_colsum_kernel, dim3((unsigned)S, (unsigned)(C / 32)), dim3(256), 0, s, gy, C, row_scale, ppi,
                       (long long)P, pcs);
    reduce_into(s, pw1, S, 4ll * C * C, 4ll * C * C, g_w1);
    reduce_into(s, pb1, S, 4ll * C, 4ll * C, g_b1);
    hipLaunchKernelGGL(cnx_mlp_finish_kernel, dim3((unsigned)C), dim3(256), 0, s, pg, pcs, (int)S, C, w2, b2, layer_scale, g_w2, g_b2,
                       g_layer_scale);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_dwconv_ln_bwd(const float* x, const float* gxn, const float* gy, int n, int h, int w, int C, const float* wt,
                          const float* bias, const float* ln_w, float eps, float* gx, float* g_dw, float* g_dwbias, float* g_ln_w,
                          float* g_ln_b, void* bwd_workspace, int64_t bwd_workspace_bytes, void* stream) {
    if (!x || !gxn || !gy || !wt || !bias || !ln_w || !gx || !g_dw || !g_dwbias || !g_ln_w || !g_ln_b || !bwd_workspace) return AGP_E_BADARG;
    if (!cnx_map_ok(n, h, w) || !cnx_c_host_ok(C) || ((uintptr_t)bwd_workspace & 15)) return AGP_E_BADARG;
    if (bwd_workspace_bytes < dwln_bwd_floats(n, h, w, C) * 4) return AGP_E_BADARG;
    const int ty = (h + 3) / 4, tx = (w + 7) / 8;
    const long long tiles = dwln_tiles(n, h, w), nb = ceil_div(tiles, CNX_DW_TILES);
    float* const gz = (float*)bwd_workspace;
    float* const pln = gz + (long long)n * h * w * C;
    float* const pdw = pln + tiles * 3 * C;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
#define CNX_DWB(CC)                                                                                                              \
    hipLaunchKernelGGL(cnx_dwln_gz_kernel<CC>, dim3((unsigned)tiles), dim3(256), 0, s, x, gxn, h, w, ty, tx, wt, bias, ln_w, eps, gz, pln); \
    hipLaunchKernelGGL(cnx_dw_bwd_kernel<CC>, dim3((unsigned)nb), dim3(256), 0, s, x, gz, gy, h, w, ty, tx, tiles, wt, gx, pdw)
    if (C == 96) { CNX_DWB(96); } else if (C == 192) { CNX_DWB(192); } else { CNX_DWB(384); }
#undef CNX_DWB
    reduce_into(s, pln, tiles, 3ll * C, C, g_ln_w);
    reduce_into(s, pln + C, tiles, 3ll * C, C, g_ln_b);
    reduce_into(s, pln + 2 * C, tiles, 3ll * C, C, g_dwbias);
    reduce_into(s, pdw, nb, 49ll * C, 49ll * C, g_dw, 1, 49, C);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_downsample_bwd(const float* x, const float* gout, int n, int h, int w, int C, const float* ln_w, const float* ln_b,
                           float eps, const void* wt_hi, const void* wt_lo, float* gx, float* g_w, float* g_bias, float* g_ln_w,
                           float* g_ln_b, void* bwd_workspace, int64_t bwd_workspace_bytes, void* stream) {
    if (!x || !gout || !ln_w || !ln_b || !wt_hi || !wt_lo || !gx || !g_w || !g_bias || !g_ln_w || !g_ln_b || !bwd_workspace) return AGP_E_BADARG;
    if (!cnx_map_ok(n, h, w) || !cnx_c_host_ok(C) || ((uintptr_t)bwd_workspace & 15)) return AGP_E_BADARG;
    const int ho = h / 2, wo = w / 2;
    if (ho < 1 || wo < 1 || bwd_workspace_bytes < down_bwd_floats(n, h, w, C) * 4) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo, Pin = (long long)n * h * w, S = slices_of(P), nbl = ceil_div(Pin, 32);
    float* const pw = (float*)bwd_workspace;
    float* const pcs = pw + S * 8 * C * C;
    float* const pln = pcs + S * 2 * C;
    hipStream_t s = (hipStream_t)stream;
    const bf16x8 *a = (const bf16x8*)wt_hi, *b = (const bf16x8*)wt_lo;
    const dim3 gd((unsigned)(cnx_pad(P) / CNX_TP)), gw((unsigned)(2 * C / 32), (unsigned)(4 * C / 384), (unsigned)S);
    (void)hipGetLastError();
    // the data gradient lands in gx, which the LayerNorm backward then rewrites in place (uncovered pixels: exactly 0)
#define CNX_DNB(CC)                                                                                                                  \
    hipLaunchKernelGGL(cnx_down_dgrad_kernel<CC>, gd, dim3(256), 0, s, gout, h, w, ho, wo, P, a, b, gx);                               \
    hipLaunchKernelGGL(cnx_ln_bwd_kernel<CC>, dim3((unsigned)nbl), dim3(256), 0, s, x, gx, h, w, 2 * ho, 2 * wo, Pin, ln_w, eps, gx, pln); \
    hipLaunchKernelGGL(cnx_down_wgrad_kernel<CC>, gw, dim3(256), 0, s, x, gout, h, w, ho, wo, P, ln_w, ln_b, eps, pw)
    if (C == 96) { CNX_DNB(96); } else if (C == 192) { CNX_DNB(192); } else { CNX_DNB(384); }
#undef CNX_DNB
    hipLaunchKernelGGL(cnx_colsum_kernel, dim3((unsigned)S, (unsigned)(2 * C / 32)), dim3(256), 0, s, gout, 2 * C,
                       (const float*)nullptr, 1ll, P, pcs);
    reduce_into(s, pw, S, 8ll * C * C, 8ll * C * C, g_w, 2, C, 0);
    reduce_into(s, pcs, S, 2ll * C, 2ll * C, g_bias);
    reduce_into(s, pln, nbl, 2ll * C, C, g_ln_w);
    reduce_into(s, pln + C, nbl, 2ll * C, C, g_ln_b);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_stem_bwd(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int n, int h, int w, const float* wt,
                     const float* bias, const float* ln_w, float eps, const float* gout, float* g_w, float* g_bias, float* g_ln_w,
                     float* g_ln_b, void* bwd_workspace, int64_t bwd_workspace_bytes, void* stream) {
    if (!x || !wt || !bias || !ln_w || !gout || !g_w || !g_bias || !g_ln_w || !g_ln_b || !bwd_workspace || n <= 0 || h < 4 || w < 4)
        return AGP_E_BADARG;
    const int ho = (h - 4) / 4 + 1, wo = (w - 4) / 4 + 1;
    if (!cnx_map_ok(n, ho, wo)) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo, nb = ceil_div(ceil_div(P, 32), CNX_STEM_TILES);
    if (bwd_workspace_bytes < stem_bwd_floats(P) * 4) return AGP_E_BADARG;
    float* const part = (float*)bwd_workspace;
    hipStream_t s = (hipStream_t)stream;
    const CnxLoadF32 ld = {x, (long long)sn, (long long)sc, (long long)sh, (long long)sw};
    AGP_LAUNCH(cnx_stem_bwd_kernel<CnxLoadF32>, dim3((unsigned)nb), dim3(256), 0, s, ld, ho, wo, P, wt, bias, ln_w, eps, gout, part);
    reduce_into(s, part, nb, CNX_STEM_PART, 96 * 48, g_w);
    reduce_into(s, part + 96 * 48, nb, CNX_STEM_PART, 96, g_bias);
    reduce_into(s, part + 96 * 48 + 96, nb, CNX_STEM_PART, 96, g_ln_w);
    reduce_into(s, part + 96 * 48 + 192, nb, CNX_STEM_PART, 96, g_ln_b);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_stem_u8_bwd(const uint8_t* tiles, int n, int ncam, int h, int w, const float* mean3, const float* std3, const float* wt,
                        const float* bias, const float* ln_w, float eps, const float* gout, float* g_w, float* g_bias, float* g_ln_w,
                        float* g_ln_b, void* bwd_workspace, int64_t bwd_workspace_bytes, void* stream) {
    if (!tiles || !mean3 || !std3 || !wt || !bias || !ln_w || !gout || !g_w || !g_bias || !g_ln_w || !g_ln_b || !bwd_workspace || n <= 0 ||
        ncam <= 0 || h < 4 || w <= 0)
        return AGP_E_BADARG;
    const long long W = (long long)ncam * w;
    if (W < 4 || W >= (1ll << 31)) return AGP_E_BADARG;
    const int ho = (h - 4) / 4 + 1, wo = (int)((W - 4) / 4 + 1);
    if (!cnx_map_ok(n, ho, wo)) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo, nb = ceil_div(ceil_div(P, 32), CNX_STEM_TILES);
    if (bwd_workspace_bytes < stem_bwd_floats(P) * 4) return AGP_E_BADARG;
    float* const part = (float*)bwd_workspace;
    hipStream_t s = (hipStream_t)stream;
    const CnxLoadU8 ld = {tiles, ncam, h, w, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
    AGP_LAUNCH(cnx_stem_bwd_kernel<CnxLoadU8>, dim3((unsigned)nb), dim3(256), 0, s, ld, ho, wo, P, wt, bias, ln_w, eps, gout, part);
    reduce_into(s, part, nb, CNX_STEM_PART, 96 * 48, g_w);
    reduce_into(s, part + 96 * 48, nb, CNX_STEM_PART, 96, g_bias);
    reduce_into(s, part + 96 * 48 + 96, nb, CNX_STEM_PART, 96, g_ln_w);
    reduce_into(s, part + 96 * 48 + 192, nb, CNX_STEM_PART, 96, g_ln_b);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

}  // extern "C"
