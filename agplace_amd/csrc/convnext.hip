// ConvNeXt-tiny forward kernels (agplace_amd/convnext.py): stem, depthwise 7x7 + LayerNorm, the fused
// Linear -> GELU -> Linear block (with an optional per-image factor for the training forward), and the LayerNorm + 2x2/s2
// downsample.  The backward kernels are in convnext_bwd.hip.
//
// The residual stream is a plain fp32 [n][h][w][C] tensor (C = 96, 192 or 384).  Arithmetic follows the project's mode 3
// (AGP_PREC_BF16X3): every MFMA operand is a bf16 (hi, lo) pair and a product is hi*hi + hi*lo + lo*hi accumulated in fp32;
// LayerNorm statistics, GELU and the residual add are fp32; nothing is stored in fp16.
// The opt-in precision 4 of the inference path (template parameter PREC = 4 of the three matrix kernels, agp_cnx_*_f16_fwd) rounds
// the MFMA operands -- normalised operand, W1, GELU output, W2, downsample operand and weight -- to fp16 (cnx_h2: nearest even,
// saturating, NaN kept) and spends ONE mfma_f32_32x32x16_f16 per product; everything else, the fp32 stream included, is shared, and
// every difference sits behind `if constexpr`, so the PREC = 3 instantiations are the code they were.
//
// The matrix kernels compute TRANSPOSED products with mfma_f32_32x32x16_bf16: the weights are the A operand (output feature on
// the row), 32 pixels are the B operand (pixel on the column = on the lane).  A 32x32 result then has its pixel on the lane and
// its 32 features in the lane's 16 registers -- which is already the B-operand layout of a following MFMA that sums over those
// features.  agp_cnx_mlp_fwd uses this: a 32-wide slice of the hidden map leaves the first GEMM in registers, goes through
// bias + GELU + the bf16 split there and is consumed at once by the second GEMM.  The hidden map [P][4C] never exists in memory,
// LDS included.  The register r of lane (col, h = lane >> 5) holds feature row (r & 3) + 8 (r >> 2) + 4 h; the MFMA that takes
// registers 8t .. 8t+7 as its K slots 8h .. 8h+7 needs W2's columns in that order, which is how convnext.py lays them out.
#include "convnext_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------- grouped launches
// Up to CNX_MAXG independent problems (the trunks of a query / database pair advancing in lock-step, agplace_amd/pair.py) as ONE
// launch of the SAME kernel template: the trailing argument pack of the four forward kernels is empty (one problem, the arguments),
// the range guard's word (the guarded twin), or a CnxTable by value.  With a table the grid is the problems' own grids one behind
// the other, start[i] the first block of problem i (0xffffffff for an unused slot): a workgroup finds its problem from those prefix
// sums (wave-uniform: scalar compares), takes that problem's pointers and geometry in place of its arguments and runs the body at
// the block index it has INSIDE the problem -- so tiles, partial last tiles, arithmetic and summation order are the plain launch's,
// problem by problem, and nothing is shared across a problem boundary.  The problems share C, the precision and eps.  Every
// difference sits behind `if constexpr`: the instantiations without a table are the code they were.  Unguarded only (the pair falls
// back to the separate, guarded forwards while a ConvNeXt range guard would bind).
constexpr int CNX_MAXG = AGP_CNX_MAX_GROUPS;
template <class LOAD> struct CnxStemGroup {
    LOAD ld;
    int ho, wo;
    long long P;
    const float *wt, *bias, *g, *b;
    float* out;
};
struct CnxDwGroup {
    const float* x;
    int h, w, ty, tx;
    const float *wt, *bias, *g, *b;
    bf16_t *o_hi, *o_lo;
};
struct CnxMlpGroup {
    const bf16_t *x_hi, *x_lo;
    long long P;
    const bf16x8 *w1_hi, *w1_lo, *w2_hi, *w2_lo;
    const float *b1, *b2, *ls, *resid;
    float* out;
};
struct CnxDownGroup {
    const float* x;
    int h, w, ho, wo;
    long long P;
    const float *g, *b, *bias;
    const bf16x8 *w_hi, *w_lo;
    float* out;
};
template <class G> struct CnxTable {
    unsigned start[CNX_MAXG];
    G g[CNX_MAXG];
};
// what a kernel's trailing pack says
template <class... EX> struct CnxPack {
    static constexpr bool grouped = false, guarded = sizeof...(EX) != 0;
};
template <class G> struct CnxPack<CnxTable<G>> {
    static constexpr bool grouped = true, guarded = false;
};
// the problem of block `bid`; bid becomes the block index inside it
template <class B, class G> __device__ __forceinline__ const G& cnx_group(B& bid, const CnxTable<G>& tab) {
    int gi = 0;
#pragma unroll
    for (int i = 1; i < CNX_MAXG; ++i)
        if ((unsigned)bid >= tab.start[i]) gi = i;
    bid -= (B)tab.start[gi];
    return tab.g[gi];
}
using ::rg_word;               // (common.hpp) the range guard's word of a trailing pack: none for a table
template <class G> __device__ __forceinline__ uint32_t* rg_word(const CnxTable<G>&) { return nullptr; }

// ------------------------------------------------------------------------------------------------------------------ stem
// Conv2d(3, 96, k=4, s=4, bias) + LayerNorm over the 96 channels.  32 output pixels per block; a thread owns 3 channels
// (cl, cl + 32, cl + 64) of 4 pixels, the 32 lanes of a half wave hold one pixel's 96 channels.  wt: [48][96], 48 = (ci, ky, kx).
// LOAD: the image source (convnext_common.hpp: CnxLoadF32 strided fp32, CnxLoadU8 uint8 camera tiles normalised on the fly).
// gr: empty, or the table of a grouped launch (CnxTable above; the leading arguments but eps are then unused).
template <class LOAD, class... GR>
__global__ __launch_bounds__(256) void cnx_stem_kernel(const LOAD ld0, int ho, int wo, long long P, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, const float* __restrict__ g,
                                                       const float* __restrict__ b, float eps, float* __restrict__ out, GR... gr) {
    __shared__ float xin[32][48];
    const int t = threadIdx.x, cl = t & 31, pg = t >> 5;
    unsigned bid = blockIdx.x;
    const LOAD* lp = &ld0;
    if constexpr (CnxPack<GR...>::grouped) {
        const CnxStemGroup<LOAD>& d = cnx_group(bid, gr...);
        lp = &d.ld, ho = d.ho, wo = d.wo, P = d.P, wt = d.wt, bias = d.bias, g = d.g, b = d.b, out = d.out;
    }
    const LOAD& ld = *lp;
    const long long p0 = (long long)bid * 32;
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
        float w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = wt[idx * 96 + cl + 32 * k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float xv = xin[pg * 4 + i][idx];
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[i][k] = fmaf(xv, w[k], acc[i][k]);
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
        if (p < P) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = cl + 32 * k;
                out[p * 96 + c] = fmaf(d[k] * rstd, g[c], b[c]);
            }
        }
    }
}

// uint8 camera tiles -> the fp32 panorama [n][3][h][W = ncam * w] they stand for (contiguous NCHW): the image the uint8 stems
// read, element for element the same expression (CnxLoadU8).  Streaming: one element per thread and step, coalesced stores.
__global__ void cnx_normalize_u8_kernel(const CnxLoadU8 ld, int W, long long total, float* __restrict__ out) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int X = (int)(r % W);
        r /= W;
        const int y = (int)(r % ld.h);
        r /= ld.h;
        const int ci = (int)(r % 3);
        out[e] = ld(r / 3, ci, y, X);
    }
}

// ------------------------------------------------------------------------------------------- depthwise 7x7 + LayerNorm
// One block per 4 x 8 tile of output pixels of one image, all C channels.  The channels are walked in chunks of 32: the chunk's
// 10 x 14 input window (3-pixel halo, zeros outside the image: the window is addressed by (image, y, x), never by the flattened
// pixel index, so it cannot reach into a neighbouring image) and its 49 x 32 weights go to LDS; thread (cl = t & 31,
// col = t >> 5) computes the 4 outputs of its column for channel cl of the chunk.  Its C / 32 x 4 conv results stay in
// registers; the 32 lanes of a half wave then hold one pixel's C channels for the LayerNorm.  wt: [49][C].
// PREC: 3 = the operand as bf16 (hi, lo) planes; 4 = as ONE fp16 plane in o_hi (cnx_h1: nearest even, saturating), o_lo unused.
// rf (here, in cnx_mlp_kernel and in cnx_downsample_kernel; PREC = 4 only): the fp16 range guard's word in the guarded instantiation
// (common.hpp rg_word), the table of a grouped launch (CnxTable above), absent otherwise.  Tracked: the fp32 values handed to cnx_h1 / cnx_h2, before the clamp, of REAL pixels only.
template <int C, int PREC = 3, class... RF>
__global__ __launch_bounds__(256) void cnx_dwconv_ln_kernel(const float* __restrict__ x, int h, int w, int tiles_y, int tiles_x,
                                                            const float* __restrict__ wt, const float* __restrict__ bias,
                                                            const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                            bf16_t* __restrict__ o_hi, bf16_t* __restrict__ o_lo, RF... rf) {
    static_assert(!CnxPack<RF...>::guarded || PREC == 4, "the range guard covers the fp16 instantiations only");
    constexpr int NK = C / 32;
    RangeTrack<CnxPack<RF...>::guarded> rg;
    __shared__ __attribute__((aligned(16))) float tile[10][14][32];
    __shared__ float wl[49][32];
    const int t = threadIdx.x, cl = t & 31, col = t >> 5;
    int bid = blockIdx.x;
    if constexpr (CnxPack<RF...>::grouped) {
        const CnxDwGroup& d = cnx_group(bid, rf...);
        x = d.x, h = d.h, w = d.w, tiles_y = d.ty, tiles_x = d.tx, wt = d.wt, bias = d.bias, g = d.g, b = d.b, o_hi = d.o_hi, o_lo = d.o_lo;
    }
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
            for (int r = 0; r < 10; ++r) v[r] = tile[r][col + kx][cl];
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
        const int gy = y0 + i, gx = x0 + col;
        if (gy < h && gx < w) {
            const size_t p = ((size_t)img * h + gy) * w + gx;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int c = k * 32 + cl;
                if constexpr (PREC == 4) {
                    const float xn = fmaf(conv[i][k] * rstd, g[c], b[c]);
                    rg.sym2(xn, 0.f);          // inside the image test: the out-of-image positions of a partial tile do not report
                    o_hi[p * C + c] = cnx_h1(xn);
                    // (the twin only: without it the scheduler hoists every channel's gamma / beta load above the running maximum
                    // and C = 384 needs 100 VGPRs instead of 86 -- 4 waves per SIMD instead of the unguarded form's 5)
                    if constexpr (CnxPack<RF...>::guarded) __builtin_amdgcn_sched_barrier(0);
                } else {
                    bf16_t hi, lo;
                    split_bf16(fmaf(conv[i][k] * rstd, g[c], b[c]), hi, lo);
                    o_hi[p * C + c] = hi;
                    o_lo[p * C + c] = lo;
                }
            }
        }
    }
    rg.flush(rg_word(rf...));
}

// --------------------------------------------------------------------------------------- Linear -> GELU -> Linear, fused
// out[p][c] = resid[p][c] + ls[c] * (sum_j GELU(sum_k xn[p][k] W1[j][k] + b1[j]) W2[c][j] + b2[c]) for 32 pixels per block.
// The tile's operand planes sit in LDS ([32][C + 8] bf16 each).  The four waves split the hidden dimension: wave v takes the
// 32-wide hidden blocks v, v + 4, ...; per block: C / 16 k-steps of the first GEMM into one 32x32 accumulator, bias + GELU +
// split in registers, then 2 k-steps into each of the C / 32 output accumulators.  The waves' partial [C][32] sums are added in
// wave order through LDS (the operand planes' space, free by then), 32 channels at a time, with the epilogue: every output
// element is read (resid) and written (out) by the same thread, so `out` may alias `resid`.
// ROWS (the training forward, agp_cnx_mlp_fwd_rows): layer_scale is multiplied by row_scale[p / ppi], the stochastic-depth
// factor of the pixel's image -- per pixel, since a tile may straddle two images.  ROWS = false is the inference kernel, whose
// arithmetic does not change.
//   w1 planes: [4C / 32][C / 16][64 lanes][8]     lane (r, h) of block jb, step kk: W1[jb * 32 + r][kk * 16 + 8 h + e]
//   w2 planes: [4C / 32][2][C / 32][64 lanes][8]  lane (r, h) of block jb, half t, tile ct: W2[ct * 32 + r][jb * 32 + acc_row(8 t + e, h)]
// PREC = 4 (agp_cnx_mlp_f16_fwd): the operand, W1, the GELU output and W2 are fp16 and a product is ONE MFMA (mfma1h); one operand
// plane in LDS, one plane per weight (the *_hi arguments; the *_lo ones are unused), the same layouts, loop order and epilogue.
// Guarded (rf): a lane's hidden values belong to pixel p0 + r; rows p0 + r >= P are tile padding (a zero operand, hidden = GELU(b1))
// and do not report.
template <int C, bool ROWS, int PREC = 3, class... RF>
__global__ __launch_bounds__(256) void cnx_mlp_kernel(const bf16_t* __restrict__ x_hi, const bf16_t* __restrict__ x_lo, long long P,
                                                      const bf16x8* __restrict__ w1_hi, const bf16x8* __restrict__ w1_lo,
                                                      const float* __restrict__ b1, const bf16x8* __restrict__ w2_hi,
                                                      const bf16x8* __restrict__ w2_lo, const float* __restrict__ b2,
                                                      const float* __restrict__ ls, const float* resid, float* out,
                                                      const float* __restrict__ row_scale, long long ppi, RF... rf) {
    static_assert(!CnxPack<RF...>::guarded || (PREC == 4 && !ROWS), "the range guard covers the fp16 instantiations only");
    static_assert(!CnxPack<RF...>::grouped || !ROWS, "grouped launches are the inference kernel's");
    constexpr int LD = C + CNX_KPAD, KK = C / 16, CT = C / 32, JB = C / 8, VR = C / 8;
    RangeTrack<CnxPack<RF...>::guarded> rg;
    constexpr int XBYTES = (PREC == 4 ? 1 : 2) * CNX_TP * LD * 2, RBYTES = 4 * 32 * 36 * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[XBYTES > RBYTES ? XBYTES : RBYTES];
    bf16_t* const sx_hi = (bf16_t*)smem;
    bf16_t* const sx_lo = sx_hi + CNX_TP * LD;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
    unsigned bid = blockIdx.x;
    if constexpr (CnxPack<RF...>::grouped) {
        const CnxMlpGroup& d = cnx_group(bid, rf...);
        x_hi = d.x_hi, x_lo = d.x_lo, P = d.P, w1_hi = d.w1_hi, w1_lo = d.w1_lo, b1 = d.b1, w2_hi = d.w2_hi, w2_lo = d.w2_lo, b2 = d.b2;
        ls = d.ls, resid = d.resid, out = d.out;
    }
    const long long p0 = (long long)bid * CNX_TP;
    for (int e = t; e < CNX_TP * VR; e += 256) {
        const int row = e / VR, v = e - row * VR;
        u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
        if (p0 + row < P) {
            vh = *(const u32x4*)(x_hi + (size_t)(p0 + row) * C + v * 8);
            if constexpr (PREC != 4) vl = *(const u32x4*)(x_lo + (size_t)(p0 + row) * C + v * 8);
        }
        *(u32x4*)(sx_hi + row * LD + v * 8) = vh;
        if constexpr (PREC != 4) *(u32x4*)(sx_lo + row * LD + v * 8) = vl;
    }
    __syncthreads();
    f32x16 y[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) y[ct][i] = 0.f;
    const bf16_t* const bx_hi = sx_hi + r * LD + 8 * h;
    const bf16_t* const bx_lo = sx_lo + r * LD + 8 * h;
#pragma unroll 1
    for (int jb = wave; jb < JB; jb += 4) {
        f32x16 hacc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bv = *(const f32x4*)(b1 + jb * 32 + 8 * q + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) hacc[4 * q + i] = bv[i];
        }
        const bf16x8* const a_hi = w1_hi + (size_t)jb * KK * 64 + lane;
        const bf16x8* const a_lo = w1_lo + (size_t)jb * KK * 64 + lane;
        if constexpr (PREC == 4) {
#pragma unroll 4
            for (int kk = 0; kk < KK; ++kk) mfma1h(hacc, a_hi[kk * 64], *(const bf16x8*)(bx_hi + kk * 16));
            u32x4 gp[2];
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const float ga = gelu_exact(hacc[i]), gb = gelu_exact(hacc[i + 1]);
                rg.sym2_if(p0 + r < P, ga, gb);
                gp[i >> 3][(i & 7) >> 1] = cnx_h2(ga, gb);
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const bf16x8* const c_hi = w2_hi + ((size_t)(jb * 2 + tt) * CT) * 64 + lane;
                const bf16x8 gv = __builtin_bit_cast(bf16x8, gp[tt]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) mfma1h(y[ct], c_hi[ct * 64], gv);
            }
        } else {
#pragma unroll 4
            for (int kk = 0; kk < KK; ++kk)
                mfma3(hacc, a_hi[kk * 64], a_lo[kk * 64], *(const bf16x8*)(bx_hi + kk * 16), *(const bf16x8*)(bx_lo + kk * 16));
            bf16x8 g_hi[2], g_lo[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                bf16_t hi, lo;
                split_bf16(gelu_exact(hacc[i]), hi, lo);
                g_hi[i >> 3][i & 7] = (short)hi;
                g_lo[i >> 3][i & 7] = (short)lo;
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const bf16x8* const c_hi = w2_hi + ((size_t)(jb * 2 + tt) * CT) * 64 + lane;
                const bf16x8* const c_lo = w2_lo + ((size_t)(jb * 2 + tt) * CT) * 64 + lane;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) mfma3(y[ct], c_hi[ct * 64], c_lo[ct * 64], g_hi[tt], g_lo[tt]);
            }
        }
    }
    rg.flush(rg_word(rf...));
    float* const red = (float*)smem;       // [4 waves][32 pixels][36]: 32 channels + 4 floats of padding
    const int epx = t >> 3, ec = (t & 7) * 4;
    const long long ep = p0 + epx;
    float rs = 1.f;
    if (ROWS && ep < P) rs = row_scale[ep / ppi];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        __syncthreads();                   // the operand planes (first round) / the previous round's sums have been read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = {y[ct][4 * q], y[ct][4 * q + 1], y[ct][4 * q + 2], y[ct][4 * q + 3]};
            *(f32x4*)(red + (wave * 32 + r) * 36 + 8 * q + 4 * h) = v;
        }
        __syncthreads();
        if (ep < P) {
            const f32x4 s0 = *(const f32x4*)(red + (0 * 32 + epx) * 36 + ec), s1 = *(const f32x4*)(red + (1 * 32 + epx) * 36 + ec);
            const f32x4 s2 = *(const f32x4*)(red + (2 * 32 + epx) * 36 + ec), s3 = *(const f32x4*)(red + (3 * 32 + epx) * 36 + ec);
            const int c = ct * 32 + ec;
            const f32x4 rv = *(const f32x4*)(resid + (size_t)ep * C + c);
            const f32x4 bv = *(const f32x4*)(b2 + c);
            f32x4 lv = *(const f32x4*)(ls + c);
            if (ROWS) lv *= rs;
            f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = fmaf(lv[i], (((s0[i] + s1[i]) + s2[i]) + s3[i]) + bv[i], rv[i]);
            *(f32x4*)(out + (size_t)ep * C + c) = o;
        }
    }
}

// -------------------------------------------------------------------------------- LayerNorm + Conv2d(C, 2C, k=2, s=2)
// A GEMM with K = 4C (k = (ky * 2 + kx) * C + c) and N = 2C over the floor(h/2) x floor(w/2) output pixels, 32 per block, on
// the MLP kernel's MFMA core.  K is walked in chunks of 384 = 384 / C whole input pixels: eight lanes normalise one input
// pixel (fp32 statistics, two passes in registers) and write its operand planes to LDS, then wave v accumulates the output
// feature blocks v, v + 4, ... over the chunk.  w planes: [2C / 32][4C / 16][64 lanes][8] as w1 above.
// PREC = 4 (agp_cnx_downsample_f16_fwd): the normalised operand and the weight are fp16, one plane each (w_hi; w_lo unused), ONE MFMA.
template <int C, int PREC = 3, class... RF>
__global__ __launch_bounds__(256) void cnx_downsample_kernel(const float* __restrict__ x, int h, int w, int ho, int wo, long long P,
                                                             const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                             const bf16x8* __restrict__ w_hi, const bf16x8* __restrict__ w_lo,
                                                             const float* __restrict__ bias, float* __restrict__ out, RF... rf) {
    static_assert(!CnxPack<RF...>::guarded || PREC == 4, "the range guard covers the fp16 instantiations only");
    RangeTrack<CnxPack<RF...>::guarded> rg;
    constexpr int KC = 384, LD = KC + CNX_KPAD, IPP = KC / C, NCH = 4 * C / KC, NT = 2 * C / 32, NTW = (NT + 3) / 4, KKT = 4 * C / 16;
    constexpr int NV = C / 32;             // float4 per lane of a pixel's eight
    __shared__ __attribute__((aligned(16))) bf16_t sx_hi[CNX_TP * LD];
    __shared__ __attribute__((aligned(16))) bf16_t sx_lo[PREC == 4 ? 8 : CNX_TP * LD];     // (precision 4: one plane, unused)
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, hh = lane >> 5;
    unsigned bid = blockIdx.x;
    if constexpr (CnxPack<RF...>::grouped) {
        const CnxDownGroup& d = cnx_group(bid, rf...);
        x = d.x, h = d.h, w = d.w, ho = d.ho, wo = d.wo, P = d.P, g = d.g, b = d.b, w_hi = d.w_hi, w_lo = d.w_lo, bias = d.bias, out = d.out;
    }
    const long long p0 = (long long)bid * CNX_TP;
    const int lpx = t >> 3, sl = t & 7;
    const long long lp = p0 + lpx;
    long long img = 0;
    int oy = 0, ox = 0;
    if (lp < P) {
        img = lp / ((long long)ho * wo);
        const int rem = (int)(lp - img * ho * wo);
        oy = rem / wo;
        ox = rem - oy * wo;
    }
    f32x16 y[NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) y[n][i] = 0.f;
    const bf16_t* const bx_hi = sx_hi + r * LD + 8 * hh;
    const bf16_t* const bx_lo = sx_lo + r * LD + 8 * hh;
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
        __syncthreads();
#pragma unroll 1
        for (int sub = 0; sub < IPP; ++sub) {
            const int kp = ch * IPP + sub, ky = kp >> 1, kx = kp & 1;
            f32x4 v[NV];
            float s = 0.f;
            if (lp < P) {
                const float* src = x + (((size_t)img * h + (2 * oy + ky)) * w + (2 * ox + kx)) * C;
#pragma unroll
                for (int m = 0; m < NV; ++m) {
                    v[m] = *(const f32x4*)(src + (sl + 8 * m) * 4);
                    s += (v[m][0] + v[m][1]) + (v[m][2] + v[m][3]);
                }
            } else {
#pragma unroll
                for (int m = 0; m < NV; ++m) v[m] = f32x4{0.f, 0.f, 0.f, 0.f};
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
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const int c = (sl + 8 * m) * 4;
                const f32x4 gv = *(const f32x4*)(g + c), bv = *(const f32x4*)(b + c);
                if constexpr (PREC == 4) {
                    float xn[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) xn[i] = lp < P ? fmaf(v[m][i] * rstd, gv[i], bv[i]) : 0.f;
                    rg.sym2(xn[0], xn[1]);     // (a padding row lp >= P holds zeros)
                    rg.sym2(xn[2], xn[3]);
                    *(u32x2*)(sx_hi + lpx * LD + sub * C + c) = u32x2{cnx_h2(xn[0], xn[1]), cnx_h2(xn[2], xn[3])};
                } else {
                    bf16_t hi[4], lo[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) split_bf16(lp < P ? fmaf(v[m][i] * rstd, gv[i], bv[i]) : 0.f, hi[i], lo[i]);
                    *(u32x2*)(sx_hi + lpx * LD + sub * C + c) = u32x2{pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
                    *(u32x2*)(sx_lo + lpx * LD + sub * C + c) = u32x2{pack2(lo[0], lo[1]), pack2(lo[2], lo[3])};
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
            const int nt = wave + 4 * n;
            if (nt < NT) {
                const bf16x8* const a_hi = w_hi + ((size_t)nt * KKT + ch * (KC / 16)) * 64 + lane;
                const bf16x8* const a_lo = w_lo + ((size_t)nt * KKT + ch * (KC / 16)) * 64 + lane;
#pragma unroll 4
                for (int kk = 0; kk < KC / 16; ++kk) {
                    if constexpr (PREC == 4) mfma1h(y[n], a_hi[kk * 64], *(const bf16x8*)(bx_hi + kk * 16));
                    else mfma3(y[n], a_hi[kk * 64], a_lo[kk * 64], *(const bf16x8*)(bx_hi + kk * 16), *(const bf16x8*)(bx_lo + kk * 16));
                }
            }
        }
    }
    rg.flush(rg_word(rf...));
    const long long op = p0 + r;
    if (op < P) {
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
            const int nt = wave + 4 * n;
            if (nt < NT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = nt * 32 + 8 * q + 4 * hh;
                    const f32x4 bv = *(const f32x4*)(bias + c);
                    const f32x4 o = {y[n][4 * q] + bv[0], y[n][4 * q + 1] + bv[1], y[n][4 * q + 2] + bv[2], y[n][4 * q + 3] + bv[3]};
                    *(f32x4*)(out + (size_t)op * (2 * C) + c) = o;
                }
            }
        }
    }
}

// Host side of a grouped launch: an empty table; append a problem of `blocks` workgroups (false when the launch would leave the
// 2^31 - 1 blocks of a grid).
template <class G> inline void cnx_table_init(CnxTable<G>& tab) {
    for (int i = 0; i < CNX_MAXG; ++i) {
        tab.start[i] = 0xffffffffu;
        tab.g[i] = G{};
    }
}
template <class G> inline bool cnx_table_add(CnxTable<G>& tab, int i, long long& total, long long blocks, const G& g) {
    if (blocks <= 0 || total + blocks >= (1ll << 31)) return false;
    tab.start[i] = (unsigned)total;
    tab.g[i] = g;
    total += blocks;
    return true;
}
inline bool cnx_groups_ok(const agp_cnx_group* groups, int ngroups) { return groups && ngroups >= 1 && ngroups <= CNX_MAXG; }

}  // namespace

extern "C" {

int64_t agp_cnx_workspace_bytes(int n, int h, int w, int C) {
    if (!cnx_map_ok(n, h, w) || !cnx_c_host_ok(C)) return -1;
    return 2 * cnx_pad((long long)n * h * w) * C * 2;      // the normalised operand: two bf16 planes [P_pad][C]
}

int agp_cnx_stem_fwd(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int n, int h, int w, const float* wt,
                     const float* bias, const float* ln_w, const float* ln_b, float eps, float* out, void* stream) {
    if (!x || !wt || !bias || !ln_w || !ln_b || !out || n <= 0 || h < 4 || w < 4) return AGP_E_BADARG;
    const int ho = (h - 4) / 4 + 1, wo = (w - 4) / 4 + 1;
    if (!cnx_map_ok(n, ho, wo)) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo;
    const CnxLoadF32 ld = {x, (long long)sn, (long long)sc, (long long)sh, (long long)sw};
    AGP_LAUNCH(cnx_stem_kernel<CnxLoadF32>, dim3((unsigned)((P + 31) / 32)), dim3(256), 0, (hipStream_t)stream, ld, ho, wo, P, wt, bias,
               ln_w, ln_b, eps, out);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_stem_u8_fwd(const uint8_t* tiles, int n, int ncam, int h, int w, const float* mean3, const float* std3, const float* wt,
                        const float* bias, const float* ln_w, const float* ln_b, float eps, float* out, void* stream) {
    if (!tiles || !mean3 || !std3 || !wt || !bias || !ln_w || !ln_b || !out || n <= 0 || ncam <= 0 || h < 4 || w <= 0) return AGP_E_BADARG;
    const long long W = (long long)ncam * w;
    if (W < 4 || W >= (1ll << 31)) return AGP_E_BADARG;
    const int ho = (h - 4) / 4 + 1, wo = (int)((W - 4) / 4 + 1);
    if (!cnx_map_ok(n, ho, wo)) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo;
    const CnxLoadU8 ld = {tiles, ncam, h, w, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
    AGP_LAUNCH(cnx_stem_kernel<CnxLoadU8>, dim3((unsigned)((P + 31) / 32)), dim3(256), 0, (hipStream_t)stream, ld, ho, wo, P, wt, bias,
               ln_w, ln_b, eps, out);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_normalize_u8_cams(const uint8_t* tiles, int n, int ncam, int h, int w, const float* mean3, const float* std3, float* out,
                          void* stream) {
    if (!tiles || !mean3 || !std3 || !out || n <= 0 || ncam <= 0 || h < 4 || w <= 0) return AGP_E_BADARG;
    const long long W = (long long)ncam * w;
    if (W < 4 || W >= (1ll << 31)) return AGP_E_BADARG;      // (an image the stem takes: at least one 4x4 patch)
    const CnxLoadU8 ld = {tiles, ncam, h, w, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
    const long long total = (long long)n * 3 * h * W;
    const long long blocks = (total + 255) / 256;
    AGP_LAUNCH(cnx_normalize_u8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, ld, (int)W,
               total, out);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_dwconv_ln_fwd(const float* x, int n, int h, int w, int C, const float* wt, const float* bias, const float* ln_w,
                          const float* ln_b, float eps, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !wt || !bias || !ln_w || !ln_b || !workspace || !cnx_map_ok(n, h, w) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    if (workspace_bytes < agp_cnx_workspace_bytes(n, h, w, C) || ((uintptr_t)workspace & 15)) return AGP_E_BADARG;
    bf16_t* const hi = (bf16_t*)workspace;
    bf16_t* const lo = hi + cnx_pad((long long)n * h * w) * C;
    const int ty = (h + 3) / 4, tx = (w + 7) / 8;
    const dim3 grid((unsigned)((long long)n * ty * tx));
    hipStream_t s = (hipStream_t)stream;
    if (C == 96) { AGP_LAUNCH(cnx_dwconv_ln_kernel<96>, grid, dim3(256), 0, s, x, h, w, ty, tx, wt, bias, ln_w, ln_b, eps, hi, lo); }
    else if (C == 192) { AGP_LAUNCH(cnx_dwconv_ln_kernel<192>, grid, dim3(256), 0, s, x, h, w, ty, tx, wt, bias, ln_w, ln_b, eps, hi, lo); }
    else { AGP_LAUNCH(cnx_dwconv_ln_kernel<384>, grid, dim3(256), 0, s, x, h, w, ty, tx, wt, bias, ln_w, ln_b, eps, hi, lo); }
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_mlp_fwd_rows(const void* workspace, int64_t workspace_bytes, int64_t P, int C, const void* w1_hi, const void* w1_lo,
                         const float* b1, const void* w2_hi, const void* w2_lo, const float* b2, const float* layer_scale,
                         const float* resid, float* out, const float* row_scale, int64_t pixels_per_image, void* stream) {
    if (!workspace || !w1_hi || !w1_lo || !b1 || !w2_hi || !w2_lo || !b2 || !layer_scale || !resid || !out) return AGP_E_BADARG;
    if (P <= 0 || P >= (1ll << 31) / 32 || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    if (row_scale && (pixels_per_image <= 0 || P % pixels_per_image)) return AGP_E_BADARG;
    if (workspace_bytes < 2 * cnx_pad(P) * C * 2 || ((uintptr_t)workspace & 15)) return AGP_E_BADARG;
    const bf16_t* const hi = (const bf16_t*)workspace;
    const bf16_t* const lo = hi + cnx_pad(P) * C;
    const dim3 grid((unsigned)((P + CNX_TP - 1) / CNX_TP));
    hipStream_t s = (hipStream_t)stream;
    const bf16x8 *a = (const bf16x8*)w1_hi, *b = (const bf16x8*)w1_lo, *c = (const bf16x8*)w2_hi, *d = (const bf16x8*)w2_lo;
    const long long ppi = pixels_per_image;
#define CNX_MLP(CC, RR) AGP_LAUNCH((cnx_mlp_kernel<CC, RR>), grid, dim3(256), 0, s, hi, lo, (long long)P, a, b, b1, c, d, b2, layer_scale, resid, out, row_scale, ppi)
    if (row_scale) {
        if (C == 96) { CNX_MLP(96, true); } else if (C == 192) { CNX_MLP(192, true); } else { CNX_MLP(384, true); }
    } else {
        if (C == 96) { CNX_MLP(96, false); } else if (C == 192) { CNX_MLP(192, false); } else { CNX_MLP(384, false); }
    }
#undef CNX_MLP
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_mlp_fwd(const void* workspace, int64_t workspace_bytes, int64_t P, int C, const void* w1_hi, const void* w1_lo,
                    const float* b1, const void* w2_hi, const void* w2_lo, const float* b2, const float* layer_scale,
                    const float* resid, float* out, void* stream) {
    return agp_cnx_mlp_fwd_rows(workspace, workspace_bytes, P, C, w1_hi, w1_lo, b1, w2_hi, w2_lo, b2, layer_scale, resid, out, nullptr,
                                0, stream);
}

int agp_cnx_downsample_fwd(const float* x, int n, int h, int w, int C, const float* ln_w, const float* ln_b, float eps,
                           const void* w_hi, const void* w_lo, const float* bias, float* out, void* stream) {
    if (!x || !ln_w || !ln_b || !w_hi || !w_lo || !bias || !out || !cnx_map_ok(n, h, w) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    const int ho = h / 2, wo = w / 2;
    if (ho < 1 || wo < 1) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo;
    const dim3 grid((unsigned)((P + CNX_TP - 1) / CNX_TP));
    hipStream_t s = (hipStream_t)stream;
    const bf16x8 *a = (const bf16x8*)w_hi, *b = (const bf16x8*)w_lo;
    if (C == 96) { AGP_LAUNCH(cnx_downsample_kernel<96>, grid, dim3(256), 0, s, x, h, w, ho, wo, P, ln_w, ln_b, eps, a, b, bias, out); }
    else if (C == 192) { AGP_LAUNCH(cnx_downsample_kernel<192>, grid, dim3(256), 0, s, x, h, w, ho, wo, P, ln_w, ln_b, eps, a, b, bias, out); }
    else { AGP_LAUNCH(cnx_downsample_kernel<384>, grid, dim3(256), 0, s, x, h, w, ho, wo, P, ln_w, ln_b, eps, a, b, bias, out); }
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

// ---- precision 4 (Options.convnext_precision = 4): the PREC = 4 instantiations.  One fp16 operand plane [P_pad][C] at the start of
// the workspace, one fp16 plane per weight; the kernels' unused second-plane arguments are null.
int agp_cnx_dwconv_ln_f16_fwd(const float* x, int n, int h, int w, int C, const float* wt, const float* bias, const float* ln_w,
                              const float* ln_b, float eps, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !wt || !bias || !ln_w || !ln_b || !workspace || !cnx_map_ok(n, h, w) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    if (workspace_bytes < cnx_pad((long long)n * h * w) * C * 2 || ((uintptr_t)workspace & 15)) return AGP_E_BADARG;
    bf16_t* const xp = (bf16_t*)workspace;
    bf16_t* const none = nullptr;
    const int ty = (h + 3) / 4, tx = (w + 7) / 8;
    const dim3 grid((unsigned)((long long)n * ty * tx));
    hipStream_t s = (hipStream_t)stream;
    // the guarded twin while a range-guard word is bound (common.hpp agp_launch_rg); here and in the two launchers below
    auto launch = [&](auto cc) {
        return agp_launch_rg<AGP_RG_TWINS(cnx_dwconv_ln_kernel, decltype(cc)::value, 4)>(
            agp_range_flag_get(), grid, dim3(256), 0, 0, s, x, h, w, ty, tx, wt, bias, ln_w, ln_b, eps, xp, none);
    };
    if (C == 96) return launch(std::integral_constant<int, 96>{});
    if (C == 192) return launch(std::integral_constant<int, 192>{});
    return launch(std::integral_constant<int, 384>{});
}

int agp_cnx_mlp_f16_fwd(const void* workspace, int64_t workspace_bytes, int64_t P, int C, const void* w1, const float* b1,
                        const void* w2, const float* b2, const float* layer_scale, const float* resid, float* out, void* stream) {
    if (!workspace || !w1 || !b1 || !w2 || !b2 || !layer_scale || !resid || !out) return AGP_E_BADARG;
    if (P <= 0 || P >= (1ll << 31) / 32 || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    if (workspace_bytes < cnx_pad(P) * C * 2 || ((uintptr_t)workspace & 15)) return AGP_E_BADARG;
    const bf16_t* const xp = (const bf16_t*)workspace;
    const bf16_t* const nox = nullptr;
    const bf16x8 *a = (const bf16x8*)w1, *c = (const bf16x8*)w2, *now = nullptr;
    const float* const norows = nullptr;
    const dim3 grid((unsigned)((P + CNX_TP - 1) / CNX_TP));
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto cc) {
        return agp_launch_rg<AGP_RG_TWINS(cnx_mlp_kernel, decltype(cc)::value, false, 4)>(
            agp_range_flag_get(), grid, dim3(256), 0, 0, s, xp, nox, (long long)P, a, now, b1, c, now, b2, layer_scale, resid, out, norows,
            0ll);
    };
    if (C == 96) return launch(std::integral_constant<int, 96>{});
    if (C == 192) return launch(std::integral_constant<int, 192>{});
    return launch(std::integral_constant<int, 384>{});
}

int agp_cnx_downsample_f16_fwd(const float* x, int n, int h, int w, int C, const float* ln_w, const float* ln_b, float eps,
                               const void* wt, const float* bias, float* out, void* stream) {
    if (!x || !ln_w || !ln_b || !wt || !bias || !out || !cnx_map_ok(n, h, w) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    const int ho = h / 2, wo = w / 2;
    if (ho < 1 || wo < 1) return AGP_E_BADARG;
    const long long P = (long long)n * ho * wo;
    const dim3 grid((unsigned)((P + CNX_TP - 1) / CNX_TP));
    hipStream_t s = (hipStream_t)stream;
    const bf16x8 *a = (const bf16x8*)wt, *none = nullptr;
    auto launch = [&](auto cc) {
        return agp_launch_rg<AGP_RG_TWINS(cnx_downsample_kernel, decltype(cc)::value, 4)>(
            agp_range_flag_get(), grid, dim3(256), 0, 0, s, x, h, w, ho, wo, P, ln_w, ln_b, eps, a, none, bias, out);
    };
    if (C == 96) return launch(std::integral_constant<int, 96>{});
    if (C == 192) return launch(std::integral_constant<int, 192>{});
    return launch(std::integral_constant<int, 384>{});
}

// ---- grouped launches (include/agplace_hip.h: agp_cnx_group): 1 .. AGP_CNX_MAX_GROUPS problems per launch, each validated as by its
// plain entry above; the kernels' leading arguments are unused (the table replaces them) except eps.
int agp_cnx_stem_fwd_grouped(const agp_cnx_group* groups, int ngroups, float eps, void* stream) {
    if (!cnx_groups_ok(groups, ngroups)) return AGP_E_BADARG;
    using T = CnxTable<CnxStemGroup<CnxLoadF32>>;
    T tab;
    cnx_table_init(tab);
    long long total = 0;
    for (int i = 0; i < ngroups; ++i) {
        const agp_cnx_group& q = groups[i];
        if (!q.x || !q.wt || !q.bias || !q.ln_w || !q.ln_b || !q.out || q.n <= 0 || q.h < 4 || q.w < 4) return AGP_E_BADARG;
        const int ho = (q.h - 4) / 4 + 1, wo = (q.w - 4) / 4 + 1;
        if (!cnx_map_ok(q.n, ho, wo)) return AGP_E_BADARG;
        const long long P = (long long)q.n * ho * wo;
        const CnxLoadF32 ld = {(const float*)q.x, (long long)q.sn, (long long)q.sc, (long long)q.sh, (long long)q.sw};
        if (!cnx_table_add(tab, i, total, (P + 31) / 32, {ld, ho, wo, P, q.wt, q.bias, q.ln_w, q.ln_b, (float*)q.out})) return AGP_E_BADARG;
    }
    const float* const nof = nullptr;
    float* const noo = nullptr;
    AGP_LAUNCH((cnx_stem_kernel<CnxLoadF32, T>), dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, CnxLoadF32{}, 0, 0, 0ll, nof,
               nof, nof, nof, eps, noo, tab);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_stem_u8_fwd_grouped(const agp_cnx_group* groups, int ngroups, float eps, void* stream) {
    if (!cnx_groups_ok(groups, ngroups)) return AGP_E_BADARG;
    using T = CnxTable<CnxStemGroup<CnxLoadU8>>;
    T tab;
    cnx_table_init(tab);
    long long total = 0;
    for (int i = 0; i < ngroups; ++i) {
        const agp_cnx_group& q = groups[i];
        if (!q.x || !q.wt || !q.bias || !q.ln_w || !q.ln_b || !q.out || q.n <= 0 || q.ncam <= 0 || q.h < 4 || q.w <= 0) return AGP_E_BADARG;
        const long long W = (long long)q.ncam * q.w;
        if (W < 4 || W >= (1ll << 31)) return AGP_E_BADARG;
        const int ho = (q.h - 4) / 4 + 1, wo = (int)((W - 4) / 4 + 1);
        if (!cnx_map_ok(q.n, ho, wo)) return AGP_E_BADARG;
        const long long P = (long long)q.n * ho * wo;
        const CnxLoadU8 ld = {(const uint8_t*)q.x, q.ncam, q.h, q.w, q.mean3[0], q.mean3[1], q.mean3[2], q.std3[0], q.std3[1], q.std3[2]};
        if (!cnx_table_add(tab, i, total, (P + 31) / 32, {ld, ho, wo, P, q.wt, q.bias, q.ln_w, q.ln_b, (float*)q.out})) return AGP_E_BADARG;
    }
    const float* const nof = nullptr;
    float* const noo = nullptr;
    AGP_LAUNCH((cnx_stem_kernel<CnxLoadU8, T>), dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, CnxLoadU8{}, 0, 0, 0ll, nof, nof,
               nof, nof, eps, noo, tab);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

// planes: operand / weight planes per tensor, 2 = bf16 (hi, lo), 1 = fp16 (the PREC = 4 instantiations)
static int cnx_dwconv_ln_grouped(const agp_cnx_group* groups, int ngroups, int C, float eps, int planes, void* stream) {
    if (!cnx_groups_ok(groups, ngroups) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    using T = CnxTable<CnxDwGroup>;
    T tab;
    cnx_table_init(tab);
    long long total = 0;
    for (int i = 0; i < ngroups; ++i) {
        const agp_cnx_group& q = groups[i];
        if (!q.x || !q.wt || !q.bias || !q.ln_w || !q.ln_b || !q.workspace || !cnx_map_ok(q.n, q.h, q.w)) return AGP_E_BADARG;
        const long long plane = cnx_pad((long long)q.n * q.h * q.w) * C;
        if (q.workspace_bytes < planes * plane * 2 || ((uintptr_t)q.workspace & 15)) return AGP_E_BADARG;
        bf16_t* const hi = (bf16_t*)q.workspace;
        bf16_t* const lo = planes == 2 ? hi + plane : nullptr;
        const int ty = (q.h + 3) / 4, tx = (q.w + 7) / 8;
        if (!cnx_table_add(tab, i, total, (long long)q.n * ty * tx, {(const float*)q.x, q.h, q.w, ty, tx, q.wt, q.bias, q.ln_w, q.ln_b, hi, lo}))
            return AGP_E_BADARG;
    }
    const dim3 grid((unsigned)total);
    hipStream_t s = (hipStream_t)stream;
    const float* const nof = nullptr;
    bf16_t* const nob = nullptr;
#define CNX_DWG(CC, PP) AGP_LAUNCH((cnx_dwconv_ln_kernel<CC, PP, T>), grid, dim3(256), 0, s, nof, 0, 0, 0, 0, nof, nof, nof, nof, eps, nob, nob, tab)
    if (planes == 2) {
        if (C == 96) { CNX_DWG(96, 3); } else if (C == 192) { CNX_DWG(192, 3); } else { CNX_DWG(384, 3); }
    } else {
        if (C == 96) { CNX_DWG(96, 4); } else if (C == 192) { CNX_DWG(192, 4); } else { CNX_DWG(384, 4); }
    }
#undef CNX_DWG
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

static int cnx_mlp_grouped(const agp_cnx_group* groups, int ngroups, int C, int planes, void* stream) {
    if (!cnx_groups_ok(groups, ngroups) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    using T = CnxTable<CnxMlpGroup>;
    T tab;
    cnx_table_init(tab);
    long long total = 0;
    const bool two = planes == 2;
    for (int i = 0; i < ngroups; ++i) {
        const agp_cnx_group& q = groups[i];
        if (!q.workspace || !q.w1_hi || !q.b1 || !q.w2_hi || !q.b2 || !q.layer_scale || !q.x || !q.out) return AGP_E_BADARG;
        if (two && (!q.w1_lo || !q.w2_lo)) return AGP_E_BADARG;
        if (!cnx_map_ok(q.n, q.h, q.w)) return AGP_E_BADARG;
        const long long P = (long long)q.n * q.h * q.w, plane = cnx_pad(P) * C;
        if (q.workspace_bytes < planes * plane * 2 || ((uintptr_t)q.workspace & 15)) return AGP_E_BADARG;
        const bf16_t* const hi = (const bf16_t*)q.workspace;
        const bf16_t* const lo = two ? hi + plane : nullptr;
        if (!cnx_table_add(tab, i, total, (P + CNX_TP - 1) / CNX_TP,
                           {hi, lo, P, (const bf16x8*)q.w1_hi, two ? (const bf16x8*)q.w1_lo : nullptr, (const bf16x8*)q.w2_hi,
                            two ? (const bf16x8*)q.w2_lo : nullptr, q.b1, q.b2, q.layer_scale, (const float*)q.x, (float*)q.out}))
            return AGP_E_BADARG;
    }
    const dim3 grid((unsigned)total);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* const nox = nullptr;
    const bf16x8* const now = nullptr;
    const float* const nof = nullptr;
    float* const noo = nullptr;
#define CNX_MLPG(CC, PP) \
    AGP_LAUNCH((cnx_mlp_kernel<CC, false, PP, T>), grid, dim3(256), 0, s, nox, nox, 0ll, now, now, nof, now, now, nof, nof, nof, noo, nof, 0ll, tab)
    if (two) {
        if (C == 96) { CNX_MLPG(96, 3); } else if (C == 192) { CNX_MLPG(192, 3); } else { CNX_MLPG(384, 3); }
    } else {
        if (C == 96) { CNX_MLPG(96, 4); } else if (C == 192) { CNX_MLPG(192, 4); } else { CNX_MLPG(384, 4); }
    }
#undef CNX_MLPG
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

static int cnx_downsample_grouped(const agp_cnx_group* groups, int ngroups, int C, float eps, int planes, void* stream) {
    if (!cnx_groups_ok(groups, ngroups) || !cnx_c_host_ok(C)) return AGP_E_BADARG;
    using T = CnxTable<CnxDownGroup>;
    T tab;
    cnx_table_init(tab);
    long long total = 0;
    for (int i = 0; i < ngroups; ++i) {
        const agp_cnx_group& q = groups[i];
        if (!q.x || !q.ln_w || !q.ln_b || !q.w1_hi || !q.bias || !q.out || !cnx_map_ok(q.n, q.h, q.w)) return AGP_E_BADARG;
        if (planes == 2 && !q.w1_lo) return AGP_E_BADARG;
        const int ho = q.h / 2, wo = q.w / 2;
        if (ho < 1 || wo < 1) return AGP_E_BADARG;
        const long long P = (long long)q.n * ho * wo;
        if (!cnx_table_add(tab, i, total, (P + CNX_TP - 1) / CNX_TP,
                           {(const float*)q.x, q.h, q.w, ho, wo, P, q.ln_w, q.ln_b, q.bias, (const bf16x8*)q.w1_hi,
                            planes == 2 ? (const bf16x8*)q.w1_lo : nullptr, (float*)q.out}))
            return AGP_E_BADARG;
    }
    const dim3 grid((unsigned)total);
    hipStream_t s = (hipStream_t)stream;
    const float* const nof = nullptr;
    const bf16x8* const now = nullptr;
    float* const noo = nullptr;
#define CNX_DOWNG(CC, PP) \
    AGP_LAUNCH((cnx_downsample_kernel<CC, PP, T>), grid, dim3(256), 0, s, nof, 0, 0, 0, 0, 0ll, nof, nof, eps, now, now, nof, noo, tab)
    if (planes == 2) {
        if (C == 96) { CNX_DOWNG(96, 3); } else if (C == 192) { CNX_DOWNG(192, 3); } else { CNX_DOWNG(384, 3); }
    } else {
        if (C == 96) { CNX_DOWNG(96, 4); } else if (C == 192) { CNX_DOWNG(192, 4); } else { CNX_DOWNG(384, 4); }
    }
#undef CNX_DOWNG
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

int agp_cnx_dwconv_ln_fwd_grouped(const agp_cnx_group* groups, int ngroups, int C, float eps, void* stream) {
    return cnx_dwconv_ln_grouped(groups, ngroups, C, eps, 2, stream);
}
int agp_cnx_dwconv_ln_f16_fwd_grouped(const agp_cnx_group* groups, int ngroups, int C, float eps, void* stream) {
    return cnx_dwconv_ln_grouped(groups, ngroups, C, eps, 1, stream);
}
int agp_cnx_mlp_fwd_grouped(const agp_cnx_group* groups, int ngroups, int C, void* stream) {
    return cnx_mlp_grouped(groups, ngroups, C, 2, stream);
}
int agp_cnx_mlp_f16_fwd_grouped(const agp_cnx_group* groups, int ngroups, int C, void* stream) {
    return cnx_mlp_grouped(groups, ngroups, C, 1, stream);
}
int agp_cnx_downsample_fwd_grouped(const agp_cnx_group* groups, int ngroups, int C, float eps, void* stream) {
    return cnx_downsample_grouped(groups, ngroups, C, eps, 2, stream);
}
int agp_cnx_downsample_f16_fwd_grouped(const agp_cnx_group* groups, int ngroups, int C, float eps, void* stream) {
    return cnx_downsample_grouped(groups, ngroups, C, eps, 1, stream);
}

}  // extern "C"
