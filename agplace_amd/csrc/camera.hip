// Camera front end: decoded uint8 frames -> Pillow's bilinear resize (ImagingResample, 8 bits per channel) -> either the resized
// uint8 tiles or the stem's normalised NHWC4 input map, in one launch.
//
// The arithmetic is Pillow's, integer for integer: per axis a table of 22-bit fixed-point coefficients and of (first tap, tap
// count) bounds, made on the host in double (agp_resize_coeffs); out = min(255, (2^21 + sum_t k[t] * in[first + t]) >> 22).
// The horizontal pass runs first and its result is ROUNDED TO uint8 before the vertical pass reads it -- Pillow stores the
// intermediate image as 8-bit pixels, so a wider intermediate would be a different (if "better") function.
//
// One workgroup owns a TH x TW output tile of one frame.  The bounds tables give the input patch the tile needs; its rows are
// staged into LDS in chunks (16-byte loads from aligned-down addresses: a row is 3 * W0 bytes and starts anywhere), each chunk's
// horizontal pass lands in a uint8 LDS buffer of patch rows x TW pixels, and the vertical pass reads that buffer.  Memory-bound,
// integer-only, no MFMA.
#include <math.h>
#include "common.hpp"

namespace agp_camera {

constexpr int TH = 16, TW = 64;                 // output tile (rows x columns) of a workgroup of 256 threads
constexpr int KS_MAX = 17;                      // taps per output pixel at the largest supported reduction (in / out = 8)
constexpr int MAX_RATIO = 8;
constexpr int MAX_DIM = 16384;
// input patch of a tile at in / out <= 8: (T + 1) * 8 + 1 pixels, + 1 for the rounding of the bounds
constexpr int ROWS_MAX = (TH + 1) * MAX_RATIO + 4;      // 140 patch rows
constexpr int COLS_MAX = (TW + 1) * MAX_RATIO + 4;      // 524 patch columns
constexpr int HP = TW * 3;                              // bytes of a row of the horizontal pass's result
constexpr int STAGE_BYTES = 16384;                      // >= 10 rows of the widest patch (pitch <= 1600)
static_assert((COLS_MAX * 3 + 15 + 15) / 16 * 16 <= 1600 && STAGE_BYTES / 1600 >= 1, "stage buffer too small");

__device__ __forceinline__ int wave_min_i(int v) {
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// PACK == false: out8 = uint8 [n * ncam][h][w][3].  PACK == true: hi / lo = the stem's map [n][h + 2 pad][ncam * w + 2 pad][4]
// (lo == nullptr: one fp16 plane), v = (u8 / 255 - mean) / std exactly as pack_u8_cams_kernel (pack.hip) writes it.
// kx / ky: int32 [out][ksx / ksy], bx / by: int32 [out][2] = (first tap, tap count).  Bounds are clamped to the frame when they
// are loaded, and a tile whose patch would not fit the LDS buffers writes nothing: tables that do not belong to the geometry
// (the host cannot see device memory) can give wrong pixels, never an access outside the frame or the buffers.
// The kernel resizes a WINDOW of H0 x W0 pixels of every frame (torchvision's CenterCrop in front of the Resize; the whole frame
// is the window at origin 0): frame f's window starts at frames + f * fstride + origin and its rows are gpitch bytes apart.  The
// tables are those of the window's size, so the bounds, clamped to H0 x W0, never leave the window.
template <bool PACK>
__global__ __launch_bounds__(256) void resize_cams_kernel(const uint8_t* __restrict__ frames, size_t fstride, size_t origin,
                                                          int gpitch, int ncam, int H0, int W0, int h, int w,
                                                          const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, int ksx,
                                                          const int32_t* __restrict__ ky, const int32_t* __restrict__ by, int ksy,
                                                          int tiles_x, int tiles_y, uint8_t* __restrict__ out8, float m0, float m1,
                                                          float m2, float s0, float s1, float s2, int pad, bf16_t* __restrict__ hi,
                                                          bf16_t* __restrict__ lo) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
    __shared__ uint8_t hbuf[ROWS_MAX * HP];
    __shared__ int32_t kxs[TW * KS_MAX], kys[TH * KS_MAX];
    __shared__ int32_t bxs[TW * 2], bys[TH * 2];
    __shared__ int32_t span[4];                 // patch: first column, end column, first row, end row

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t b = blockIdx.x;
    const int tx = (int)(b % (uint32_t)tiles_x); b /= (uint32_t)tiles_x;
    const int ty = (int)(b % (uint32_t)tiles_y);
    const uint32_t frame = b / (uint32_t)tiles_y;                      // n * ncam frames
    const int ox0 = tx * TW, oy0 = ty * TH;
    const int ow_t = min(TW, w - ox0), oh_t = min(TH, h - oy0);

    // ---- the tile's coefficient rows and bounds -> LDS
    for (int i = tid; i < ow_t * ksx; i += 256) {
        const int x = i / ksx, t = i - x * ksx;
        kxs[x * KS_MAX + t] = kx[(size_t)(ox0 + x) * ksx + t];
    }
    for (int i = tid; i < oh_t * ksy; i += 256) {
        const int y = i / ksy, t = i - y * ksy;
        kys[y * KS_MAX + t] = ky[(size_t)(oy0 + y) * ksy + t];
    }
    if (wv == 0) {
        int mn = W0, en = 0;
        if (lane < ow_t) {
            mn = min(max(bx[2 * (ox0 + lane)], 0), W0 - 1);
            const int cnt = min(max(bx[2 * (ox0 + lane) + 1], 0), min(ksx, W0 - mn));
            bxs[2 * lane] = mn; bxs[2 * lane + 1] = cnt;
            en = mn + cnt;
        }
        mn = wave_min_i(mn); en = wave_max_i(en);
        if (lane == 0) { span[0] = mn; span[1] = en; }
    } else if (wv == 1) {
        int mn = H0, en = 0;
        if (lane < oh_t) {
            mn = min(max(by[2 * (oy0 + lane)], 0), H0 - 1);
            const int cnt = min(max(by[2 * (oy0 + lane) + 1], 0), min(ksy, H0 - mn));
            bys[2 * lane] = mn; bys[2 * lane + 1] = cnt;
            en = mn + cnt;
        }
        mn = wave_min_i(mn); en = wave_max_i(en);
        if (lane == 0) { span[2] = mn; span[3] = en; }
    }
    __syncthreads();
    const int cx0 = span[0], ncols = span[1] - cx0, ry0 = span[2], nrows = span[3] - ry0;
    if (ncols <= 0 || nrows <= 0 || ncols > COLS_MAX || nrows > ROWS_MAX) return;      // (uniform: not this geometry's tables)
    const int rowbytes = ncols * 3;
    const int pitch = (rowbytes + 15 + 15) & ~15;                      // a row may start up to 15 bytes into its first vector
    const int chunk = STAGE_BYTES / pitch;
    const uint8_t* fbase = frames + (size_t)frame * fstride + origin;

    for (int c0 = 0; c0 < nrows; c0 += chunk) {
        const int nr = min(chunk, nrows - c0);
        // ---- stage rows [ry0 + c0, ry0 + c0 + nr) x columns [cx0, cx0 + ncols): a wave per row, 16 bytes per lane
        for (int i = wv; i < nr; i += 4) {
            const uint8_t* g = fbase + (size_t)(ry0 + c0 + i) * gpitch + (size_t)cx0 * 3;
            const int sh = (int)((uintptr_t)g & 15);
            const u32x4* ga = (const u32x4*)(g - sh);                  // aligned down: every vector loaded holds a byte of the row,
            const int nvec = (sh + rowbytes + 15) >> 4;                // so it lies in a page the frames own
            for (int v = lane; v < nvec; v += 64) *(u32x4*)(stage + i * pitch + 16 * v) = ga[v];
        }
        __syncthreads();
        // ---- horizontal pass: thread = (output column, staged row)
        if (lane < ow_t) {
            const int mn = bxs[2 * lane], cnt = bxs[2 * lane + 1];
            const int32_t* kr = kxs + lane * KS_MAX;
            for (int i = wv; i < nr; i += 4) {
                const uint8_t* g = fbase + (size_t)(ry0 + c0 + i) * gpitch + (size_t)cx0 * 3;
                const uint8_t* p = stage + i * pitch + (int)((uintptr_t)g & 15) + (mn - cx0) * 3;
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                for (int t = 0; t < cnt; ++t) {
                    const int k = kr[t];
                    a0 += __mul24(k, (int)p[3 * t]);
                    a1 += __mul24(k, (int)p[3 * t + 1]);
                    a2 += __mul24(k, (int)p[3 * t + 2]);
                }
                uint8_t* o = hbuf + (c0 + i) * HP + lane * 3;
                o[0] = (uint8_t)min(max(a0 >> 22, 0), 255);
                o[1] = (uint8_t)min(max(a1 >> 22, 0), 255);
                o[2] = (uint8_t)min(max(a2 >> 22, 0), 255);
            }
        }
        __syncthreads();
    }

    // ---- vertical pass from the uint8 buffer: thread = (output column, output row)
    if (lane >= ow_t) return;
    for (int y = wv; y < oh_t; y += 4) {
        const int mn = bys[2 * y], cnt = bys[2 * y + 1];
        const int32_t* kr = kys + y * KS_MAX;
        const uint8_t* p = hbuf + (mn - ry0) * HP + lane * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < cnt; ++t) {
            const int k = kr[t];
            a0 += __mul24(k, (int)p[t * HP]);
            a1 += __mul24(k, (int)p[t * HP + 1]);
            a2 += __mul24(k, (int)p[t * HP + 2]);
        }
        const int r0 = min(max(a0 >> 22, 0), 255), r1 = min(max(a1 >> 22, 0), 255), r2 = min(max(a2 >> 22, 0), 255);
        const int oy = oy0 + y, ox = ox0 + lane;
        if (!PACK) {
            uint8_t* o = out8 + (((size_t)frame * h + oy) * w + ox) * 3;
            o[0] = (uint8_t)r0; o[1] = (uint8_t)r1; o[2] = (uint8_t)r2;
        } else {
            // ToTensor + Normalize: pack_u8_cams_kernel's expression (pack.hip), so the planes are the same bits
            const float v0 = ((float)r0 / 255.f - m0) / s0;
            const float v1 = ((float)r1 / 255.f - m1) / s1;
            const float v2 = ((float)r2 / 255.f - m2) / s2;
            bf16_t hh[4], ll[4];
            map_split1(v0, lo != nullptr, hh[0], ll[0]);
            map_split1(v1, lo != nullptr, hh[1], ll[1]);
            map_split1(v2, lo != nullptr, hh[2], ll[2]);
            hh[3] = 0; ll[3] = 0;
            const uint32_t im = frame / (uint32_t)ncam, cam = frame - im * (uint32_t)ncam;
            const int hp = h + 2 * pad, wp = ncam * w + 2 * pad;
            const size_t off = (((size_t)im * hp + oy + pad) * wp + (size_t)cam * w + ox + pad) * 4;
            u32x2 a = {pack2(hh[0], hh[1]), pack2(hh[2], hh[3])};
            *(u32x2*)(hi + off) = a;
            if (lo) { u32x2 c = {pack2(ll[0], ll[1]), pack2(ll[2], ll[3])}; *(u32x2*)(lo + off) = c; }
        }
    }
}

inline bool dim_ok(int in, int out) { return in >= 1 && out >= 1 && in <= MAX_DIM && out <= MAX_DIM; }

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter (support 1), in double
inline int ksize_of(int in, int out) {
    double fs = (double)in / (double)out;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(1.0 * fs) * 2 + 1;
}

// (H0, W0): the window's size; pitch / fstride: bytes between the rows / the frames of the full frames; (y0, x0): the window's origin
int launch(bool pack, const uint8_t* frames, int n, int ncam, int64_t pitch, int64_t fstride, int y0, int x0, int H0, int W0, int h,
           int w, const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by, uint8_t* out8, const float* mean3,
           const float* std3, int pad, void* hi, void* lo, void* stream) {
    if (!frames || !kx || !bx || !ky || !by || n <= 0 || ncam <= 0 || H0 <= 0 || W0 <= 0 || h <= 0 || w <= 0) return AGP_E_BADARG;
    if (pack ? (!hi || !mean3 || !std3 || pad < 0) : !out8) return AGP_E_BADARG;
    if (!dim_ok(H0, h) || !dim_ok(W0, w) || H0 > MAX_RATIO * h || W0 > MAX_RATIO * w) return AGP_E_UNSUPPORTED;
    // the window lies inside a frame: its rows inside the frame's rows, its last row inside the frame
    if (y0 < 0 || x0 < 0 || pitch <= 0 || fstride <= 0) return AGP_E_BADARG;
    if (3 * ((int64_t)x0 + W0) > pitch || ((int64_t)y0 + H0) * pitch > fstride) return AGP_E_BADARG;
    if (pitch > 3 * (int64_t)MAX_DIM) return AGP_E_UNSUPPORTED;
    const int ksx = ksize_of(W0, w), ksy = ksize_of(H0, h);
    if (ksx > KS_MAX || ksy > KS_MAX) return AGP_E_UNSUPPORTED;
    const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
    const int64_t blocks = (int64_t)n * ncam * tiles_x * tiles_y;
    if (blocks >= (1ll << 31) || (int64_t)n * ncam >= (1ll << 31)) return AGP_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const size_t origin = (size_t)y0 * (size_t)pitch + (size_t)x0 * 3;
    if (pack) {
        AGP_LAUNCH(resize_cams_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, frames, (size_t)fstride, origin,
                   (int)pitch, ncam, H0, W0, h, w, kx, bx, ksx, ky, by, ksy, tiles_x, tiles_y, (uint8_t*)nullptr, mean3[0], mean3[1],
                   mean3[2], std3[0], std3[1], std3[2], pad, (bf16_t*)hi, (bf16_t*)lo);
    } else {
        AGP_LAUNCH(resize_cams_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, frames, (size_t)fstride, origin,
                   (int)pitch, ncam, H0, W0, h, w, kx, bx, ksx, ky, by, ksy, tiles_x, tiles_y, out8, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 0,
                   (bf16_t*)nullptr, (bf16_t*)nullptr);
    }
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

}  // namespace agp_camera
using namespace agp_camera;

extern "C" int agp_resize_ksize(int in, int out) {
    if (!dim_ok(in, out)) return -1;
    return ksize_of(in, out);
}

extern "C" int agp_resize_coeffs(int in, int out, int32_t* k, int32_t* bounds) {
#pragma clang fp contract(off)      // Pillow's doubles, operation for operation
    if (!k || !bounds || !dim_ok(in, out)) return AGP_E_BADARG;
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        auto tap = [&](int x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            return a < 1.0 ? 1.0 - a : 0.0;
        };
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) ww += tap(x);
        int32_t* kr = k + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            const double wt = ww != 0.0 ? tap(x) / ww : tap(x);
            kr[x] = wt < 0 ? (int32_t)(-0.5 + wt * (double)(1 << 22)) : (int32_t)(0.5 + wt * (double)(1 << 22));
        }
        for (int x = xmax; x < ksize; ++x) kr[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return AGP_OK;
}

extern "C" int agp_resized_size(int h, int w, int size, int* oh, int* ow) {
    if (!oh || !ow || h <= 0 || w <= 0 || size <= 0) return AGP_E_BADARG;
    // torchvision Resize(int): the shorter edge becomes `size`, the longer int(size * long / short)
    const int sh = w <= h ? w : h, lg = w <= h ? h : w;
    const int64_t nl = (int64_t)((double)((int64_t)size * lg) / (double)sh);
    if (nl > INT32_MAX) return AGP_E_BADARG;
    if (w <= h) { *ow = size; *oh = (int)nl; }
    else { *oh = size; *ow = (int)nl; }
    return AGP_OK;
}

extern "C" int agp_resize_u8_cams(const uint8_t* frames, int n, int ncam, int H0, int W0, int h, int w, const int32_t* kx,
                                  const int32_t* bx, const int32_t* ky, const int32_t* by, uint8_t* out, void* stream) {
    return launch(false, frames, n, ncam, 3 * (int64_t)W0, 3 * (int64_t)W0 * H0, 0, 0, H0, W0, h, w, kx, bx, ky, by, out, nullptr,
                  nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int agp_resize_pack_u8_cams(const uint8_t* frames, int n, int ncam, int H0, int W0, int h, int w, const int32_t* kx,
                                       const int32_t* bx, const int32_t* ky, const int32_t* by, const float* mean3,
                                       const float* std3, int pad, void* hi, void* lo, void* stream) {
    return launch(true, frames, n, ncam, 3 * (int64_t)W0, 3 * (int64_t)W0 * H0, 0, 0, H0, W0, h, w, kx, bx, ky, by, nullptr, mean3,
                  std3, pad, hi, lo, stream);
}

extern "C" int agp_resize_u8_cams_roi(const uint8_t* frames, int n, int ncam, int64_t pitch, int64_t frame_stride, int y0, int x0,
                                      int ch, int cw, int h, int w, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                                      const int32_t* by, uint8_t* out, void* stream) {
    return launch(false, frames, n, ncam, pitch, frame_stride, y0, x0, ch, cw, h, w, kx, bx, ky, by, out, nullptr, nullptr, 0, nullptr,
                  nullptr, stream);
}

extern "C" int agp_resize_pack_u8_cams_roi(const uint8_t* frames, int n, int ncam, int64_t pitch, int64_t frame_stride, int y0, int x0,
                                           int ch, int cw, int h, int w, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                                           const int32_t* by, const float* mean3, const float* std3, int pad, void* hi, void* lo,
                                           void* stream) {
    return launch(true, frames, n, ncam, pitch, frame_stride, y0, x0, ch, cw, h, w, kx, bx, ky, by, nullptr, mean3, std3, pad, hi, lo,
                  stream);
}
