// Camera front end, colour jitter: torchvision's ColorJitter on the resized uint8 tiles [n * ncam][h][w][3], one
// parameter record per frame in device memory (colour.hpp: up to four ops in an order, three fp32 factors, a hue byte shift),
// Pillow's bytes.  Three launches, none of which needs the host to look at a parameter:
//   zero    the per-frame sums (a kernel, not a memset node: DESIGN.md section 0)
//   stats   frames WITH contrast: every pixel through the ops that precede contrast, sum(L) per frame -- uint32 partial sums per
//           thread, a 64-bit sum per workgroup, ONE 64-bit integer atomic add per workgroup (exact, order-independent);
//           workgroups of frames without contrast return at once
//   apply   every pixel through its frame's ops, the contrast grey level from the sum; writes the uint8 tiles, or the stem's
//           NHWC4 map with pack_u8_cams_kernel's normalisation (the jittered bytes are then never stored)
// Pointwise and memory-bound except for the hue op, whose HSV round trip is Pillow's mix of fp32 and fp64.
#include "common.hpp"
#include "colour.hpp"

namespace agp_jitter {
using namespace agp_colour;

constexpr int STAT_PIXELS = 8192;       // pixels of a frame per statistics workgroup (256 threads x 32)

__global__ __launch_bounds__(256) void zero_sums_kernel(unsigned long long* __restrict__ sums, int nframes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nframes) sums[i] = 0ull;
}

__device__ __forceinline__ rgb8 load_px(const uint8_t* p) {
    rgb8 v = {(int)p[0], (int)p[1], (int)p[2]};
    return v;
}

// grid = (workgroups per frame, frames)
__global__ __launch_bounds__(256) void jitter_stats_kernel(const uint8_t* __restrict__ tiles, int npix,
                                                           const float* __restrict__ params,
                                                           unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[4];
    const uint32_t frame = blockIdx.y;
    const record c = load_record(params + (size_t)frame * RECORD);
    const int kc = contrast_pos(c);
    if (kc < 0) return;                                             // (uniform over the workgroup)
    const uint8_t* f = tiles + (size_t)frame * npix * 3;
    const int p0 = blockIdx.x * STAT_PIXELS, p1 = min(npix, p0 + STAT_PIXELS);
    uint32_t acc = 0;                                               // <= 32 pixels x 255
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) acc += (uint32_t)luma(apply_ops(load_px(f + (size_t)p * 3), c, 0, kc, 0));
    unsigned long long s = acc;
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + frame, part[0] + part[1] + part[2] + part[3]);
}

// PACK == false: out8 = uint8 [n * ncam][h][w][3].  PACK == true: hi / lo as resize_cams_kernel<true> (camera.hip) writes them.
// grid = (workgroups per frame, frames), a thread per pixel
template <bool PACK>
__global__ __launch_bounds__(256) void jitter_apply_kernel(const uint8_t* __restrict__ tiles, int ncam, int h, int w,
                                                           const float* __restrict__ params,
                                                           const unsigned long long* __restrict__ sums, uint8_t* __restrict__ out8,
                                                           float m0, float m1, float m2, float s0, float s1, float s2, int pad,
                                                           bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
    const uint32_t frame = blockIdx.y;
    const int npix = h * w;
    const int p = blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= npix) return;
    const record c = load_record(params + (size_t)frame * RECORD);
    const int m = contrast_pos(c) >= 0 ? contrast_mean(sums[frame], (uint64_t)npix) : 0;
    const size_t src = ((size_t)frame * npix + p) * 3;
    const rgb8 v = apply_ops(load_px(tiles + src), c, 0, 4, m);
    if (!PACK) {
        out8[src] = (uint8_t)v.r; out8[src + 1] = (uint8_t)v.g; out8[src + 2] = (uint8_t)v.b;
    } else {
        // ToTensor + Normalize: pack_u8_cams_kernel's expression (pack.hip), so the planes are the same bits
        const float v0 = ((float)v.r / 255.f - m0) / s0;
        const float v1 = ((float)v.g / 255.f - m1) / s1;
        const float v2 = ((float)v.b / 255.f - m2) / s2;
        bf16_t hh[4], ll[4];
        map_split1(v0, lo != nullptr, hh[0], ll[0]);
        map_split1(v1, lo != nullptr, hh[1], ll[1]);
        map_split1(v2, lo != nullptr, hh[2], ll[2]);
        hh[3] = 0; ll[3] = 0;
        const int oy = p / w, ox = p - oy * w;
        const uint32_t im = frame / (uint32_t)ncam, cam = frame - im * (uint32_t)ncam;
        const int hp = h + 2 * pad, wp = ncam * w + 2 * pad;
        const size_t off = (((size_t)im * hp + oy + pad) * wp + (size_t)cam * w + ox + pad) * 4;
        u32x2 a = {pack2(hh[0], hh[1]), pack2(hh[2], hh[3])};
        *(u32x2*)(hi + off) = a;
        if (lo) { u32x2 b = {pack2(ll[0], ll[1]), pack2(ll[2], ll[3])}; *(u32x2*)(lo + off) = b; }
    }
}

int launch(bool pack, const uint8_t* tiles, int n, int ncam, int h, int w, const float* params, void* sums, uint8_t* out8,
           const float* mean3, const float* std3, int pad, void* hi, void* lo, void* stream) {
    if (!tiles || !params || !sums || n <= 0 || ncam <= 0 || h <= 0 || w <= 0) return AGP_E_BADARG;
    if (pack ? (!hi || !mean3 || !std3 || pad < 0) : !out8) return AGP_E_BADARG;
    const int64_t nframes = (int64_t)n * ncam, npix = (int64_t)h * w;
    // grid.y holds the frames; a frame's pixel index is an int
    if (nframes > 65535 || npix > (1 << 30)) return AGP_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* sm = (unsigned long long*)sums;
    AGP_LAUNCH(zero_sums_kernel, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, s, sm, (int)nframes);
    AGP_CHECK_LAUNCH();
    AGP_LAUNCH(jitter_stats_kernel, dim3((unsigned)((npix + STAT_PIXELS - 1) / STAT_PIXELS), (unsigned)nframes), dim3(256), 0, s,
               tiles, (int)npix, params, sm);
    AGP_CHECK_LAUNCH();
    const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)nframes);
    if (pack) {
        AGP_LAUNCH(jitter_apply_kernel<true>, grid, dim3(256), 0, s, tiles, ncam, h, w, params, sm, (uint8_t*)nullptr, mean3[0],
                   mean3[1], mean3[2], std3[0], std3[1], std3[2], pad, (bf16_t*)hi, (bf16_t*)lo);
    } else {
        AGP_LAUNCH(jitter_apply_kernel<false>, grid, dim3(256), 0, s, tiles, ncam, h, w, params, sm, out8, 0.f, 0.f, 0.f, 1.f, 1.f,
                   1.f, 0, (bf16_t*)nullptr, (bf16_t*)nullptr);
    }
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

}  // namespace agp_jitter

extern "C" int agp_center_crop_origin(int H0, int W0, int c, int* top, int* left) {
    if (!top || !left || H0 <= 0 || W0 <= 0 || c <= 0) return AGP_E_BADARG;
    if (c > H0 || c > W0) return AGP_E_UNSUPPORTED;              // torchvision pads with black there: not built
    *top = agp_colour::crop_origin(H0, c);
    *left = agp_colour::crop_origin(W0, c);
    return AGP_OK;
}

extern "C" int agp_jitter_u8_cams(const uint8_t* tiles, int n, int ncam, int h, int w, const float* params, void* sums,
                                  uint8_t* out, void* stream) {
    return agp_jitter::launch(false, tiles, n, ncam, h, w, params, sums, out, nullptr, nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int agp_jitter_pack_u8_cams(const uint8_t* tiles, int n, int ncam, int h, int w, const float* params, void* sums,
                                       const float* mean3, const float* std3, int pad, void* hi, void* lo, void* stream) {
    return agp_jitter::launch(true, tiles, n, ncam, h, w, params, sums, nullptr, mean3, std3, pad, hi, lo, stream);
}
