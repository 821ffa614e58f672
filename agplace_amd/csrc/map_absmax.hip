// max |x| over a halo-padded NHWC feature map in either storage format: the measuring instrument of the map-exponent
// calibration (agplace_amd/map_exponents.py).  One HBM pass, no workspace.
//
// The planes are read as ONE contiguous run, halo included: a map's halo is zero by contract (ops.SplitMap: zeroed at allocation,
// never written by a kernel) and |x| >= 0, so the halo cannot change the maximum, every wave instruction reads 1 KB of
// consecutive bytes and no thread divides.  Lanes load 16 bytes per plane (map_load8), four independent loads in flight per trip.
//
// The running maximum is kept as the BIT PATTERN of |x| in an unsigned integer: for non-negative floats the unsigned order of
// the patterns is the float order, +inf (0x7f800000) sorts above every finite value and every NaN pattern above +inf.  NaN
// therefore PROPAGATES: a map holding one reads back as NaN (v_max_u32 has no NaN-dropping rule, unlike v_max_f32), which the
// host refuses (map_exponents.choose_exponents).  Wave reduction by __shfl_xor, then ONE atomic max per wave on the word
// (relaxed, agent scope; a max commutes, so the result does not depend on arrival order).  The word ACCUMULATES across calls.
#include "common.hpp"

namespace agp_absmax {

constexpr int TPB = 256, UNROLL = 4;

__device__ __forceinline__ uint32_t absbits8(const bf16_t* hi, const bf16_t* lo, size_t off) {
    float v[8];
    map_load8(hi, lo, off, v);
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t b = __builtin_bit_cast(uint32_t, v[e]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    return m;
}

__global__ __launch_bounds__(TPB) void map_absmax_kernel(const bf16_t* __restrict__ hi, const bf16_t* __restrict__ lo,
                                                         int64_t vecs, uint32_t* __restrict__ word) {
    const int64_t step = (int64_t)gridDim.x * TPB;
    int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    uint32_t m = 0;
    // whole trips of UNROLL vectors per lane (each at stride `step`: consecutive lanes stay on consecutive 16-byte vectors)
    for (; t + (UNROLL - 1) * step < vecs; t += UNROLL * step) {
        uint32_t p[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) p[u] = absbits8(hi, lo, (size_t)(t + u * step) * 8);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) m = p[u] > m ? p[u] : m;
    }
    for (; t < vecs; t += step) {
        const uint32_t p = absbits8(hi, lo, (size_t)t * 8);
        m = p > m ? p : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0) __hip_atomic_fetch_max(word, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (a kernel, not a memset node: csrc/coords.hip)
__global__ void zero_floats_kernel(float* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

}  // namespace agp_absmax

extern "C" int agp_map_absmax(const void* hi, const void* lo, int n, int h, int w, int c, int pad, float* inout_max, void* stream) {
    if (!hi || !inout_max || n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 8 || pad < 0) return AGP_E_BADARG;
    const int64_t vecs = (int64_t)n * (h + 2 * pad) * (w + 2 * pad) * (c / 8);
    // 256 CUs x 8 blocks of 4 waves: enough loads in flight to cover HBM latency; smaller maps get one UNROLL trip per lane
    int64_t grid = (vecs + (int64_t)agp_absmax::TPB * agp_absmax::UNROLL - 1) / ((int64_t)agp_absmax::TPB * agp_absmax::UNROLL);
    if (grid > 256 * 8) grid = 256 * 8;
    AGP_LAUNCH(agp_absmax::map_absmax_kernel, dim3((unsigned)grid), dim3(agp_absmax::TPB), 0, (hipStream_t)stream,
               (const bf16_t*)hi, (const bf16_t*)lo, vecs, (uint32_t*)inout_max);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_map_absmax_reset(float* words, int n, void* stream) {
    if (!words || n <= 0) return AGP_E_BADARG;
    AGP_LAUNCH(agp_absmax::zero_floats_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, words, n);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}
