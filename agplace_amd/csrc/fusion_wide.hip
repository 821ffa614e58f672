// One-launch fixed-grid Neural-ODE solve at 384 columns (agp_fcode_wide_fwd): the inference kernel of FCODE(384).
//
// fcode_kernel (fusion.hip) keeps both split-bf16 planes of a 256 x 256 W in registers.  At 384 the two planes are 576 KiB,
// more than a CU's 512 KiB register file, so here only the `hi` plane is resident and the `lo` plane is streamed from L2
// once per f-evaluation (288 KiB, L2-resident after the first pass).
//
// Work shape: one workgroup of 8 waves (512 threads, two waves per SIMD, up to 256 registers each) owns 16 batch rows for the
// whole solve; no workgroup ever waits for another.  Wave w owns the three 16-feature tiles [48 w, 48 w + 48) over the FULL K:
//   * 36 resident `hi` fragments (3 tiles x 12 K-steps, 144 registers), loaded once;
//   * the `lo` fragments of the same (tile, K-step) pairs come through a ring of WRING K-steps (3 fragments each); the host lays
//     both planes out in this kernel's fragment order (ops.fcode_wide_planes), so one wave instruction reads 1 KiB of
//     consecutive bytes.  The first WRING K-steps of an evaluation are issued BEFORE the barrier that publishes the new state
//     (they do not depend on it); every later K-step is issued as soon as its ring slot has been consumed.
//   * no K split, hence no cross-wave sum: ONE barrier per f-evaluation, the state planes double-buffered in LDS as in fcode_kernel.
// Arithmetic as fcode_kernel: split-bf16 x3 (hi*lo, hi*hi, lo*hi in that order per K-step, K-steps ascending -- a fixed summation
// order, so a solve repeats bit for bit), fp32 state in registers (lane = batch row l & 15, features 48 w + 16 t + 4 (l >> 4) + r),
// fp32 dt, the stage combinations written exactly as there.
#include "fusion_common.hpp"

namespace agp_fusion {

constexpr int WD = 384;                    // columns
constexpr int WT = 512;                    // threads per workgroup (8 waves)
constexpr int WKS = WD / 32;               // 12 K-steps
constexpr int WTILES = 3;                  // 16-feature tiles per wave
constexpr int WRING = 3;                   // K-steps of `lo` fragments in flight
constexpr int WYRB = WD * 2 + 16;          // LDS row pitch of a state plane (+16 B: bank spread)
constexpr int WPLANES = 2 * 2 * FROWS * WYRB;                    // 50176 B
constexpr int wide_lds_bytes(int method) {                         // 51712 B; rk4 100864 B (more than 64 KB: agp_lds_attr)
    return WPLANES + WD * 4 + (method == AGP_ODE_RK4 ? 2 * WTILES * WT * 16 : 0);
}

struct State3 {
    f32x4 t[WTILES];
};
__device__ __forceinline__ State3 operator+(const State3& a, const State3& b) {
    State3 o;
#pragma unroll
    for (int i = 0; i < WTILES; ++i) o.t[i] = a.t[i] + b.t[i];
    return o;
}
__device__ __forceinline__ State3 operator-(const State3& a, const State3& b) {
    State3 o;
#pragma unroll
    for (int i = 0; i < WTILES; ++i) o.t[i] = a.t[i] - b.t[i];
    return o;
}
__device__ __forceinline__ State3 operator*(const State3& a, float s) {
    State3 o;
#pragma unroll
    for (int i = 0; i < WTILES; ++i) o.t[i] = a.t[i] * s;
    return o;
}
__device__ __forceinline__ State3 operator*(float s, const State3& a) { return a * s; }

template <int ACT, int METHOD>
__global__ __launch_bounds__(WT) void fcode_wide_kernel(const float* __restrict__ x, const float* __restrict__ add1,
                                                        const float* __restrict__ add2, const bf16x8* __restrict__ wf_hi,
                                                        const bf16x8* __restrict__ wf_lo, const float* __restrict__ bias, int b,
                                                        OdeSteps steps, int nsteps, float* __restrict__ y) {
    // dynamic LDS (wide_lds_bytes): the state planes [buf][plane], the bias, and for rk4 two slots for each thread's own k_i
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const sbias = (float*)(smem + WPLANES);
    f32x4* const stash = (f32x4*)(smem + WPLANES + WD * 4);      // [slot][tile][thread]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int brow = blockIdx.x * FROWS + (lane & 15);
    const int nf = wave * (16 * WTILES) + (lane >> 4) * 4;      // this lane's first feature of tile 0
    const bool live = brow < b;

    // fragment-major planes: [wave][ks][tile][lane] of 16 bytes = W[48 wave + 16 tile + (lane & 15)][32 ks + 8 (lane >> 4) .. + 7]
    const bf16x8* fh = wf_hi + (size_t)wave * (WKS * WTILES * 64) + lane;
    const bf16x8* fl = wf_lo + (size_t)wave * (WKS * WTILES * 64) + lane;
    bf16x8 wh[WKS][WTILES];
#pragma unroll
    for (int ks = 0; ks < WKS; ++ks)
#pragma unroll
        for (int t = 0; t < WTILES; ++t) wh[ks][t] = fh[(ks * WTILES + t) * 64];

    if (tid < WD) sbias[tid] = bias ? bias[tid] : 0.f;     // (published by the first evaluation's barrier)
    State3 yv;
#pragma unroll
    for (int t = 0; t < WTILES; ++t) {
        yv.t[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (live) {
            const size_t g = (size_t)brow * WD + nf + 16 * t;
            yv.t[t] = *(const f32x4*)(x + g);
            if (add1) yv.t[t] += *(const f32x4*)(add1 + g);
            if (add2) yv.t[t] += *(const f32x4*)(add2 + g);
        }
    }

    int buf = 0;
    const int soff = (lane & 15) * WYRB + nf * 2;                 // where this lane's 4 features of tile 0 go in a plane
    const int boff = (lane & 15) * WYRB + (lane >> 4) * 16;       // this lane's B fragment of K-step 0
    auto feval = [&](const State3& state) -> State3 {
        // (the pointer is made opaque once per evaluation and once per K-step: W is loop-invariant, and a compiler that knows it
        // hoists all 36 `lo` fragments out of the step loop -- 144 more registers, i.e. scratch)
        const bf16x8* fp = fl;
        asm volatile("" : "+v"(fp));
        bf16x8 ring[WRING][WTILES];
#pragma unroll
        for (int c = 0; c < WRING; ++c)
#pragma unroll
            for (int t = 0; t < WTILES; ++t) ring[c][t] = fp[(c * WTILES + t) * 64];
        char* hi = smem + buf * (2 * FROWS * WYRB);
        char* lo = hi + FROWS * WYRB;
#pragma unroll
        for (int t = 0; t < WTILES; ++t) {
            bf16_t h[4], l[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) split_bf16(state.t[t][r], h[r], l[r]);
            *(u32x2*)(hi + soff + 32 * t) = u32x2{pack2(h[0], h[1]), pack2(h[2], h[3])};
            *(u32x2*)(lo + soff + 32 * t) = u32x2{pack2(l[0], l[1]), pack2(l[2], l[3])};
        }
        __syncthreads();
        State3 acc;
#pragma unroll
        for (int t = 0; t < WTILES; ++t) acc.t[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < WKS; ++ks) {
            const bf16x8 bh = *(const bf16x8*)(hi + boff + ks * 64);
            const bf16x8 bl = *(const bf16x8*)(lo + boff + ks * 64);
            // (tile-interleaved: an accumulator is touched every third MFMA)
#pragma unroll
            for (int t = 0; t < WTILES; ++t) acc.t[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][t], bl, acc.t[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < WTILES; ++t) acc.t[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][t], bh, acc.t[t], 0, 0, 0);
            // (the streamed plane last: its loads have six more MFMAs to arrive)
#pragma unroll
            for (int t = 0; t < WTILES; ++t) acc.t[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[ks % WRING][t], bh, acc.t[t], 0, 0, 0);
            if (ks + WRING < WKS) {
                asm volatile("" : "+v"(fp));
#pragma unroll
                for (int t = 0; t < WTILES; ++t) ring[ks % WRING][t] = fp[((ks + WRING) * WTILES + t) * 64];
            }
        }
        buf ^= 1;
        State3 o;
#pragma unroll
        for (int t = 0; t < WTILES; ++t) {
            o.t[t] = act4<ACT>(acc.t[t] + *(const f32x4*)(sbias + nf + 16 * t));
            __builtin_amdgcn_sched_barrier(0);      // one tile at a time: twelve interleaved IEEE divisions (sigmoid) cost scratch
        }
        return o;
    };
    // a stage derivative that is needed again after the next evaluation waits in LDS, not in registers (the 144 registers of
    // W leave room for ONE state-sized vector beside the evaluation's own): a thread reads back only what it wrote itself
    auto put = [&](int slot, const State3& v) {
#pragma unroll
        for (int t = 0; t < WTILES; ++t) stash[(slot * WTILES + t) * WT + tid] = v.t[t];
    };
    auto get = [&](int slot) -> State3 {
        State3 v;
#pragma unroll
        for (int t = 0; t < WTILES; ++t) v.t[t] = stash[(slot * WTILES + t) * WT + tid];
        return v;
    };

    const float third = 1.f / 3.f;
    for (int s = 0; s < nsteps; ++s) {
        const float dt = steps.dt[s];
        if constexpr (METHOD == AGP_ODE_EULER) {
            const State3 k1 = feval(yv);
            yv = yv + dt * k1;
        } else if constexpr (METHOD == AGP_ODE_MIDPOINT) {
            const State3 k1 = feval(yv);
            const State3 k2 = feval(yv + k1 * (0.5f * dt));
            yv = yv + dt * k2;
        } else {  // rk4, 3/8 rule (torchdiffeq rk4_alt_step_func); the sums grouped as in fcode_kernel
            State3 k1 = feval(yv);
            put(0, k1);
            State3 k2 = feval(yv + dt * k1 * third);
            put(1, k2);
            k1 = get(0);
            const State3 k3 = feval(yv + dt * (k2 - k1 * third));
            k1 = get(0);
            k2 = get(1);
            const State3 u4 = yv + dt * (k1 - k2 + k3);
            put(0, k1 + 3.f * (k2 + k3));                   // k1, k2, k3 are dead before the last evaluation
            const State3 k4 = feval(u4);
            yv = yv + (get(0) + k4) * dt * 0.125f;
        }
    }
    if (live) {
#pragma unroll
        for (int t = 0; t < WTILES; ++t) *(f32x4*)(y + (size_t)brow * WD + nf + 16 * t) = yv.t[t];
    }
}

}  // namespace agp_fusion
using namespace agp_fusion;

extern "C" int agp_fcode_wide_fwd(const float* x, const float* add1, const float* add2, const void* wf_hi, const void* wf_lo,
                                  const float* bias, int b, int d, int act, int method, const float* dt, int nsteps, float* y,
                                  void* stream) {
    if (!x || !wf_hi || !wf_lo || !y || !dt || b <= 0 || d <= 0 || nsteps <= 0 || nsteps > 64) return AGP_E_BADARG;
    if (method < AGP_ODE_EULER || method > AGP_ODE_RK4) return AGP_E_BADARG;
    if (d != WD) return AGP_E_UNSUPPORTED;
    OdeSteps st;
    for (int i = 0; i < 64; ++i) st.dt[i] = i < nsteps ? dt[i] : 0.f;
    const dim3 grid((b + FROWS - 1) / FROWS), blk(WT);
    hipStream_t s = (hipStream_t)stream;
    const bf16x8* wh = (const bf16x8*)wf_hi;
    const bf16x8* wl = (const bf16x8*)wf_lo;
    static std::atomic<uint64_t> attr_done[4][3];
#define AGP_WIDE_CASE(A, M)                                                                                                 \
    case (A) * 3 + (M):                                                                                                     \
        if (!agp_lds_attr((const void*)fcode_wide_kernel<A, M>, wide_lds_bytes(M), attr_done[A][M])) return AGP_E_LAUNCH;   \
        AGP_LAUNCH((fcode_wide_kernel<A, M>), grid, blk, wide_lds_bytes(M), s, x, add1, add2, wh, wl, bias, b, st, nsteps, y); \
        break;
    if (act < AGP_ACT_ID || act > AGP_ACT_SIGMOID) return AGP_E_BADARG;
    switch (act * 3 + method) {
        AGP_WIDE_CASE(AGP_ACT_ID, AGP_ODE_EULER) AGP_WIDE_CASE(AGP_ACT_ID, AGP_ODE_MIDPOINT) AGP_WIDE_CASE(AGP_ACT_ID, AGP_ODE_RK4)
        AGP_WIDE_CASE(AGP_ACT_RELU, AGP_ODE_EULER) AGP_WIDE_CASE(AGP_ACT_RELU, AGP_ODE_MIDPOINT) AGP_WIDE_CASE(AGP_ACT_RELU, AGP_ODE_RK4)
        AGP_WIDE_CASE(AGP_ACT_TANH, AGP_ODE_EULER) AGP_WIDE_CASE(AGP_ACT_TANH, AGP_ODE_MIDPOINT) AGP_WIDE_CASE(AGP_ACT_TANH, AGP_ODE_RK4)
        AGP_WIDE_CASE(AGP_ACT_SIGMOID, AGP_ODE_EULER) AGP_WIDE_CASE(AGP_ACT_SIGMOID, AGP_ODE_MIDPOINT) AGP_WIDE_CASE(AGP_ACT_SIGMOID, AGP_ODE_RK4)
        default: return AGP_E_BADARG;
    }
#undef AGP_WIDE_CASE
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}
