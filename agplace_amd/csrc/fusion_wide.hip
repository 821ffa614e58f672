// One-launch fixed-grid Neural-ODE solve at 384 columns: agp_fcode_wide_fwd, the inference kernel of FCODE(384); the same
// kernel recording its trajectory (agp_fcode_wide_fwd_traj) and the backward through that record (agp_fcode_wide_bwd, at the
// end of this file) for training.
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
#include <type_traits>
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

// acc[t] = sum_k M[48 w + 16 t + ..][k] * v[row][k] for this lane's twelve elements of v = M's input vector: v goes into the
// planes `hi` / `lo` of LDS as split bf16 (this lane's 4 elements of tile 0 at soff), ONE barrier publishes it, then three
// products per K-step -- hi*lo, hi*hi, lo*hi, K-steps ascending, one accumulator chain per tile: a fixed order.  wh = M's resident
// `hi` fragments, fl = this wave's streamed `lo` fragments (a uniform pointer; the lane's own at + lane).  The forward's f
// (M = W) and the backward's gz W (M = W^T).
__device__ __forceinline__ State3 wide_product(const bf16x8 (&wh)[WKS][WTILES], const bf16x8* fl, int lane, char* hi, char* lo,
                                               int soff, int boff, const State3& v) {
    // (the lane index is made opaque once per evaluation and once per K-step: W is loop-invariant, and a compiler that knows it
    // hoists all 36 `lo` fragments out of the step loop -- 144 more registers, i.e. scratch.  What is opaque is the 32-bit lane
    // index under a uniform pointer, one register across an evaluation; an opaque per-lane 64-bit pointer was a register pair,
    // and more pairs derived from it per 4 KiB of fragments, which the backward kernel below has no room for.)
    unsigned fo = lane;
    asm volatile("" : "+v"(fo));
    const bf16x8* fp = fl + fo;
    bf16x8 ring[WRING][WTILES];
#pragma unroll
    for (int c = 0; c < WRING; ++c)
#pragma unroll
        for (int t = 0; t < WTILES; ++t) ring[c][t] = fp[(c * WTILES + t) * 64];
#pragma unroll
    for (int t = 0; t < WTILES; ++t) {
        bf16_t h[4], l[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) split_bf16(v.t[t][r], h[r], l[r]);
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
            asm volatile("" : "+v"(fo));
            fp = fl + fo;
#pragma unroll
            for (int t = 0; t < WTILES; ++t) ring[ks % WRING][t] = fp[((ks + WRING) * WTILES + t) * 64];
        }
    }
    return acc;
}

// REC: also record the trajectory the backward reads (agp_fcode_wide_fwd_traj) -- traj[s][0][b][384] = y before step s,
// traj[s][1 + i][b][384] = k_i, rows < b only; the stores are the only difference, so y has the bits of the other instantiation.
template <int ACT, int METHOD, bool REC>
__global__ __launch_bounds__(WT) void fcode_wide_kernel(const float* __restrict__ x, const float* __restrict__ add1,
                                                        const float* __restrict__ add2, const bf16x8* __restrict__ wf_hi,
                                                        const bf16x8* __restrict__ wf_lo, const float* __restrict__ bias, int b,
                                                        OdeSteps steps, int nsteps, float* __restrict__ y,
                                                        float* __restrict__ traj) {
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
    const bf16x8* fl = wf_lo + (size_t)wave * (WKS * WTILES * 64);
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
        char* hi = smem + buf * (2 * FROWS * WYRB);
        const State3 acc = wide_product(wh, fl, lane, hi, hi + FROWS * WYRB, soff, boff, state);
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

    constexpr int NSLOT = 1 + (METHOD == AGP_ODE_EULER ? 1 : (METHOD == AGP_ODE_MIDPOINT ? 2 : 4));
    auto rec = [&](int s, int slot, const State3& v) {
        if constexpr (REC) {
            if (live) {
                float* p = traj + ((size_t)(s * NSLOT + slot) * b + brow) * WD + nf;
#pragma unroll
                for (int t = 0; t < WTILES; ++t) *(f32x4*)(p + 16 * t) = v.t[t];
            }
        }
    };

    const float third = 1.f / 3.f;
    for (int s = 0; s < nsteps; ++s) {
        const float dt = steps.dt[s];
        rec(s, 0, yv);
        if constexpr (METHOD == AGP_ODE_EULER) {
            const State3 k1 = feval(yv);
            rec(s, 1, k1);
            yv = yv + dt * k1;
        } else if constexpr (METHOD == AGP_ODE_MIDPOINT) {
            const State3 k1 = feval(yv);
            rec(s, 1, k1);
            const State3 k2 = feval(yv + k1 * (0.5f * dt));
            rec(s, 2, k2);
            yv = yv + dt * k2;
        } else {  // rk4, 3/8 rule (torchdiffeq rk4_alt_step_func); the sums grouped as in fcode_kernel
            State3 k1 = feval(yv);
            put(0, k1);
            rec(s, 1, k1);
            State3 k2 = feval(yv + dt * k1 * third);
            put(1, k2);
            rec(s, 2, k2);
            k1 = get(0);
            const State3 k3 = feval(yv + dt * (k2 - k1 * third));
            rec(s, 3, k3);
            k1 = get(0);
            k2 = get(1);
            const State3 u4 = yv + dt * (k1 - k2 + k3);
            put(0, k1 + 3.f * (k2 + k3));                   // k1, k2, k3 are dead before the last evaluation
            const State3 k4 = feval(u4);
            rec(s, 4, k4);
            yv = yv + (get(0) + k4) * dt * 0.125f;
        }
    }
    if (live) {
#pragma unroll
        for (int t = 0; t < WTILES; ++t) *(f32x4*)(y + (size_t)brow * WD + nf + 16 * t) = yv.t[t];
    }
}

// Backward of the recorded solve: the recurrences at the head of fusion_bwd.hip (fcode_bwd_state_kernel) in the work shape above.
// One workgroup of 8 waves per 16 batch rows, wave w owns features [48 w, 48 w + 48), W^T's `hi` fragments resident, its `lo`
// fragments streamed; gs = gz W is wide_product on W^T's planes (ops.fcode_wide_planes_t).  A lane owns twelve features of its
// row, so beside an evaluation there is room for ONE state-sized vector: the adjoint a.  Everything else of a step is formed one
// feature tile at a time from the trajectory; rk4's gs4 and gs3, which two later stages read again, wait in LDS (a thread reads
// back only what it wrote itself).  Every (gz_i, s_i) pair goes to workspace row (s stages + i) Bp + brow, rows >= b as zeros
// (their loads are replaced by zeros, and every quantity of a row is a sum of products of that row's own): the weight
// gradient's GEMM reads all Bp rows of a block.
constexpr int wide_bwd_lds_bytes(int method) {                     // 50176 B; rk4 99328 B (more than 64 KB: agp_lds_attr)
    return WPLANES + (method == AGP_ODE_RK4 ? 2 * WTILES * WT * 16 : 0);
}

template <int ACT, int METHOD>
__global__ __launch_bounds__(WT) void fcode_wide_bwd_kernel(const float* __restrict__ traj, const float* __restrict__ gy,
                                                            const bf16x8* __restrict__ wtf_hi, const bf16x8* __restrict__ wtf_lo,
                                                            int b, OdeSteps steps, int nsteps, float* __restrict__ gx,
                                                            float* __restrict__ GZ, float* __restrict__ S, int Bp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* const stash = (f32x4*)(smem + WPLANES);                // rk4: [slot][tile][thread]
    constexpr int NST = METHOD == AGP_ODE_EULER ? 1 : (METHOD == AGP_ODE_MIDPOINT ? 2 : 4), NSLOT = 1 + NST;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int brow = blockIdx.x * FROWS + (lane & 15);
    const int nf = wave * (16 * WTILES) + (lane >> 4) * 4;
    const bool live = brow < b;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    const bf16x8* fh = wtf_hi + (size_t)wave * (WKS * WTILES * 64) + lane;
    const bf16x8* fl = wtf_lo + (size_t)wave * (WKS * WTILES * 64);
    bf16x8 wh[WKS][WTILES];
#pragma unroll
    for (int ks = 0; ks < WKS; ++ks)
#pragma unroll
        for (int t = 0; t < WTILES; ++t) wh[ks][t] = fh[(ks * WTILES + t) * 64];

    int buf = 0;
    const int soff = (lane & 15) * WYRB + nf * 2;
    const int boff = (lane & 15) * WYRB + (lane >> 4) * 16;
    auto times_w = [&](const State3& gz) -> State3 {
        char* hi = smem + buf * (2 * FROWS * WYRB);
        const State3 gs = wide_product(wh, fl, lane, hi, hi + FROWS * WYRB, soff, boff, gz);
        buf ^= 1;
        return gs;
    };
    // this workgroup's rows within a [rows][384] block: a uniform base plus this lane's 32-bit BYTE offset (a scalar base and a
    // 32-bit lane offset is one addressing mode; a 64-bit lane address is two registers per access in flight); tile t at + 64 t
    const size_t rbase = (size_t)blockIdx.x * (FROWS * WD);
    // a row beyond b reads the trajectory of row b - 1 (every workgroup has a live row) and discards it: no branch round a load
    // (lo, lk: the two lane offsets, made opaque once per stage -- the addresses of a step are loop-invariant, and a compiler that
    // knows it keeps them all as 64-bit pairs across the step loop: scratch)
    unsigned lo = ((lane & 15) * WD + nf) * 4, lk = (((live ? brow : b - 1) - blockIdx.x * FROWS) * WD + nf) * 4;
    auto stage = [&]() {
        __builtin_amdgcn_sched_barrier(0);      // (and no load of the next stage moves up into the product before it)
        asm volatile("" : "+v"(lo), "+v"(lk));
    };
    auto ld = [&](int s, int slot, int t) -> f32x4 {
        const char* p = (const char*)(traj + ((size_t)(s * NSLOT + slot) * b * WD + rbase));
        const f32x4 v = *(const f32x4*)(p + lk + 64 * t);
        return live ? v : zero4;
    };
    auto emit = [&](int s, int i, int t, const f32x4& gz, const f32x4& sin) {
        const size_t r = (size_t)(s * NST + i) * Bp * WD + rbase;
        *(f32x4*)((char*)(GZ + r) + lo + 64 * t) = gz;
        *(f32x4*)((char*)(S + r) + lo + 64 * t) = sin;
    };
    auto put = [&](int slot, int t, const f32x4& v) { stash[(slot * WTILES + t) * WT + tid] = v; };
    auto get = [&](int slot, int t) -> f32x4 { return stash[(slot * WTILES + t) * WT + tid]; };

    State3 a;
#pragma unroll
    for (int t = 0; t < WTILES; ++t) a.t[t] = live ? *(const f32x4*)((const char*)(gy + rbase) + lo + 64 * t) : zero4;
    const float third = 1.f / 3.f;
    for (int s = nsteps - 1; s >= 0; --s) {
        const float dt = steps.dt[s];
        State3 gz;
        if constexpr (METHOD == AGP_ODE_EULER) {
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                gz.t[t] = (dt * a.t[t]) * dact_from_output<ACT>(ld(s, 1, t));
                emit(s, 0, t, gz.t[t], ld(s, 0, t));
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            a = a + times_w(gz);
        } else if constexpr (METHOD == AGP_ODE_MIDPOINT) {
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                gz.t[t] = (dt * a.t[t]) * dact_from_output<ACT>(ld(s, 2, t));
                emit(s, 1, t, gz.t[t], ld(s, 0, t) + ld(s, 1, t) * (0.5f * dt));
                __builtin_amdgcn_sched_barrier(0);
            }
            const State3 gs2 = times_w(gz);
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                gz.t[t] = ((0.5f * dt) * gs2.t[t]) * dact_from_output<ACT>(ld(s, 1, t));
                emit(s, 0, t, gz.t[t], ld(s, 0, t));
                a.t[t] = a.t[t] + gs2.t[t];
                __builtin_amdgcn_sched_barrier(0);
            }
            a = a + times_w(gz);
        } else {
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                const f32x4 k1 = ld(s, 1, t), k2 = ld(s, 2, t), k3 = ld(s, 3, t);
                gz.t[t] = ((0.125f * dt) * a.t[t]) * dact_from_output<ACT>(ld(s, 4, t));
                emit(s, 3, t, gz.t[t], ld(s, 0, t) + dt * (k1 - k2 + k3));
                __builtin_amdgcn_sched_barrier(0);
            }
            const State3 gs4 = times_w(gz);
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                const f32x4 k1 = ld(s, 1, t), k2 = ld(s, 2, t);
                put(0, t, gs4.t[t]);
                gz.t[t] = ((0.375f * dt) * a.t[t] + dt * gs4.t[t]) * dact_from_output<ACT>(ld(s, 3, t));
                emit(s, 2, t, gz.t[t], ld(s, 0, t) + dt * (k2 - k1 * third));
                __builtin_amdgcn_sched_barrier(0);
            }
            const State3 gs3 = times_w(gz);
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                const f32x4 k1 = ld(s, 1, t);
                put(1, t, gs3.t[t]);
                gz.t[t] = ((0.375f * dt) * a.t[t] + dt * (gs3.t[t] - get(0, t))) * dact_from_output<ACT>(ld(s, 2, t));
                emit(s, 1, t, gz.t[t], ld(s, 0, t) + dt * k1 * third);
                __builtin_amdgcn_sched_barrier(0);
            }
            const State3 gs2 = times_w(gz);
            stage();
#pragma unroll
            for (int t = 0; t < WTILES; ++t) {
                const f32x4 g4 = get(0, t), g3 = get(1, t);
                gz.t[t] = ((0.125f * dt) * a.t[t] + dt * (g4 - third * g3 + third * gs2.t[t])) * dact_from_output<ACT>(ld(s, 1, t));
                emit(s, 0, t, gz.t[t], ld(s, 0, t));
                a.t[t] = a.t[t] + g4 + g3 + gs2.t[t];
                __builtin_amdgcn_sched_barrier(0);
            }
            a = a + times_w(gz);
        }
    }
    stage();
    if (live) {
#pragma unroll
        for (int t = 0; t < WTILES; ++t) *(f32x4*)((char*)(gx + rbase) + lo + 64 * t) = a.t[t];
    }
}

}  // namespace agp_fusion
using namespace agp_fusion;

// fn(std::integral_constant<int, ACT>{}, std::integral_constant<int, METHOD>{}) for a checked activation and fixed-grid method:
// one kernel instantiation each
template <class F>
static int by_act_method(int act, int method, F&& fn) {
    auto by_method = [&](auto A) -> int {
        switch (method) {
            case AGP_ODE_EULER: return fn(A, std::integral_constant<int, AGP_ODE_EULER>{});
            case AGP_ODE_MIDPOINT: return fn(A, std::integral_constant<int, AGP_ODE_MIDPOINT>{});
            default: return fn(A, std::integral_constant<int, AGP_ODE_RK4>{});
        }
    };
    switch (act) {
        case AGP_ACT_ID: return by_method(std::integral_constant<int, AGP_ACT_ID>{});
        case AGP_ACT_RELU: return by_method(std::integral_constant<int, AGP_ACT_RELU>{});
        case AGP_ACT_TANH: return by_method(std::integral_constant<int, AGP_ACT_TANH>{});
        default: return by_method(std::integral_constant<int, AGP_ACT_SIGMOID>{});
    }
}

static bool wide_sizes_ok(int b, int d, int method, int nsteps) {
    return b > 0 && d == WD && nsteps >= 1 && nsteps <= 64 && method >= AGP_ODE_EULER && method <= AGP_ODE_RK4;
}

template <bool REC>
static int wide_fwd(const float* x, const float* add1, const float* add2, const void* wf_hi, const void* wf_lo, const float* bias,
                    int b, int d, int act, int method, const float* dt, int nsteps, float* y, float* traj, void* stream) {
    if (!x || !wf_hi || !wf_lo || !y || !dt || (REC && !traj) || b <= 0 || d <= 0 || nsteps <= 0 || nsteps > 64) return AGP_E_BADARG;
    if (method < AGP_ODE_EULER || method > AGP_ODE_RK4) return AGP_E_BADARG;
    if (d != WD) return AGP_E_UNSUPPORTED;
    if (act < AGP_ACT_ID || act > AGP_ACT_SIGMOID) return AGP_E_BADARG;
    OdeSteps st;
    for (int i = 0; i < 64; ++i) st.dt[i] = i < nsteps ? dt[i] : 0.f;
    const dim3 grid((b + FROWS - 1) / FROWS), blk(WT);
    return by_act_method(act, method, [&](auto A, auto M) -> int {
        constexpr int METHOD = decltype(M)::value;
        const auto kernel = fcode_wide_kernel<decltype(A)::value, METHOD, REC>;
        static std::atomic<uint64_t> attr_done;
        if (!agp_lds_attr((const void*)kernel, wide_lds_bytes(METHOD), attr_done)) return AGP_E_LAUNCH;
        AGP_LAUNCH(kernel, grid, blk, wide_lds_bytes(METHOD), (hipStream_t)stream, x, add1, add2, (const bf16x8*)wf_hi,
                   (const bf16x8*)wf_lo, bias, b, st, nsteps, y, traj);
        AGP_CHECK_LAUNCH();
        return AGP_OK;
    });
}

extern "C" int agp_fcode_wide_fwd(const float* x, const float* add1, const float* add2, const void* wf_hi, const void* wf_lo,
                                  const float* bias, int b, int d, int act, int method, const float* dt, int nsteps, float* y,
                                  void* stream) {
    return wide_fwd<false>(x, add1, add2, wf_hi, wf_lo, bias, b, d, act, method, dt, nsteps, y, nullptr, stream);
}

extern "C" int64_t agp_fcode_wide_traj_floats(int b, int d, int method, int nsteps) {
    return wide_sizes_ok(b, d, method, nsteps) ? (int64_t)nsteps * (1 + stages_of(method)) * b * WD : 0;
}

extern "C" int agp_fcode_wide_fwd_traj(const float* x, const float* add1, const float* add2, const void* wf_hi, const void* wf_lo,
                                       const float* bias, int b, int d, int act, int method, const float* dt, int nsteps, float* y,
                                       float* traj, void* stream) {
    return wide_fwd<true>(x, add1, add2, wf_hi, wf_lo, bias, b, d, act, method, dt, nsteps, y, traj, stream);
}

extern "C" int64_t agp_fcode_wide_bwd_workspace_bytes(int b, int d, int method, int nsteps) {
    if (!wide_sizes_ok(b, d, method, nsteps)) return 0;
    const int64_t Bp = (b + FROWS - 1) / FROWS * FROWS;
    return 2 * (int64_t)nsteps * stages_of(method) * Bp * WD * sizeof(float);
}

extern "C" int agp_fcode_wide_bwd(const float* traj, const float* gy, const void* wtf_hi, const void* wtf_lo, int b, int d, int act,
                                  int method, const float* dt, int nsteps, float* gx, float* gw, float* gb, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    if (!traj || !gy || !wtf_hi || !wtf_lo || !dt || !gx || !workspace || b <= 0 || d <= 0 || nsteps <= 0 || nsteps > 64)
        return AGP_E_BADARG;
    if (method < AGP_ODE_EULER || method > AGP_ODE_RK4 || act < AGP_ACT_ID || act > AGP_ACT_SIGMOID) return AGP_E_BADARG;
    if (d != WD) return AGP_E_UNSUPPORTED;
    if (workspace_bytes < agp_fcode_wide_bwd_workspace_bytes(b, d, method, nsteps)) return AGP_E_BADARG;
    const int Bp = (b + FROWS - 1) / FROWS * FROWS;
    const int R = nsteps * stages_of(method) * Bp;
    float* GZ = (float*)workspace;
    float* S = GZ + (size_t)R * WD;
    OdeSteps st;
    for (int i = 0; i < 64; ++i) st.dt[i] = i < nsteps ? dt[i] : 0.f;
    hipStream_t s = (hipStream_t)stream;
    const int rc = by_act_method(act, method, [&](auto A, auto M) -> int {
        constexpr int METHOD = decltype(M)::value;
        const auto kernel = fcode_wide_bwd_kernel<decltype(A)::value, METHOD>;
        static std::atomic<uint64_t> attr_done;
        if (!agp_lds_attr((const void*)kernel, wide_bwd_lds_bytes(METHOD), attr_done)) return AGP_E_LAUNCH;
        AGP_LAUNCH(kernel, dim3(Bp / FROWS), dim3(WT), wide_bwd_lds_bytes(METHOD), s, traj, gy, (const bf16x8*)wtf_hi,
                   (const bf16x8*)wtf_lo, b, st, nsteps, gx, GZ, S, Bp);
        AGP_CHECK_LAUNCH();
        return AGP_OK;
    });
    if (rc != AGP_OK) return rc;
    if (gw) {      // dW[n][k] = sum_r gz[r][n] s[r][k]
        const int rg = gemm_tn(GZ, S, gw, WD, WD, R, WD, WD, WD, s);
        if (rg != AGP_OK) return rg;
    }
    return gb ? colsum(GZ, R, WD, WD, gb, s) : AGP_OK;
}
