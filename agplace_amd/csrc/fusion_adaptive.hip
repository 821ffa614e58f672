// Adaptive Dormand-Prince 5(4) solver ('dopri5') for the Neural-ODE blocks FCODE(256) and FCODE(384), forward and backward
// (the 384-column kernels, which cannot keep W in registers, follow the 256-column ones below).
// The algorithm is stated in DESIGN.md section 2 ("Adaptive solver") and restated in fp64 by tests/dopri5_ref.py.
//
// Forward: ONE launch of ONE persistent workgroup (16 waves) per solve.  torchdiffeq's step control couples the whole
// batch (one error norm over all b*256 elements), so a workgroup per 16 rows would have to wait for the others at
// every attempted step; a single workgroup needs nothing but its own barriers.  W's split-bf16 MFMA fragments stay in
// registers as in fcode_kernel (fusion.hip; the state has a third plane here, see store_state3); the workgroup walks the ceil(b/16) row tiles for every stage.  y and the
// seven stage derivatives live in a caller-supplied ring in global memory (L2-resident); a lane only ever re-reads the
// addresses it wrote itself (same row, same four features), so the ring needs no fence.  Ring entry n holds
// [y, k1 .. k7] of the attempt that starts from accepted step n; stage 7 writes y1 and k7 also to entry n + 1 as its
// (y, k1) -- FSAL -- so accepting a step is `++n` and rejecting it leaves entry n as it was.  With a trajectory the
// ring has max_steps + 1 entries and IS the record the backward reads; without one it has two.
// Time, step size, norms, the error ratio and the step factor are fp64.  Norms are reduced in a fixed order (a lane over
// its tiles in index order, butterfly over the wave, the 16 waves in wave order): two runs give the same bits.
//
// Backward: rows are independent once the step sizes are fixed: one workgroup per 16 rows like
// fcode_bwd_state_kernel (fusion_bwd.hip), step count and step sizes read from the control block in DEVICE memory.
#include <cstddef>
#include <type_traits>
#include "fusion_common.hpp"

namespace agp_fusion {

// Dormand-Prince 5(4).  Row 6 of DP_A is the solution weights (FSAL: stage 7's input is y1).
__device__ const double DP_A[7][6] = {
    {0., 0., 0., 0., 0., 0.},
    {1. / 5, 0., 0., 0., 0., 0.},
    {3. / 40, 9. / 40, 0., 0., 0., 0.},
    {44. / 45, -56. / 15, 32. / 9, 0., 0., 0.},
    {19372. / 6561, -25360. / 2187, 64448. / 6561, -212. / 729, 0., 0.},
    {9017. / 3168, -355. / 33, 46732. / 5247, 49. / 176, -5103. / 18656, 0.},
    {35. / 384, 0., 500. / 1113, 125. / 192, -2187. / 6784, 11. / 84}};
__device__ const double DP_CS[7] = {35. / 384, 0., 500. / 1113, 125. / 192, -2187. / 6784, 11. / 84, 0.};
__device__ const double DP_CE[7] = {35. / 384 - 1951. / 21600, 0., 500. / 1113 - 22642. / 50085, 125. / 192 - 451. / 720,
                                    -2187. / 6784 + 12231. / 42400, 11. / 84 - 649. / 6300, -1. / 60};
__device__ const double DP_MID[7] = {0.5 * 6025192743. / 30085553152., 0., 0.5 * 51252292925. / 65400821598.,
                                     0.5 * -2691868925. / 45128329728., 0.5 * 187940372067. / 1594534317056.,
                                     0.5 * -1776094331. / 19743644256., 0.5 * 11237099. / 235043384.};

// out = y + dt sum_j beta_j(x) k_j is the quartic interpolant of a step at x in [0, 1]; beta(1) = DP_CS
__device__ __forceinline__ double dp_beta(int j, double x) {
    const double d1 = j == 0 ? 1. : 0., d7 = j == 6 ? 1. : 0.;
    const double c4 = 16. * DP_MID[j] - 8. * DP_CS[j] + 2. * (d7 - d1);
    const double c3 = 14. * DP_CS[j] - 32. * DP_MID[j] + 5. * d1 - 3. * d7;
    const double c2 = 16. * DP_MID[j] - 5. * DP_CS[j] + d7 - 4. * d1;
    return (((c4 * x + c3) * x + c2) * x + d1) * x;
}

// control block: agp_ode_stats (include/agplace_hip.h), the max_steps step sizes of the accepted steps, then (dt, ratio) of
// every attempted step
struct OdeCtrl {
    int status, accepted, rejected, f_evals;
    double t0, t1;
    double dt[1];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // a + b == b + a: every lane ends with the same bits
    return v;
}

// a value every lane holds, moved to scalar registers (the stage coefficients: W's fragments leave few vector registers)
__device__ __forceinline__ float uniform_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double uniform_d(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// r^(-1/5) for finite r > 0, to fp64 accuracy: r = a 32^q with a in [1/2, 16), a single-precision power of a, two Newton
// steps z <- z (6 - a z^5) / 5 (quadratic: 1e-7 -> 1e-14 -> rounding).  A double-precision pow() next to W's 64 resident
// registers spills; this does not.
__device__ __forceinline__ double inv_fifth_root(double r) {
    int e;
    const double m = frexp(r, &e);
    const int q = e >= 0 ? e / 5 : -((4 - e) / 5);
    const double a = ldexp(m, e - 5 * q);
    double z = (double)powf((float)a, -0.2f);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double z2 = z * z;
        z = z * (6. - a * (z2 * z2 * z)) * 0.2;
    }
    return ldexp(z, -q);
}

constexpr int AD = 256, AKS = AD / 32, AYRB = AD * 2 + 16;

// f for the adaptive solver: the STATE as three bf16 planes (hi + mid + lo = 24 bits), five products
// W_hi (y_hi + y_mid + y_lo) + W_lo (y_hi + y_mid).  The fixed-grid kernels' two-plane state carries 2^-17 of rounding per
// element and stage, fresh at every stage; W k turns it into 1e-5 of noise on each k_i, and the error estimate
// dt sum CE_j k_j is a cancelling sum of them: at a ratio of 0.1 and tol = 1e-4 it was mostly that noise (step sizes 40 %
// off the fp64 restatement's on the device).  W keeps its two resident planes: their rounding is the same at every
// stage, i.e. a slightly different but smooth right-hand side, which the estimate is indifferent to.
__device__ __forceinline__ void store_state3(char* yhi, char* ymid, char* ylo, int yrb, int lane, int wave, const f32x4& v) {
    const int off = (lane & 15) * yrb + (wave * 16 + (lane >> 4) * 4) * 2;
    bf16_t h[4], m[4], l[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h[r] = f2bf(v[r]);
        const float r1 = v[r] - bf2f(h[r]);
        m[r] = f2bf(r1);
        l[r] = f2bf(r1 - bf2f(m[r]));
    }
    *(u32x2*)(yhi + off) = u32x2{pack2(h[0], h[1]), pack2(h[2], h[3])};
    *(u32x2*)(ymid + off) = u32x2{pack2(m[0], m[1]), pack2(m[2], m[3])};
    *(u32x2*)(ylo + off) = u32x2{pack2(l[0], l[1]), pack2(l[2], l[3])};
}
template <int KS>
__device__ __forceinline__ f32x4 mfma_resident5(const bf16x8 (&wh)[KS], const bf16x8 (&wl)[KS], const char* yhi,
                                                const char* ymid, const char* ylo, int yrb, int lane) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;     // three chains: the small products, the middle ones, hi.hi
    const int boff = (lane & 15) * yrb + (lane >> 4) * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 bh = *(const bf16x8*)(yhi + boff + ks * 64);
        const bf16x8 bm = *(const bf16x8*)(ymid + boff + ks * 64);
        const bf16x8 bl = *(const bf16x8*)(ylo + boff + ks * 64);
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks], bl, a0, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks], bm, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks], bh, a1, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks], bm, a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks], bh, a2, 0, 0, 0);
    }
    return (a0 + a1) + a2;
}

// per-attempt constants, written by thread 0 and read by every wave into scalar registers: the products of dt with the
// tableau.  (Computed by every lane they are hoisted out of the step loop as 50 fp64 values and spilled.)
struct StepCoef {
    double dt;
    double ce[7];      // dt * CE
    float a[5][5];     // dt * A rows 1 .. 5
    float cs[6];       // dt * CS
};
__device__ __forceinline__ void publish_step(StepCoef& c, double dt) {
    c.dt = dt;
#pragma unroll
    for (int j = 0; j < 7; ++j) c.ce[j] = dt * DP_CE[j];
#pragma unroll
    for (int i = 1; i <= 5; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) c.a[i - 1][j] = (float)(dt * DP_A[i][j]);
#pragma unroll
    for (int j = 0; j < 6; ++j) c.cs[j] = (float)(dt * DP_A[6][j]);
}

template <int ACT>
__global__ __launch_bounds__(FT) void fcode_adaptive_kernel(const float* __restrict__ x, const float* __restrict__ add1,
                                                            const float* __restrict__ add2,
                                                            const bf16_t* __restrict__ w_hi,
                                                            const bf16_t* __restrict__ w_lo,
                                                            const float* __restrict__ bias, int b, double rtol,
                                                            double atol, int max_steps, float* ring, int nring,
                                                            float* __restrict__ yout, OdeCtrl* __restrict__ ctrl) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 3 * FROWS * AYRB];   // [buf][plane]
    __shared__ double red[2][16];
    __shared__ StepCoef coef;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nf = wave * 16 + (lane >> 4) * 4;
    const int nt = (b + FROWS - 1) / FROWS;
    const double count = (double)b * AD;
    const float rtolf = (float)rtol, atolf = (float)atol;

    bf16x8 wh[AKS], wl[AKS];
    {
        const size_t wo = (size_t)(wave * 16 + (lane & 15)) * AD + (lane >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < AKS; ++ks) {
            wh[ks] = *(const bf16x8*)(w_hi + wo + ks * 32);
            wl[ks] = *(const bf16x8*)(w_lo + wo + ks * 32);
        }
    }
    f32x4 bia;
#pragma unroll
    for (int r = 0; r < 4; ++r) bia[r] = bias ? bias[nf + r] : 0.f;

    int buf = 0;
    auto feval = [&](const f32x4& state) -> f32x4 {
        char* hi = smem + buf * (3 * FROWS * AYRB);
        char* mid = hi + FROWS * AYRB;
        char* lo = mid + FROWS * AYRB;
        store_state3(hi, mid, lo, AYRB, lane, wave, state);
        __syncthreads();
        f32x4 z = mfma_resident5<AKS>(wh, wl, hi, mid, lo, AYRB, lane);
        buf ^= 1;
        return act4<ACT>(z + bia);
    };
    // ring[entry][sub][row][256]: sub 0 = y, 1 + j = k_{j+1}.  A uniform base plus this lane's 32-bit offset.
    const size_t plane = (size_t)b * AD;
    const int loff = (lane & 15) * AD + nf;
    auto at = [&](int entry, int sub, int T) -> float* {
        return ring + ((size_t)(entry * 8 + sub) * plane + (size_t)T * (FROWS * AD)) + loff;
    };
    // sums of two per-thread values over the workgroup, the same bits in every thread
    auto block_sum2 = [&](double& u, double& v) {
        u = wave_sum_f64(u);
        v = wave_sum_f64(v);
        __syncthreads();                      // the previous sums have been read
        if (lane == 0) { red[0][wave] = u; red[1][wave] = v; }
        __syncthreads();
        u = 0.; v = 0.;
        for (int w = 0; w < 16; ++w) { u += red[0][w]; v += red[1][w]; }
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- first step size (torchdiffeq _select_initial_step, order 4 -> exponent 1/5)
    double sq0 = 0., sq1 = 0.;
    for (int T = 0; T < nt; ++T) {
        const bool live = T * FROWS + (lane & 15) < b;
        f32x4 yv = zero4;
        if (live) {
            const size_t g = (size_t)T * (FROWS * AD) + loff;
            yv = *(const f32x4*)(x + g);
            if (add1) yv += *(const f32x4*)(add1 + g);
            if (add2) yv += *(const f32x4*)(add2 + g);
        }
        const f32x4 f0 = feval(yv);
        if (live) {
            *(f32x4*)at(0, 0, T) = yv;
            *(f32x4*)at(0, 1, T) = f0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sc = atolf + fabsf(yv[r]) * rtolf;
                const double a = (double)(yv[r] / sc), c = (double)(f0[r] / sc);
                sq0 += a * a; sq1 += c * c;
            }
        }
    }
    block_sum2(sq0, sq1);
    const double d0 = sqrt(sq0 / count), d1 = sqrt(sq1 / count);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    double sq2 = 0., unused = 0.;
    {
        const float h0f = uniform_f((float)h0);
        for (int T = 0; T < nt; ++T) {
            const bool live = T * FROWS + (lane & 15) < b;
            f32x4 yv = zero4, f0 = zero4;
            if (live) { yv = *(const f32x4*)at(0, 0, T); f0 = *(const f32x4*)at(0, 1, T); }
            const f32x4 f1 = feval(yv + h0f * f0);
            if (live) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sc = atolf + fabsf(yv[r]) * rtolf;
                    const double a = (double)((f1[r] - f0[r]) / sc);
                    sq2 += a * a;
                }
            }
        }
    }
    block_sum2(sq2, unused);
    if (tid == 0) {
        const double d2 = sqrt(sq2 / count) / h0;
        const double dm = fmax(d1, d2);
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : (dm < 1e298 ? inv_fifth_root(dm * 100.) : 0.);
        publish_step(coef, fmin(100. * h0, h1));
    }
    __syncthreads();

    // stage I (0-based, 1 .. 5): k_{I+1} = f(y + dt sum_{j < I} A[I][j] k_{j+1})
    auto stage = [&](auto Ic, int cur) {
        constexpr int I = decltype(Ic)::value;
        float cf[I];
#pragma unroll
        for (int j = 0; j < I; ++j) cf[j] = uniform_f(coef.a[I - 1][j]);
        for (int T = 0; T < nt; ++T) {
            const bool live = T * FROWS + (lane & 15) < b;
            f32x4 s = zero4;
            if (live) {
                f32x4 kk[I];
                s = *(const f32x4*)at(cur, 0, T);
#pragma unroll
                for (int j = 0; j < I; ++j) kk[j] = *(const f32x4*)at(cur, 1 + j, T);
#pragma unroll
                for (int j = 0; j < I; ++j) s += cf[j] * kk[j];
            }
            const f32x4 k = feval(s);
            if (live) *(f32x4*)at(cur, 1 + I, T) = k;
        }
    };

    double t = 0., t_end = 0.;
    int status = 0, attempts = 0, acc = 0, rej = 0, nfe = 2;
    for (;;) {
        const double dt = uniform_d(coef.dt);
        if (attempts >= max_steps) { status = AGP_ODE_E_MAXSTEPS; break; }
        if (t + dt == t) { status = AGP_ODE_E_UNDERFLOW; break; }
        ++attempts;
        const int cur = __builtin_amdgcn_readfirstlane(acc % nring), nxt = __builtin_amdgcn_readfirstlane((acc + 1) % nring);
        stage(std::integral_constant<int, 1>{}, cur);
        stage(std::integral_constant<int, 2>{}, cur);
        stage(std::integral_constant<int, 3>{}, cur);
        stage(std::integral_constant<int, 4>{}, cur);
        stage(std::integral_constant<int, 5>{}, cur);
        // stage 7: y1, k7 = f(y1) and the error ratio
        double sq = 0., sqx = 0.;
        {
            float cs[6];
            double ce[7];
#pragma unroll
            for (int j = 0; j < 6; ++j) cs[j] = uniform_f(coef.cs[j]);
#pragma unroll
            for (int j = 0; j < 7; ++j) ce[j] = uniform_d(coef.ce[j]);
            for (int T = 0; T < nt; ++T) {
                const bool live = T * FROWS + (lane & 15) < b;
                f32x4 yv = zero4, y1 = zero4;
                double e[4] = {0., 0., 0., 0.};
                if (live) {
                    yv = *(const f32x4*)at(cur, 0, T);
                    f32x4 kk[6];
#pragma unroll
                    for (int j = 0; j < 6; ++j) kk[j] = *(const f32x4*)at(cur, 1 + j, T);
                    y1 = yv;
#pragma unroll
                    for (int j = 0; j < 6; ++j) y1 += cs[j] * kk[j];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int j = 0; j < 6; ++j) e[r] += ce[j] * (double)kk[j][r];
                }
                const f32x4 k7 = feval(y1);
                if (live) {
                    *(f32x4*)at(cur, 7, T) = k7;
                    *(f32x4*)at(nxt, 0, T) = y1;
                    *(f32x4*)at(nxt, 1, T) = k7;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // the cancelling sum in fp64, the quotient in fp32 (1e-7 relative: nothing next to the k's own rounding)
                        const float ef = (float)(e[r] + ce[6] * (double)k7[r]);
                        const double q = (double)(ef / (atolf + rtolf * fmaxf(fabsf(yv[r]), fabsf(y1[r]))));
                        sq += q * q;
                    }
                }
            }
        }
        nfe += 6;
        block_sum2(sq, sqx);
        const double ratio = sqrt(sq / count);
        if (tid == 0) {
            double* att = ctrl->dt + max_steps + 2 * (attempts - 1);
            att[0] = dt;
            att[1] = ratio;
        }
        if (!(ratio == ratio)) { status = AGP_ODE_E_NAN; break; }
        const bool accept = __builtin_amdgcn_readfirstlane(ratio <= 1. ? 1 : 0) != 0;
        if (accept) {
            if (tid == 0) ctrl->dt[acc] = dt;
            const double t1 = t + dt;
            ++acc;
            if (t1 >= 1.) {     // the quartic interpolant of this step at time 1
                const double xs = (1. - t) / (t1 - t);
                float be[7];
#pragma unroll
                for (int j = 0; j < 7; ++j) be[j] = uniform_f((float)(dt * dp_beta(j, xs)));
                for (int T = 0; T < nt; ++T) {
                    if (T * FROWS + (lane & 15) < b) {
                        f32x4 o = *(const f32x4*)at(cur, 0, T);
                        f32x4 kk[7];
#pragma unroll
                        for (int j = 0; j < 7; ++j) kk[j] = *(const f32x4*)at(cur, 1 + j, T);
#pragma unroll
                        for (int j = 0; j < 7; ++j) o += be[j] * kk[j];
                        *(f32x4*)(yout + (size_t)T * (FROWS * AD) + loff) = o;
                    }
                }
                t_end = t1;
                break;
            }
            t = t1;
        } else {
            ++rej;
        }
        // every wave has read this attempt's constants (the barriers of stage 7 lie behind their last read)
        if (tid == 0) {
            double fac = 10.;
            if (ratio != 0.) fac = fmin(10., fmax(ratio < 1e300 ? 0.9 * inv_fifth_root(ratio) : 0., ratio < 1. ? 1. : 0.2));
            publish_step(coef, dt * fac);
        }
        __syncthreads();
    }
    if (status != 0) {     // a failed solve must not pass for a result
        const float qnan = __builtin_nanf("");
        for (int T = 0; T < nt; ++T)
            if (T * FROWS + (lane & 15) < b) *(f32x4*)(yout + (size_t)T * (FROWS * AD) + loff) = f32x4{qnan, qnan, qnan, qnan};
        t_end = t;
    }
    // the unused tail of the control block is zero: two equal solves leave equal blocks
    for (int i = tid; i < 3 * max_steps; i += FT)
        if (i < max_steps ? i >= acc : i - max_steps >= 2 * attempts) ctrl->dt[i] = 0.;
    if (tid == 0) {
        ctrl->status = status;
        ctrl->accepted = acc;
        ctrl->rejected = rej;
        ctrl->f_evals = nfe;
        ctrl->t0 = t;
        ctrl->t1 = t_end;
    }
}

template <int ACT>
__device__ __forceinline__ f32x4 dact_out(const f32x4& k) {
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (ACT == AGP_ACT_RELU) o[r] = k[r] > 0.f ? 1.f : 0.f;
        else if (ACT == AGP_ACT_TANH) o[r] = 1.f - k[r] * k[r];
        else if (ACT == AGP_ACT_SIGMOID) o[r] = k[r] * (1.f - k[r]);
        else o[r] = 1.f;
    }
    return o;
}

// Discretise-then-optimise through the accepted steps.  Step n: s_1 = y, s_i = y + dt sum_{j<i} A_ij k_j, k_i = f(s_i)
// (i = 2 .. 7, A_7 = CS), out = y + dt sum_j w_j k_j with w = CS (out = s_7) or, for the last step, w = beta(x).
// k_1 of step n + 1 IS k_7 of step n (FSAL), so the adjoint of k_1 is carried into the step before (g7).  With a = dL/d out:
//     gk_j = dt w_j a (+ g7 for j = 7);  for i = 7 .. 2: gz_i = gk_i act'(k_i), gs_i = gz_i W, a += gs_i,
//     gk_j += dt A_ij gs_i (j < i);  g7 <- gk_1;  at step 0: gz_1 = gk_1 act'(k_1), a += gz_1 W.
// Every gz_i goes to the workspace, row block 6 n + (i - 2), the one of step 0's k_1 to block 6 N; the stage inputs s_i the
// weight gradient pairs them with are rebuilt by adaptive_stage_inputs_kernel (the recursion itself does not need them).
template <int ACT>
__global__ __launch_bounds__(FT) void fcode_adaptive_bwd_kernel(const float* __restrict__ traj,
                                                                const OdeCtrl* __restrict__ ctrl,
                                                                const float* __restrict__ gy,
                                                                const bf16_t* __restrict__ wt_hi,
                                                                const bf16_t* __restrict__ wt_lo, int b, int max_steps,
                                                                float* __restrict__ gx, float* __restrict__ GZ,
                                                                int Bp) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * FROWS * AYRB];
    __shared__ float bc[28];      // this step's dt A[i][j] at i (i - 1) / 2 + j (i = 1 .. 6, j < i), dt w_j at 21 + j
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int brow = blockIdx.x * FROWS + (lane & 15);
    const int nf = wave * 16 + (lane >> 4) * 4;
    const bool live = brow < b;
    const int status = __builtin_amdgcn_readfirstlane(ctrl->status);
    int N = __builtin_amdgcn_readfirstlane(ctrl->accepted);
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (status != 0) {      // the forward returned NaN: so does the backward (row block 0 is the only one the sums read)
        const float qnan = __builtin_nanf("");
        const f32x4 n4 = {qnan, qnan, qnan, qnan};
        *(f32x4*)(GZ + (size_t)brow * AD + nf) = live ? n4 : zero4;
        if (live) *(f32x4*)(gx + (size_t)brow * AD + nf) = n4;
        return;
    }

    bf16x8 wh[AKS], wl[AKS];
    {
        const size_t wo = (size_t)(wave * 16 + (lane & 15)) * AD + (lane >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < AKS; ++ks) {
            wh[ks] = *(const bf16x8*)(wt_hi + wo + ks * 32);
            wl[ks] = *(const bf16x8*)(wt_lo + wo + ks * 32);
        }
    }
    int buf = 0;
    auto times_w = [&](const f32x4& gz) -> f32x4 {
        char* hi = smem + buf * (2 * FROWS * AYRB);
        char* lo = hi + FROWS * AYRB;
        store_state(hi, lo, AYRB, lane, wave, gz);
        __syncthreads();
        const f32x4 r = mfma_resident<AKS>(wh, wl, hi, lo, AYRB, lane);
        buf ^= 1;
        return r;
    };
    auto ld = [&](int n, int sub) -> f32x4 {
        if (!live) return zero4;
        return *(const f32x4*)(traj + (((size_t)n * 8 + sub) * b + brow) * AD + nf);
    };
    auto emit = [&](int blk, const f32x4& gz) { *(f32x4*)(GZ + ((size_t)blk * Bp + brow) * AD + nf) = gz; };

    f32x4 a = live ? *(const f32x4*)(gy + (size_t)brow * AD + nf) : zero4;
    f32x4 g7 = zero4;
    const double t0 = ctrl->t0, t1 = ctrl->t1;
    const double xs = (1. - t0) / (t1 - t0);
    for (int n = N - 1; n >= 0; --n) {
        __syncthreads();          // the step before has read its constants
        if (tid < 28) {           // one constant per thread (computed by every lane they are hoisted as fp64 and spilled)
            const double dt = ctrl->dt[n];
            double c;
            if (tid < 21) {
                int i = 1;
                while ((i + 1) * i / 2 <= tid) ++i;
                c = DP_A[i][tid - i * (i - 1) / 2];
            } else {
                c = n == N - 1 ? dp_beta(tid - 21, xs) : DP_CS[tid - 21];
            }
            bc[tid] = (float)(dt * c);
        }
        __syncthreads();
        f32x4 gk[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) gk[j] = uniform_f(bc[21 + j]) * a;
        gk[6] += g7;
#pragma unroll
        for (int i = 6; i >= 1; --i) {
            const f32x4 gz = gk[i] * dact_out<ACT>(ld(n, 1 + i));
            emit(6 * n + (i - 1), gz);
            const f32x4 gs = times_w(gz);
            a += gs;
#pragma unroll
            for (int j = 0; j < i; ++j) gk[j] += uniform_f(bc[i * (i - 1) / 2 + j]) * gs;
        }
        g7 = gk[0];
        if (n == 0) {
            const f32x4 gz = g7 * dact_out<ACT>(ld(0, 1));
            emit(6 * N, gz);
            a += times_w(gz);
        }
    }
    if (N == 0) emit(0, zero4);
    if (live) *(f32x4*)(gx + (size_t)brow * AD + nf) = a;
}

// S[6 n + i - 1] = y_n + dt_n sum_{j < i} A[i][j] k_{j+1} (i = 1 .. 6: the inputs of stages 2 .. 7 of accepted step n),
// S[6 N] = y_0.  blockIdx.y = n; one thread per (row, four features); rows beyond b are zero like their gz.
// D = the width (256 or 384): the three kernels below are the same code at either, in the same fixed order.
template <int D>
__global__ __launch_bounds__(256) void adaptive_stage_inputs_kernel(const float* __restrict__ traj,
                                                                    const OdeCtrl* __restrict__ ctrl, int b, int max_steps,
                                                                    float* __restrict__ S, int Bp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;      // < Bp * D / 4
    const int brow = idx / (D / 4), nf = (idx % (D / 4)) * 4;
    const int n = blockIdx.y;
    const int status = ctrl->status;
    int N = status != 0 ? 0 : ctrl->accepted;
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const bool live = brow < b;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    auto ld = [&](int sub) -> f32x4 {
        return live ? *(const f32x4*)(traj + (((size_t)n * 8 + sub) * b + brow) * D + nf) : zero4;
    };
    auto st = [&](int blk, const f32x4& v) { *(f32x4*)(S + ((size_t)blk * Bp + brow) * D + nf) = v; };
    if (n == 0) {
        const float qnan = __builtin_nanf("");
        st(6 * N, status != 0 && live ? f32x4{qnan, qnan, qnan, qnan} : ld(0));
    }
    if (n >= N) return;
    const double dt = ctrl->dt[n];
    const f32x4 y = ld(0);
    f32x4 k[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) k[j] = ld(1 + j);
#pragma unroll
    for (int i = 1; i <= 6; ++i) {
        f32x4 s = y;
#pragma unroll
        for (int j = 0; j < i; ++j) s += (float)(dt * DP_A[i][j]) * k[j];
        st(6 * n + i - 1, s);
    }
}

// C[D][D] = sum_r A[r][m] * B[r][n] over the R = (6 N + 1) Bp rows the state kernel wrote, N read from the control
// block (gemm_tn_f32_kernel of fusion_bwd.hip with a device-side row count; same tile shape, same fixed order).
template <int D>
__global__ __launch_bounds__(256) void adaptive_gw_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          float* __restrict__ C, const OdeCtrl* __restrict__ ctrl,
                                                          int max_steps, int Bp) {
    __shared__ float as[16][64 + 4], bs[16][64 + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    int N = ctrl->status != 0 ? 0 : ctrl->accepted;
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const int R = (6 * N + 1) * Bp;      // a multiple of 16
    float acc[4][4] = {};
    for (int r0 = 0; r0 < R; r0 += 16) {
        for (int i = tid; i < 16 * 64; i += 256) {
            const int rr = i >> 6, cc = i & 63;
            as[rr][cc] = A[(size_t)(r0 + rr) * D + m0 + cc];
            bs[rr][cc] = B[(size_t)(r0 + rr) * D + n0 + cc];
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = as[rr][ty * 4 + i]; bv[i] = bs[rr][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[i][jj] += av[i] * bv[jj];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) C[(size_t)(m0 + ty * 4 + i) * D + n0 + tx * 4 + jj] = acc[i][jj];
}

// gb[c] = sum_r GZ[r][c]: wave w adds the rows w, w + 4, ..., the four wave sums are added in wave order
template <int D>
__global__ __launch_bounds__(256) void adaptive_gb_kernel(const float* __restrict__ A, float* __restrict__ out,
                                                          const OdeCtrl* __restrict__ ctrl, int max_steps, int Bp) {
    __shared__ float redf[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    int N = ctrl->status != 0 ? 0 : ctrl->accepted;
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const int R = (6 * N + 1) * Bp;
    float s = 0.f;
    for (int r = w; r < R; r += 4) s += A[(size_t)r * D + c];
    redf[w][lane] = s;
    __syncthreads();
    if (w == 0) out[c] = ((redf[0][lane] + redf[1][lane]) + redf[2][lane]) + redf[3][lane];
}

// ---------------------------------------------------------------------------------------------------------------------
// The same solver at 384 columns (agp_fcode_adaptive_wide_fwd / _bwd).  Both split-bf16 planes of a 384 x 384 W are 576 KiB,
// more than a CU's register file, so the work shape is fcode_wide_kernel's (fusion_wide.hip): ONE workgroup of 8 waves, wave w
// owns the three 16-feature tiles [48 w, 48 w + 48) over the full K; the 36 `hi` fragments stay in registers (144), the `lo`
// fragments of the same (tile, K-step) pairs are streamed from L2 through a ring of XRING K-steps, in the fragment order of
// ops.fcode_wide_planes; no K split, hence no cross-wave sum and ONE barrier per evaluation and row tile.  Everything else is
// fcode_adaptive_kernel: the row-tile walk, the three-plane state and the five products, the FSAL ring in global memory (a
// lane re-reads only what it wrote: row l & 15 of a tile, features 48 w + 16 t + 4 (l >> 4) + r), the norms reduced in a fixed
// order (a lane over its row tiles, feature tiles and elements in index order, butterfly over the wave, the 8 waves in wave
// order), fp64 step control by thread 0.  A lane owns twelve features of a row here, not four: the stage combinations run one
// feature tile at a time, and stage 7 forms its error sum AFTER the evaluation from the ring (y1 is already in entry n + 1),
// so nothing state-sized waits in registers across an evaluation.
constexpr int XD = 384, XT = 512, XKS = XD / 32, XTILES = 3, XRING = 3, XYRB = XD * 2 + 16, XWAVES = XT / 64;
constexpr int XPLANES_FWD = 2 * 3 * FROWS * XYRB;      // 75264 B: [buf][plane hi, mid, lo]; more than 64 KB (agp_lds_attr)
constexpr int XPLANES_BWD = 2 * 2 * FROWS * XYRB;      // 50176 B: [buf][plane hi, lo]
constexpr int XLDS_FWD = XPLANES_FWD + XD * 4;         // + the bias

struct Tiles3 {
    f32x4 t[XTILES];
};

// acc[t] = sum_k W[48 w + 16 t + ..][k] * state[row][k] on the planes in LDS: NP = 3 the forward's five products
// W_hi (y_hi + y_mid + y_lo) + W_lo (y_hi + y_mid), NP = 2 the backward's three, W_hi (g_hi + g_lo) + W_lo g_hi.  One chain
// per tile as in fcode_wide_kernel (a second one costs scratch), the tiles interleaved, K-steps ascending -- a fixed order.
// (The pointer is made opaque once per evaluation, in ring_prime, and once per K-step: W is loop-invariant, and a compiler
// that knows it hoists all 36 `lo` fragments out of the step loop.)
template <int NP>
__device__ __forceinline__ Tiles3 mfma_streamed(const bf16x8 (&wh)[XKS][XTILES], const bf16x8* fl, const char* planes,
                                                bf16x8 (&ring)[XRING][XTILES], int boff) {
    const bf16x8* fp = fl;
    const char* hi = planes;
    const char* mid = planes + FROWS * XYRB;
    const char* lo = planes + (NP - 1) * FROWS * XYRB;
    f32x4 as[XTILES];
#pragma unroll
    for (int t = 0; t < XTILES; ++t) as[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks) {
        const bf16x8 bh = *(const bf16x8*)(hi + boff + ks * 64);
        const bf16x8 bl = *(const bf16x8*)(lo + boff + ks * 64);
#pragma unroll
        for (int t = 0; t < XTILES; ++t) as[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][t], bl, as[t], 0, 0, 0);
        if constexpr (NP == 3) {
            const bf16x8 bm = *(const bf16x8*)(mid + boff + ks * 64);
#pragma unroll
            for (int t = 0; t < XTILES; ++t) as[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][t], bm, as[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < XTILES; ++t) as[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][t], bh, as[t], 0, 0, 0);
            // (the streamed plane last: its loads have nine more MFMAs to arrive)
#pragma unroll
            for (int t = 0; t < XTILES; ++t) as[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[ks % XRING][t], bm, as[t], 0, 0, 0);
        } else {
#pragma unroll
            for (int t = 0; t < XTILES; ++t) as[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks][t], bh, as[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < XTILES; ++t) as[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[ks % XRING][t], bh, as[t], 0, 0, 0);
        if (ks + XRING < XKS) {
            asm volatile("" : "+v"(fp));
#pragma unroll
            for (int t = 0; t < XTILES; ++t) ring[ks % XRING][t] = fp[((ks + XRING) * XTILES + t) * 64];
        }
    }
    Tiles3 o;
#pragma unroll
    for (int t = 0; t < XTILES; ++t) o.t[t] = as[t];
    return o;
}
// the first XRING K-steps of an evaluation's `lo` fragments: issued BEFORE the barrier that publishes the new state
__device__ __forceinline__ void ring_prime(const bf16x8* fl, bf16x8 (&ring)[XRING][XTILES]) {
    const bf16x8* fp = fl;
    asm volatile("" : "+v"(fp));
#pragma unroll
    for (int c = 0; c < XRING; ++c)
#pragma unroll
        for (int t = 0; t < XTILES; ++t) ring[c][t] = fp[(c * XTILES + t) * 64];
}

template <int ACT>
__global__ __launch_bounds__(XT) void fcode_adaptive_wide_kernel(const float* __restrict__ x, const float* __restrict__ add1,
                                                                 const float* __restrict__ add2,
                                                                 const bf16x8* __restrict__ wf_hi,
                                                                 const bf16x8* __restrict__ wf_lo,
                                                                 const float* __restrict__ bias, int b, double rtol,
                                                                 double atol, int max_steps, float* ring, int nring,
                                                                 float* __restrict__ yout, OdeCtrl* __restrict__ ctrl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // XLDS_FWD: the state planes [buf][plane], the bias
    __shared__ double red[2][XWAVES];
    __shared__ StepCoef coef;
    __shared__ float sbeta[7];
    float* const sbias = (float*)(smem + XPLANES_FWD);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nf = wave * (16 * XTILES) + (lane >> 4) * 4;      // this lane's first feature of tile 0
    const int nt = (b + FROWS - 1) / FROWS;
    const double count = (double)b * XD;
    const float rtolf = (float)rtol, atolf = (float)atol;

    const bf16x8* fh = wf_hi + (size_t)wave * (XKS * XTILES * 64) + lane;
    const bf16x8* fl = wf_lo + (size_t)wave * (XKS * XTILES * 64) + lane;
    bf16x8 wh[XKS][XTILES];
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks)
#pragma unroll
        for (int t = 0; t < XTILES; ++t) wh[ks][t] = fh[(ks * XTILES + t) * 64];
    if (tid < XD) sbias[tid] = bias ? bias[tid] : 0.f;     // (published by the first evaluation's barrier)

    int buf = 0;
    const int soff = (lane & 15) * XYRB + nf * 2;                 // where this lane's 4 features of tile 0 go in a plane
    const int boff = (lane & 15) * XYRB + (lane >> 4) * 16;       // this lane's B fragment of K-step 0
    // one feature tile of the state an evaluation is about to read, as three bf16 planes
    auto put = [&](int t, const f32x4& v) {
        char* hi = smem + buf * (3 * FROWS * XYRB) + soff + 32 * t;
        bf16_t h[4], m[4], l[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            h[r] = f2bf(v[r]);
            const float r1 = v[r] - bf2f(h[r]);
            m[r] = f2bf(r1);
            l[r] = f2bf(r1 - bf2f(m[r]));
        }
        *(u32x2*)hi = u32x2{pack2(h[0], h[1]), pack2(h[2], h[3])};
        *(u32x2*)(hi + FROWS * XYRB) = u32x2{pack2(m[0], m[1]), pack2(m[2], m[3])};
        *(u32x2*)(hi + 2 * FROWS * XYRB) = u32x2{pack2(l[0], l[1]), pack2(l[2], l[3])};
    };
    // f of the state the three put()s wrote
    auto feval = [&]() -> Tiles3 {
        bf16x8 lring[XRING][XTILES];
        ring_prime(fl, lring);
        __syncthreads();
        Tiles3 z = mfma_streamed<3>(wh, fl, smem + buf * (3 * FROWS * XYRB), lring, boff);
        buf ^= 1;
#pragma unroll
        for (int t = 0; t < XTILES; ++t) {
            z.t[t] = act4<ACT>(z.t[t] + *(const f32x4*)(sbias + nf + 16 * t));
            __builtin_amdgcn_sched_barrier(0);      // one tile at a time (twelve interleaved sigmoid divisions cost scratch)
        }
        return z;
    };
    // ring[entry][sub][row][384]: sub 0 = y, 1 + j = k_{j+1}.  A uniform base plus this lane's 32-bit offset; tile t at + 16 t.
    const size_t plane = (size_t)b * XD;
    const int loff = (lane & 15) * XD + nf;
    auto at = [&](int entry, int sub, int T) -> float* {
        return ring + ((size_t)(entry * 8 + sub) * plane + (size_t)T * (FROWS * XD)) + loff;
    };
    auto block_sum2 = [&](double& u, double& v) {
        u = wave_sum_f64(u);
        v = wave_sum_f64(v);
        __syncthreads();                      // the previous sums have been read
        if (lane == 0) { red[0][wave] = u; red[1][wave] = v; }
        __syncthreads();
        u = 0.; v = 0.;
        for (int w = 0; w < XWAVES; ++w) { u += red[0][w]; v += red[1][w]; }
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- first step size (torchdiffeq _select_initial_step, order 4 -> exponent 1/5)
    double sq0 = 0., sq1 = 0.;
    for (int T = 0; T < nt; ++T) {
        const bool live = T * FROWS + (lane & 15) < b;
#pragma unroll
        for (int t = 0; t < XTILES; ++t) {
            f32x4 yv = zero4;
            if (live) {
                const size_t g = (size_t)T * (FROWS * XD) + loff + 16 * t;
                yv = *(const f32x4*)(x + g);
                if (add1) yv += *(const f32x4*)(add1 + g);
                if (add2) yv += *(const f32x4*)(add2 + g);
                *(f32x4*)(at(0, 0, T) + 16 * t) = yv;
            }
            put(t, yv);
            __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
        }
        const Tiles3 f0 = feval();
        if (live) {
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
                const f32x4 yv = *(const f32x4*)(at(0, 0, T) + 16 * t);
                *(f32x4*)(at(0, 1, T) + 16 * t) = f0.t[t];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sc = atolf + fabsf(yv[r]) * rtolf;
                    const double a = (double)(yv[r] / sc), c = (double)(f0.t[t][r] / sc);
                    sq0 += a * a; sq1 += c * c;
                }
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
        }
    }
    block_sum2(sq0, sq1);
    const double d0 = sqrt(sq0 / count), d1 = sqrt(sq1 / count);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    double sq2 = 0., unused = 0.;
    {
        const float h0f = uniform_f((float)h0);
        for (int T = 0; T < nt; ++T) {
            const bool live = T * FROWS + (lane & 15) < b;
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
                f32x4 s = zero4;
                if (live) s = *(const f32x4*)(at(0, 0, T) + 16 * t) + h0f * *(const f32x4*)(at(0, 1, T) + 16 * t);
                put(t, s);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles3 f1 = feval();
            if (live) {
#pragma unroll
                for (int t = 0; t < XTILES; ++t) {
                    const f32x4 yv = *(const f32x4*)(at(0, 0, T) + 16 * t), f0 = *(const f32x4*)(at(0, 1, T) + 16 * t);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sc = atolf + fabsf(yv[r]) * rtolf;
                        const double a = (double)((f1.t[t][r] - f0[r]) / sc);
                        sq2 += a * a;
                    }
                    __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
                }
            }
        }
    }
    block_sum2(sq2, unused);
    if (tid == 0) {
        const double d2 = sqrt(sq2 / count) / h0;
        const double dm = fmax(d1, d2);
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : (dm < 1e298 ? inv_fifth_root(dm * 100.) : 0.);
        publish_step(coef, fmin(100. * h0, h1));
    }
    __syncthreads();

    // stage I (0-based, 1 .. 5): k_{I+1} = f(y + dt sum_{j < I} A[I][j] k_{j+1})
    auto stage = [&](auto Ic, int cur) {
        constexpr int I = decltype(Ic)::value;
        float cf[I];
#pragma unroll
        for (int j = 0; j < I; ++j) cf[j] = uniform_f(coef.a[I - 1][j]);
        for (int T = 0; T < nt; ++T) {
            const bool live = T * FROWS + (lane & 15) < b;
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
                f32x4 s = zero4;
                if (live) {
                    f32x4 kk[I];
                    s = *(const f32x4*)(at(cur, 0, T) + 16 * t);
#pragma unroll
                    for (int j = 0; j < I; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * t);
#pragma unroll
                    for (int j = 0; j < I; ++j) s += cf[j] * kk[j];
                }
                put(t, s);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles3 k = feval();
            if (live) {
#pragma unroll
                for (int t = 0; t < XTILES; ++t) *(f32x4*)(at(cur, 1 + I, T) + 16 * t) = k.t[t];
            }
        }
    };

    double t = 0., t_end = 0.;
    int status = 0, attempts = 0, acc = 0, rej = 0, nfe = 2;
    for (;;) {
        const double dt = uniform_d(coef.dt);
        if (attempts >= max_steps) { status = AGP_ODE_E_MAXSTEPS; break; }
        if (t + dt == t) { status = AGP_ODE_E_UNDERFLOW; break; }
        ++attempts;
        const int cur = __builtin_amdgcn_readfirstlane(acc % nring), nxt = __builtin_amdgcn_readfirstlane((acc + 1) % nring);
        stage(std::integral_constant<int, 1>{}, cur);
        stage(std::integral_constant<int, 2>{}, cur);
        stage(std::integral_constant<int, 3>{}, cur);
        stage(std::integral_constant<int, 4>{}, cur);
        stage(std::integral_constant<int, 5>{}, cur);
        // stage 7: y1, k7 = f(y1) and the error ratio
        double sq = 0., sqx = 0.;
        {
            float cs[6];
            double ce[7];
#pragma unroll
            for (int j = 0; j < 6; ++j) cs[j] = uniform_f(coef.cs[j]);
#pragma unroll
            for (int j = 0; j < 7; ++j) ce[j] = uniform_d(coef.ce[j]);
            for (int T = 0; T < nt; ++T) {
                const bool live = T * FROWS + (lane & 15) < b;
#pragma unroll
                for (int t = 0; t < XTILES; ++t) {
                    f32x4 y1 = zero4;
                    if (live) {
                        f32x4 kk[6];
                        y1 = *(const f32x4*)(at(cur, 0, T) + 16 * t);
#pragma unroll
                        for (int j = 0; j < 6; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * t);
#pragma unroll
                        for (int j = 0; j < 6; ++j) y1 += cs[j] * kk[j];
                        *(f32x4*)(at(nxt, 0, T) + 16 * t) = y1;
                    }
                    put(t, y1);
                    __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
                }
                const Tiles3 k7 = feval();
                if (live) {
#pragma unroll
                    for (int t = 0; t < XTILES; ++t) {
                        *(f32x4*)(at(cur, 7, T) + 16 * t) = k7.t[t];
                        *(f32x4*)(at(nxt, 1, T) + 16 * t) = k7.t[t];
                        const f32x4 yv = *(const f32x4*)(at(cur, 0, T) + 16 * t), y1 = *(const f32x4*)(at(nxt, 0, T) + 16 * t);
                        f32x4 kk[6];
#pragma unroll
                        for (int j = 0; j < 6; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * t);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            // the cancelling sum in fp64, the quotient in fp32 (1e-7 relative: nothing next to the k's own rounding)
                            double e = 0.;
#pragma unroll
                            for (int j = 0; j < 6; ++j) e += ce[j] * (double)kk[j][r];
                            const float ef = (float)(e + ce[6] * (double)k7.t[t][r]);
                            const double q = (double)(ef / (atolf + rtolf * fmaxf(fabsf(yv[r]), fabsf(y1[r]))));
                            sq += q * q;
                        }
                        __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
                    }
                }
            }
        }
        nfe += 6;
        block_sum2(sq, sqx);
        const double ratio = sqrt(sq / count);
        if (tid == 0) {
            double* att = ctrl->dt + max_steps + 2 * (attempts - 1);
            att[0] = dt;
            att[1] = ratio;
        }
        if (!(ratio == ratio)) { status = AGP_ODE_E_NAN; break; }
        const bool accept = __builtin_amdgcn_readfirstlane(ratio <= 1. ? 1 : 0) != 0;
        if (accept) {
            if (tid == 0) ctrl->dt[acc] = dt;
            const double t1 = t + dt;
            ++acc;
            if (t1 >= 1.) { t_end = t1; break; }
            t = t1;
        } else {
            ++rej;
        }
        // every wave has read this attempt's constants (the barriers of stage 7 lie behind their last read)
        if (tid == 0) {
            double fac = 10.;
            if (ratio != 0.) fac = fmin(10., fmax(ratio < 1e300 ? 0.9 * inv_fifth_root(ratio) : 0., ratio < 1. ? 1. : 0.2));
            publish_step(coef, dt * fac);
        }
        __syncthreads();
    }
    if (status == 0) {     // the quartic interpolant of the last step at time 1, one weight per thread (behind the loop and not
                           // in every lane: the quartic's fp64 constants are otherwise hoisted out of the loop and spilled)
        const double dt = uniform_d(coef.dt);
        const int cur = __builtin_amdgcn_readfirstlane((acc - 1) % nring);
        const double xs = (1. - t) / (t_end - t);
        if (tid < 7) sbeta[tid] = (float)(dt * dp_beta(tid, xs));
        __syncthreads();
        float be[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) be[j] = uniform_f(sbeta[j]);
        for (int T = 0; T < nt; ++T) {
            if (T * FROWS + (lane & 15) < b) {
#pragma unroll
                for (int tt = 0; tt < XTILES; ++tt) {
                    f32x4 o = *(const f32x4*)(at(cur, 0, T) + 16 * tt);
                    f32x4 kk[7];
#pragma unroll
                    for (int j = 0; j < 7; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * tt);
#pragma unroll
                    for (int j = 0; j < 7; ++j) o += be[j] * kk[j];
                    *(f32x4*)(yout + (size_t)T * (FROWS * XD) + loff + 16 * tt) = o;
                    __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
                }
            }
        }
    }
    if (status != 0) {     // a failed solve must not pass for a result
        const float qnan = __builtin_nanf("");
        for (int T = 0; T < nt; ++T)
            if (T * FROWS + (lane & 15) < b) {
#pragma unroll
                for (int tt = 0; tt < XTILES; ++tt)
                    *(f32x4*)(yout + (size_t)T * (FROWS * XD) + loff + 16 * tt) = f32x4{qnan, qnan, qnan, qnan};
            }
        t_end = t;
    }
    // the unused tail of the control block is zero: two equal solves leave equal blocks
    for (int i = tid; i < 3 * max_steps; i += XT)
        if (i < max_steps ? i >= acc : i - max_steps >= 2 * attempts) ctrl->dt[i] = 0.;
    if (tid == 0) {
        ctrl->status = status;
        ctrl->accepted = acc;
        ctrl->rejected = rej;
        ctrl->f_evals = nfe;
        ctrl->t0 = t;
        ctrl->t1 = t_end;
    }
}

// The backward at 384 columns: the recursion of fcode_adaptive_bwd_kernel, one workgroup (8 waves) per 16 rows, W^T's `hi`
// fragments resident and its `lo` fragments streamed, the adjoint product on two planes and three products as there.  A lane
// owns twelve features of its row, so the seven stage adjoints gk_j (84 registers beside W's 144) do not stay in registers:
// they wait in the first seven row blocks of S, the half of the workspace adaptive_stage_inputs_kernel fills AFTER this
// kernel -- this workgroup's rows only, every lane re-reading only what it wrote itself, so no fence.  gk_1 of a step (the
// FSAL adjoint the step before adds to its gk_7) is read from its block before that step overwrites it.
template <int ACT>
__global__ __launch_bounds__(XT) void fcode_adaptive_wide_bwd_kernel(const float* __restrict__ traj,
                                                                     const OdeCtrl* __restrict__ ctrl,
                                                                     const float* __restrict__ gy,
                                                                     const bf16x8* __restrict__ wtf_hi,
                                                                     const bf16x8* __restrict__ wtf_lo, int b, int max_steps,
                                                                     float* __restrict__ gx, float* __restrict__ GZ,
                                                                     float* S, int Bp) {
    __shared__ __attribute__((aligned(16))) char smem[XPLANES_BWD];
    __shared__ float bc[28];      // this step's dt A[i][j] at i (i - 1) / 2 + j (i = 1 .. 6, j < i), dt w_j at 21 + j
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int brow = blockIdx.x * FROWS + (lane & 15);
    const int nf = wave * (16 * XTILES) + (lane >> 4) * 4;
    const bool live = brow < b;
    const int status = __builtin_amdgcn_readfirstlane(ctrl->status);
    int N = __builtin_amdgcn_readfirstlane(ctrl->accepted);
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // this lane's tile 0 within a [rows][384] block: a uniform base plus a 32-bit offset
    const size_t rbase = (size_t)blockIdx.x * (FROWS * XD);
    const unsigned loff = (lane & 15) * XD + nf;
    if (status != 0) {      // the forward returned NaN: so does the backward (row block 0 is the only one the sums read)
        const float qnan = __builtin_nanf("");
        const f32x4 n4 = {qnan, qnan, qnan, qnan};
#pragma unroll
        for (int t = 0; t < XTILES; ++t) {
            *(f32x4*)(GZ + rbase + loff + 16 * t) = live ? n4 : zero4;
            if (live) *(f32x4*)(gx + rbase + loff + 16 * t) = n4;
            __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
        }
        return;
    }

    const bf16x8* fh = wtf_hi + (size_t)wave * (XKS * XTILES * 64) + lane;
    const bf16x8* fl = wtf_lo + (size_t)wave * (XKS * XTILES * 64) + lane;
    bf16x8 wh[XKS][XTILES];
#pragma unroll
    for (int ks = 0; ks < XKS; ++ks)
#pragma unroll
        for (int t = 0; t < XTILES; ++t) wh[ks][t] = fh[(ks * XTILES + t) * 64];

    int buf = 0;
    const int soff = (lane & 15) * XYRB + nf * 2;
    const int boff = (lane & 15) * XYRB + (lane >> 4) * 16;
    auto put = [&](int t, const f32x4& v) {
        char* hi = smem + buf * (2 * FROWS * XYRB) + soff + 32 * t;
        bf16_t h[4], l[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) split_bf16(v[r], h[r], l[r]);
        *(u32x2*)hi = u32x2{pack2(h[0], h[1]), pack2(h[2], h[3])};
        *(u32x2*)(hi + FROWS * XYRB) = u32x2{pack2(l[0], l[1]), pack2(l[2], l[3])};
    };
    auto times_w = [&]() -> Tiles3 {
        bf16x8 lring[XRING][XTILES];
        ring_prime(fl, lring);
        __syncthreads();
        const Tiles3 r = mfma_streamed<2>(wh, fl, smem + buf * (2 * FROWS * XYRB), lring, boff);
        buf ^= 1;
        return r;
    };
    // (the lane offset is made opaque once per stage: the ~60 addresses of a step are loop-invariant, and a compiler that
    // knows it keeps them all as 64-bit pairs across the step loop -- scratch)
    unsigned lo = loff;
    // a row beyond b reads the trajectory of row b - 1 (every workgroup has a live row) and discards it: no branch round a load
    unsigned lk = ((brow < b ? brow : b - 1) - blockIdx.x * FROWS) * XD + nf;
    auto ld = [&](int n, int sub, int t) -> f32x4 {
        return *(const f32x4*)(traj + (((size_t)n * 8 + sub) * b * XD + rbase) + lk + 16 * t);
    };
    auto sel = [&](const f32x4& v) -> f32x4 { return live ? v : zero4; };
    auto emit = [&](int blk, int t, const f32x4& gz) { *(f32x4*)(GZ + ((size_t)blk * Bp * XD + rbase) + lo + 16 * t) = gz; };
    auto gkp = [&](int j, int t) -> float* { return S + ((size_t)j * Bp * XD + rbase) + lo + 16 * t; };

    Tiles3 a;
#pragma unroll
    for (int t = 0; t < XTILES; ++t) a.t[t] = live ? *(const f32x4*)(gy + rbase + loff + 16 * t) : zero4;
    for (int n = N - 1; n >= 0; --n) {
        __syncthreads();          // the step before has read its constants
        if (tid < 28) {           // one constant per thread (computed by every lane they are hoisted as fp64 and spilled)
            const double dt = ctrl->dt[n];
            double c;
            if (tid < 21) {
                int i = 1;
                while ((i + 1) * i / 2 <= tid) ++i;
                c = DP_A[i][tid - i * (i - 1) / 2];
            } else {
                c = DP_CS[tid - 21];
                if (n == N - 1) {       // the last step ends at its interpolant
                    const double t0 = ctrl->t0, t1 = ctrl->t1;
                    c = dp_beta(tid - 21, (1. - t0) / (t1 - t0));
                }
            }
            bc[tid] = (float)(dt * c);
        }
        __syncthreads();
#pragma unroll
        for (int i = 6; i >= 1; --i) {
            asm volatile("" : "+v"(lo), "+v"(lk));
            // gz_{i+1} = gk_{i+1} act'(k_{i+1}); stage 7's gk is dt w_7 a plus the FSAL adjoint of the step after
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
                f32x4 gk;
                if (i == 6) {
                    gk = uniform_f(bc[27]) * a.t[t];
                    if (n != N - 1) gk += *(const f32x4*)gkp(0, t);
                } else {
                    gk = *(const f32x4*)gkp(i, t);
                }
                const f32x4 gz = sel(gk * dact_out<ACT>(ld(n, 1 + i, t)));
                emit(6 * n + (i - 1), t, gz);
                put(t, gz);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles3 gs = times_w();
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
#pragma unroll
                for (int j = 0; j < i; ++j) {
                    const f32x4 base = i == 6 ? uniform_f(bc[21 + j]) * a.t[t] : *(const f32x4*)gkp(j, t);
                    *(f32x4*)gkp(j, t) = base + uniform_f(bc[i * (i - 1) / 2 + j]) * gs.t[t];
                }
                a.t[t] += gs.t[t];
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
        }
        if (n == 0) {
            asm volatile("" : "+v"(lo), "+v"(lk));
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
                const f32x4 gz = sel(*(const f32x4*)gkp(0, t) * dact_out<ACT>(ld(0, 1, t)));
                emit(6 * N, t, gz);
                put(t, gz);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles3 gs = times_w();
#pragma unroll
            for (int t = 0; t < XTILES; ++t) a.t[t] += gs.t[t];
        }
    }
    if (N == 0) {
#pragma unroll
        for (int t = 0; t < XTILES; ++t) emit(0, t, zero4);
    }
    if (live) {
#pragma unroll
        for (int t = 0; t < XTILES; ++t) *(f32x4*)(gx + rbase + loff + 16 * t) = a.t[t];
    }
}

}  // namespace agp_fusion
using namespace agp_fusion;

static bool adaptive_args_ok(int b, int act, int method, int max_steps) {
    return b > 0 && method == AGP_ODE_DOPRI5 && act >= AGP_ACT_ID && act <= AGP_ACT_SIGMOID && max_steps >= 1 &&
           max_steps <= AGP_ODE_MAX_STEPS_LIMIT;
}

extern "C" int64_t agp_fcode_adaptive_ctrl_bytes(int max_steps) {
    return max_steps < 1 ? 0 : (int64_t)sizeof(agp_ode_stats) + 3 * (int64_t)max_steps * sizeof(double);
}

extern "C" int64_t agp_fcode_adaptive_ring_floats(int b, int max_steps, int want_traj) {
    if (b <= 0 || max_steps < 1) return 0;
    return (int64_t)(want_traj ? max_steps + 1 : 2) * 8 * b * 256;
}

extern "C" int agp_fcode_adaptive_fwd(const float* x, const float* add1, const float* add2, const void* w_hi,
                                      const void* w_lo, const float* bias, int b, int act, int method, double rtol,
                                      double atol, int max_steps, float* y, float* ring, int want_traj, void* ctrl,
                                      void* stream) {
    if (!x || !w_hi || !w_lo || !y || !ring || !ctrl || !adaptive_args_ok(b, act, method, max_steps)) return AGP_E_BADARG;
    if (!(rtol >= 0.) || !(atol >= 0.) || !(rtol + atol > 0.)) return AGP_E_BADARG;
    static_assert(sizeof(agp_ode_stats) == 32 && offsetof(OdeCtrl, dt) == 32, "control block layout");
    const int nring = want_traj ? max_steps + 1 : 2;
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* wh = (const bf16_t*)w_hi;
    const bf16_t* wl = (const bf16_t*)w_lo;
    OdeCtrl* c = (OdeCtrl*)ctrl;
    const dim3 grid(1), blk(FT);
    switch (act) {
        case AGP_ACT_ID: AGP_LAUNCH(fcode_adaptive_kernel<AGP_ACT_ID>, grid, blk, 0, s, x, add1, add2, wh, wl, bias, b, rtol, atol, max_steps, ring, nring, y, c); break;
        case AGP_ACT_RELU: AGP_LAUNCH(fcode_adaptive_kernel<AGP_ACT_RELU>, grid, blk, 0, s, x, add1, add2, wh, wl, bias, b, rtol, atol, max_steps, ring, nring, y, c); break;
        case AGP_ACT_TANH: AGP_LAUNCH(fcode_adaptive_kernel<AGP_ACT_TANH>, grid, blk, 0, s, x, add1, add2, wh, wl, bias, b, rtol, atol, max_steps, ring, nring, y, c); break;
        default: AGP_LAUNCH(fcode_adaptive_kernel<AGP_ACT_SIGMOID>, grid, blk, 0, s, x, add1, add2, wh, wl, bias, b, rtol, atol, max_steps, ring, nring, y, c); break;
    }
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int64_t agp_fcode_adaptive_bwd_workspace_bytes(int b, int max_steps) {
    if (b <= 0 || max_steps < 1) return 0;
    const int64_t Bp = (b + FROWS - 1) / FROWS * FROWS;
    return 2 * (6 * (int64_t)max_steps + 1) * Bp * 256 * sizeof(float);
}

extern "C" int agp_fcode_adaptive_bwd(const float* traj, const void* ctrl, const float* gy, const void* wt_hi,
                                      const void* wt_lo, int b, int act, int method, int max_steps, float* gx, float* gw,
                                      float* gb, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!traj || !ctrl || !gy || !wt_hi || !wt_lo || !gx || !workspace || !adaptive_args_ok(b, act, method, max_steps))
        return AGP_E_BADARG;
    if (workspace_bytes < agp_fcode_adaptive_bwd_workspace_bytes(b, max_steps)) return AGP_E_BADARG;
    const int Bp = (b + FROWS - 1) / FROWS * FROWS;
    float* GZ = (float*)workspace;
    float* S = GZ + (6 * (size_t)max_steps + 1) * Bp * 256;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(Bp / FROWS), blk(FT);
    const bf16_t* wh = (const bf16_t*)wt_hi;
    const bf16_t* wl = (const bf16_t*)wt_lo;
    const OdeCtrl* c = (const OdeCtrl*)ctrl;
    switch (act) {
        case AGP_ACT_ID: AGP_LAUNCH(fcode_adaptive_bwd_kernel<AGP_ACT_ID>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, Bp); break;
        case AGP_ACT_RELU: AGP_LAUNCH(fcode_adaptive_bwd_kernel<AGP_ACT_RELU>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, Bp); break;
        case AGP_ACT_TANH: AGP_LAUNCH(fcode_adaptive_bwd_kernel<AGP_ACT_TANH>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, Bp); break;
        default: AGP_LAUNCH(fcode_adaptive_bwd_kernel<AGP_ACT_SIGMOID>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, Bp); break;
    }
    AGP_CHECK_LAUNCH();
    if (gw) {
        AGP_LAUNCH(adaptive_stage_inputs_kernel<AD>, dim3(Bp * 64 / 256, max_steps), dim3(256), 0, s, traj, c, b, max_steps, S, Bp);
        AGP_CHECK_LAUNCH();
        AGP_LAUNCH(adaptive_gw_kernel<AD>, dim3(4, 4), dim3(256), 0, s, GZ, S, gw, c, max_steps, Bp);
        AGP_CHECK_LAUNCH();
    }
    if (gb) {
        AGP_LAUNCH(adaptive_gb_kernel<AD>, dim3(4), dim3(256), 0, s, GZ, gb, c, max_steps, Bp);
        AGP_CHECK_LAUNCH();
    }
    return AGP_OK;
}

// ---- 384 columns
extern "C" int64_t agp_fcode_adaptive_wide_ring_floats(int b, int d, int max_steps, int want_traj) {
    if (b <= 0 || d != XD || max_steps < 1) return 0;
    return (int64_t)(want_traj ? max_steps + 1 : 2) * 8 * b * XD;
}

extern "C" int agp_fcode_adaptive_wide_fwd(const float* x, const float* add1, const float* add2, const void* wf_hi,
                                           const void* wf_lo, const float* bias, int b, int d, int act, int method,
                                           double rtol, double atol, int max_steps, float* y, float* ring, int want_traj,
                                           void* ctrl, void* stream) {
    if (!x || !wf_hi || !wf_lo || !y || !ring || !ctrl || d <= 0 || !adaptive_args_ok(b, act, method, max_steps))
        return AGP_E_BADARG;
    if (!(rtol >= 0.) || !(atol >= 0.) || !(rtol + atol > 0.)) return AGP_E_BADARG;
    if (d != XD) return AGP_E_UNSUPPORTED;
    const int nring = want_traj ? max_steps + 1 : 2;
    hipStream_t s = (hipStream_t)stream;
    const bf16x8* wh = (const bf16x8*)wf_hi;
    const bf16x8* wl = (const bf16x8*)wf_lo;
    OdeCtrl* c = (OdeCtrl*)ctrl;
    const dim3 grid(1), blk(XT);
    static std::atomic<uint64_t> attr_done[4];
#define AGP_ADAPTIVE_WIDE_CASE(A)                                                                                          \
    case A:                                                                                                                \
        if (!agp_lds_attr((const void*)fcode_adaptive_wide_kernel<A>, XLDS_FWD, attr_done[A])) return AGP_E_LAUNCH;        \
        AGP_LAUNCH(fcode_adaptive_wide_kernel<A>, grid, blk, XLDS_FWD, s, x, add1, add2, wh, wl, bias, b, rtol, atol,      \
                   max_steps, ring, nring, y, c);                                                                          \
        break;
    switch (act) {
        AGP_ADAPTIVE_WIDE_CASE(AGP_ACT_ID) AGP_ADAPTIVE_WIDE_CASE(AGP_ACT_RELU) AGP_ADAPTIVE_WIDE_CASE(AGP_ACT_TANH)
        AGP_ADAPTIVE_WIDE_CASE(AGP_ACT_SIGMOID)
        default: return AGP_E_BADARG;
    }
#undef AGP_ADAPTIVE_WIDE_CASE
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int64_t agp_fcode_adaptive_wide_bwd_workspace_bytes(int b, int d, int max_steps) {
    if (b <= 0 || d != XD || max_steps < 1) return 0;
    const int64_t Bp = (b + FROWS - 1) / FROWS * FROWS;
    return 2 * (6 * (int64_t)max_steps + 1) * Bp * XD * sizeof(float);
}

extern "C" int agp_fcode_adaptive_wide_bwd(const float* traj, const void* ctrl, const float* gy, const void* wtf_hi,
                                           const void* wtf_lo, int b, int d, int act, int method, int max_steps, float* gx,
                                           float* gw, float* gb, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!traj || !ctrl || !gy || !wtf_hi || !wtf_lo || !gx || !workspace || d <= 0 ||
        !adaptive_args_ok(b, act, method, max_steps))
        return AGP_E_BADARG;
    if (d != XD) return AGP_E_UNSUPPORTED;
    if (workspace_bytes < agp_fcode_adaptive_wide_bwd_workspace_bytes(b, d, max_steps)) return AGP_E_BADARG;
    const int Bp = (b + FROWS - 1) / FROWS * FROWS;
    float* GZ = (float*)workspace;
    float* S = GZ + (6 * (size_t)max_steps + 1) * Bp * XD;      // (the state kernel's scratch first, then the stage inputs)
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(Bp / FROWS), blk(XT);
    const bf16x8* wh = (const bf16x8*)wtf_hi;
    const bf16x8* wl = (const bf16x8*)wtf_lo;
    const OdeCtrl* c = (const OdeCtrl*)ctrl;
    switch (act) {
        case AGP_ACT_ID: AGP_LAUNCH(fcode_adaptive_wide_bwd_kernel<AGP_ACT_ID>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, S, Bp); break;
        case AGP_ACT_RELU: AGP_LAUNCH(fcode_adaptive_wide_bwd_kernel<AGP_ACT_RELU>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, S, Bp); break;
        case AGP_ACT_TANH: AGP_LAUNCH(fcode_adaptive_wide_bwd_kernel<AGP_ACT_TANH>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, S, Bp); break;
        default: AGP_LAUNCH(fcode_adaptive_wide_bwd_kernel<AGP_ACT_SIGMOID>, grid, blk, 0, s, traj, c, gy, wh, wl, b, max_steps, gx, GZ, S, Bp); break;
    }
    AGP_CHECK_LAUNCH();
    if (gw) {
        AGP_LAUNCH(adaptive_stage_inputs_kernel<XD>, dim3(Bp * (XD / 4) / 256, max_steps), dim3(256), 0, s, traj, c, b, max_steps, S, Bp);
        AGP_CHECK_LAUNCH();
        AGP_LAUNCH(adaptive_gw_kernel<XD>, dim3(XD / 64, XD / 64), dim3(256), 0, s, GZ, S, gw, c, max_steps, Bp);
        AGP_CHECK_LAUNCH();
    }
    if (gb) {
        AGP_LAUNCH(adaptive_gb_kernel<XD>, dim3(XD / 64), dim3(256), 0, s, GZ, gb, c, max_steps, Bp);
        AGP_CHECK_LAUNCH();
    }
    return AGP_OK;
}
