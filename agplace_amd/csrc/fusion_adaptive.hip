// Adaptive embedded Runge-Kutta solvers for the Neural-ODE blocks FCODE(256) and FCODE(384), forward and backward: 'dopri5'
// (Dormand-Prince 5(4)) and 'bosh3' (Bogacki-Shampine 3(2)).  A method is a Tableau (below): a type the forward driver and
// the backward kernels take as a template parameter; step control, ring, control block, interpolant and both backward
// recursions are written once for every FSAL table of at most seven stages.
// The algorithm is stated in DESIGN.md section 2 ("Adaptive solver") and restated in fp64 by tests/dopri5_ref.py (dopri5)
// and tests/rk_adaptive_ref.py (any table).
//
// Forward: ONE launch of ONE persistent workgroup per solve.  torchdiffeq's step control couples the whole batch (one error
// norm over all b*D elements), so a workgroup per 16 rows would have to wait for the others at every attempted step; a
// single workgroup needs nothing but its own barriers.  There is ONE driver, fcode_adaptive_kernel<E, TB, ACT>: step control,
// tableau arithmetic, ring and control block exist once.  What differs between the widths is a column engine E (below,
// before the driver): Resident256 keeps both split-bf16 planes of W in registers as fcode_kernel does (fusion.hip), 16 waves,
// a lane owns 4 features of a row; Streamed384 cannot (576 KiB of planes), keeps `hi`, streams `lo`, 8 waves, a lane owns
// 3 x 4 features.  At either width the state has a third bf16 plane (see store_state3) and the workgroup walks the
// ceil(b/16) row tiles for every stage.  y and the S stage derivatives live in a caller-supplied ring in global memory
// (L2-resident); a lane only ever re-reads the addresses it wrote itself (same row, same features), so the ring needs no
// fence.  Ring entry n holds [y, k1 .. kS] of the attempt that starts from accepted step n (eight sub-planes whatever S is:
// a table with fewer than seven stages leaves the last ones unused); stage S writes y1 and kS also
// to entry n + 1 as its (y, k1) -- FSAL -- so accepting a step is `++n` and rejecting it leaves entry n as it was.  With a
// trajectory the ring has max_steps + 1 entries and IS the record the backward reads; without one it has two.
// Time, step size, norms, the error ratio and the step factor are fp64.  Norms are reduced in a fixed order (a lane over
// its row tiles, feature tiles and elements in index order, butterfly over the wave, the waves in wave order): two runs
// give the same bits.
//
// Backward: rows are independent once the step sizes are fixed: one workgroup per 16 rows like
// fcode_bwd_state_kernel (fusion_bwd.hip), step count and step sizes read from the control block in DEVICE memory.  The
// two widths keep their own recursions (where the S stage adjoints live differs in substance); the per-step constants,
// the read of the solve's outcome and act' are shared, and so are the three sum kernels, templated on the width.
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

// Bogacki-Shampine 3(2), FSAL as well.  MID is torchdiffeq's: y_mid = y + dt k2 / 2, the midpoint rule's value.
__device__ const double BS_A[4][3] = {{0., 0., 0.}, {1. / 2, 0., 0.}, {0., 3. / 4, 0.}, {2. / 9, 1. / 3, 4. / 9}};
__device__ const double BS_CS[4] = {2. / 9, 1. / 3, 4. / 9, 0.};
__device__ const double BS_CE[4] = {2. / 9 - 7. / 24, 1. / 3 - 1. / 4, 4. / 9 - 1. / 3, -1. / 8};
__device__ const double BS_MID[4] = {0., 0.5, 0., 0.};

// A Tableau is an embedded explicit FSAL method of S <= 7 stages: k_1 = f(y) (the step before's k_S),
// k_i = f(y + dt sum_{j < i} A[i-1][j] k_j) for i = 2 .. S, row S - 1 of A being the solution weights CS (so k_S = f(y1)),
// the error estimate dt sum_j CE[j] k_j of a method of order ORDER (the step factor is ratio^(-1/ORDER)), and the
// mid-point weights MID of the quartic interpolant.  METHOD is its AGP_ODE_* number.
struct Dopri5 {
    static constexpr int S = 7, ORDER = 5, METHOD = AGP_ODE_DOPRI5;
    static __device__ __forceinline__ double A(int i, int j) { return DP_A[i][j]; }
    static __device__ __forceinline__ double CS(int j) { return DP_CS[j]; }
    static __device__ __forceinline__ double CE(int j) { return DP_CE[j]; }
    static __device__ __forceinline__ double MID(int j) { return DP_MID[j]; }
};
struct Bosh3 {
    static constexpr int S = 4, ORDER = 3, METHOD = AGP_ODE_BOSH3;
    static __device__ __forceinline__ double A(int i, int j) { return BS_A[i][j]; }
    static __device__ __forceinline__ double CS(int j) { return BS_CS[j]; }
    static __device__ __forceinline__ double CE(int j) { return BS_CE[j]; }
    static __device__ __forceinline__ double MID(int j) { return BS_MID[j]; }
};

// out = y + dt sum_j beta_j(x) k_j is the quartic interpolant of a step at x in [0, 1]: the quartic through y, y_mid and y1
// with the end slopes k_1 and k_S; beta(1) = CS
template <class T>
__device__ __forceinline__ double rk_beta(int j, double x) {
    const double d1 = j == 0 ? 1. : 0., dS = j == T::S - 1 ? 1. : 0.;
    const double c4 = 16. * T::MID(j) - 8. * T::CS(j) + 2. * (dS - d1);
    const double c3 = 14. * T::CS(j) - 32. * T::MID(j) + 5. * d1 - 3. * dS;
    const double c2 = 16. * T::MID(j) - 5. * T::CS(j) + dS - 4. * d1;
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

// z^P by squaring (P = 5: (z^2 z^2) z)
template <int P>
__device__ __forceinline__ double ipow(double z) {
    if constexpr (P == 1) {
        return z;
    } else if constexpr (P % 2 == 1) {
        return ipow<P - 1>(z) * z;
    } else {
        const double h = ipow<P / 2>(z);
        return h * h;
    }
}
// r^(-1/P) for finite r > 0, to fp64 accuracy: r = a (2^P)^q with a in [1/2, 2^(P-1)), a single-precision power of a, two
// Newton steps z <- z (P + 1 - a z^P) / P (quadratic: 1e-7 -> 1e-14 -> rounding).  A double-precision pow() next to W's 64
// resident registers spills; this does not.
template <int P>
__device__ __forceinline__ double inv_root(double r) {
    int e;
    const double m = frexp(r, &e);
    const int q = e >= 0 ? e / P : -((P - 1 - e) / P);
    const double a = ldexp(m, e - P * q);
    double z = (double)powf((float)a, -1.f / P);
#pragma unroll
    for (int it = 0; it < 2; ++it) z = z * ((P + 1.) - a * ipow<P>(z)) * (1. / P);
    return ldexp(z, -q);
}
// fn(integral_constant<int, I>) for I = FROM .. TO, unrolled
template <int FROM, int TO, class F>
__device__ __forceinline__ void static_for(F&& fn) {
    if constexpr (FROM <= TO) {
        fn(std::integral_constant<int, FROM>{});
        static_for<FROM + 1, TO>(fn);
    }
}

constexpr int AD = 256, AKS = AD / 32, AYRB = AD * 2 + 16;

// f for the adaptive solver: the STATE as three bf16 planes (hi + mid + lo = 24 bits), five products
// W_hi (y_hi + y_mid + y_lo) + W_lo (y_hi + y_mid).  The fixed-grid kernels' two-plane state carries 2^-17 of rounding per
// element and stage, fresh at every stage; W k turns it into 1e-5 of noise on each k_i, and the error estimate
// dt sum CE_j k_j is a cancelling sum of them: at a ratio of 0.1 and tol = 1e-4 it was mostly that noise (step sizes 40 %
// off the fp64 restatement's on the device).  W keeps its two resident planes: their rounding is the same at every
// stage, i.e. a slightly different but smooth right-hand side, which the estimate is indifferent to.
// (hi = this lane's four features in the `hi` plane; `mid` and `lo` lie plane_bytes and 2 plane_bytes above it)
__device__ __forceinline__ void store_state3(char* hi, int plane_bytes, const f32x4& v) {
    bf16_t h[4], m[4], l[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h[r] = f2bf(v[r]);
        const float r1 = v[r] - bf2f(h[r]);
        m[r] = f2bf(r1);
        l[r] = f2bf(r1 - bf2f(m[r]));
    }
    *(u32x2*)hi = u32x2{pack2(h[0], h[1]), pack2(h[2], h[3])};
    *(u32x2*)(hi + plane_bytes) = u32x2{pack2(m[0], m[1]), pack2(m[2], m[3])};
    *(u32x2*)(hi + 2 * plane_bytes) = u32x2{pack2(l[0], l[1]), pack2(l[2], l[3])};
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

// ---------------------------------------------------------------------------------------------------------------------
// The work shape at 384 columns (the forward's Streamed384 engine and fcode_adaptive_wide_bwd_kernel).  Both split-bf16 planes
// of a 384 x 384 W are 576 KiB, more than a CU's register file, so the shape is fcode_wide_kernel's (fusion_wide.hip): a
// workgroup of 8 waves, wave w owns the three 16-feature tiles [48 w, 48 w + 48) over the full K; the 36 `hi` fragments stay
// in registers (144), the `lo` fragments of the same (tile, K-step) pairs are streamed from L2 through a ring of XRING
// K-steps, in the fragment order of ops.fcode_wide_planes; no K split, hence no cross-wave sum and ONE barrier per
// evaluation and row tile.  A lane owns twelve features of a row here (row l & 15 of a tile, features
// 48 w + 16 t + 4 (l >> 4) + r), not four.
constexpr int XD = 384, XT = 512, XKS = XD / 32, XTILES = 3, XRING = 3, XYRB = XD * 2 + 16, XWAVES = XT / 64;
constexpr int XPLANES_FWD = 2 * 3 * FROWS * XYRB;      // 75264 B: [buf][plane hi, mid, lo]; more than 64 KB (agp_lds_attr)
constexpr int XPLANES_BWD = 2 * 2 * FROWS * XYRB;      // 50176 B: [buf][plane hi, lo]
constexpr int XLDS_FWD = XPLANES_FWD + XD * 4;         // + the bias

// a lane's share of one 16-row tile: four features in each of its N feature tiles
template <int N>
struct Tiles {
    f32x4 t[N];
};
using Tiles3 = Tiles<XTILES>;

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


// per-attempt constants, written by thread 0 and read by every wave into scalar registers: the products of dt with the
// tableau.  (Computed by every lane they are hoisted out of the step loop as 50 fp64 values and spilled.)
template <class T>
struct StepCoef {
    double dt;
    double ce[T::S];               // dt * CE
    float a[T::S - 2][T::S - 2];   // dt * A rows 1 .. S - 2
    float cs[T::S - 1];            // dt * CS
};
template <class T>
__device__ __forceinline__ void publish_step(StepCoef<T>& c, double dt) {
    c.dt = dt;
#pragma unroll
    for (int j = 0; j < T::S; ++j) c.ce[j] = dt * T::CE(j);
#pragma unroll
    for (int i = 1; i <= T::S - 2; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) c.a[i - 1][j] = (float)(dt * T::A(i, j));
#pragma unroll
    for (int j = 0; j < T::S - 1; ++j) c.cs[j] = (float)(dt * T::A(T::S - 1, j));
}
// ---- The forward's two column engines: what differs between the widths, i.e. where W lives, how a tile of the state gets
// into LDS and how f is evaluated on it.  put(t, v) writes this lane's feature tile t of the state the next evaluation reads
// (three bf16 planes, double-buffered); feval<ACT>() is act(W state + bias) on this lane's features of the 16 rows, behind
// the one barrier that publishes the put()s.  An engine knows nothing of the solver: no tableau, no step control.

// 256 columns: both planes of W resident (64 registers), 16 waves of 16 features each, the bias in registers, static LDS
struct Resident256 {
    static constexpr int D = AD, THREADS = FT, TILES = 1, WAVES = FT / 64, LDS_DYNAMIC = 0;
    static constexpr int BUF = 3 * FROWS * AYRB;      // [plane hi, mid, lo] of one buffer
    using Plane = const bf16_t*;                      // a row-major [256][256] plane of ops.LinearWeights
    bf16x8 wh[AKS], wl[AKS];
    f32x4 bia;
    char* smem;
    int lane, nf, buf;      // nf: this lane's first feature
    __device__ __forceinline__ void init(Plane w_hi, Plane w_lo, const float* bias, int, int lane_, int wave) {
        __shared__ __attribute__((aligned(16))) char planes[2 * BUF];
        smem = planes;
        lane = lane_;
        buf = 0;
        nf = wave * 16 + (lane >> 4) * 4;
        const size_t wo = (size_t)(wave * 16 + (lane & 15)) * AD + (lane >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < AKS; ++ks) {
            wh[ks] = *(const bf16x8*)(w_hi + wo + ks * 32);
            wl[ks] = *(const bf16x8*)(w_lo + wo + ks * 32);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) bia[r] = bias ? bias[nf + r] : 0.f;
    }
    __device__ __forceinline__ void put(int, const f32x4& v) {
        store_state3(smem + buf * BUF + (lane & 15) * AYRB + nf * 2, FROWS * AYRB, v);
    }
    template <int ACT>
    __device__ __forceinline__ Tiles<1> feval() {
        const char* hi = smem + buf * BUF;
        __syncthreads();
        const f32x4 z = mfma_resident5<AKS>(wh, wl, hi, hi + FROWS * AYRB, hi + 2 * FROWS * AYRB, AYRB, lane);
        buf ^= 1;
        return {{act4<ACT>(z + bia)}};
    }
};

// 384 columns: `hi` resident (144 registers), `lo` streamed, 8 waves of three 16-feature tiles each, the bias in LDS (twelve
// more registers are not to be had), dynamic LDS: the state planes exceed 64 KB (agp_lds_attr)
struct Streamed384 {
    static constexpr int D = XD, THREADS = XT, TILES = XTILES, WAVES = XWAVES, LDS_DYNAMIC = XLDS_FWD;
    static constexpr int BUF = 3 * FROWS * XYRB;
    using Plane = const bf16x8*;                      // a plane in fragment order (ops.fcode_wide_planes)
    bf16x8 wh[XKS][XTILES];
    const bf16x8* fl;
    char* smem;
    float* sbias;
    int nf, soff, boff, buf;      // nf: this lane's first feature of tile 0; tile t at + 16 t
    __device__ __forceinline__ void init(Plane wf_hi, Plane wf_lo, const float* bias, int tid, int lane, int wave) {
        extern __shared__ __attribute__((aligned(16))) char planes[];      // XLDS_FWD: the state planes [buf][plane], the bias
        smem = planes;
        sbias = (float*)(planes + XPLANES_FWD);
        buf = 0;
        nf = wave * (16 * XTILES) + (lane >> 4) * 4;
        soff = (lane & 15) * XYRB + nf * 2;                 // where this lane's 4 features of tile 0 go in a plane
        boff = (lane & 15) * XYRB + (lane >> 4) * 16;       // this lane's B fragment of K-step 0
        const bf16x8* fh = wf_hi + (size_t)wave * (XKS * XTILES * 64) + lane;
        fl = wf_lo + (size_t)wave * (XKS * XTILES * 64) + lane;
#pragma unroll
        for (int ks = 0; ks < XKS; ++ks)
#pragma unroll
            for (int t = 0; t < XTILES; ++t) wh[ks][t] = fh[(ks * XTILES + t) * 64];
        if (tid < XD) sbias[tid] = bias ? bias[tid] : 0.f;     // (published by the first evaluation's barrier)
    }
    __device__ __forceinline__ void put(int t, const f32x4& v) { store_state3(smem + buf * BUF + soff + 32 * t, FROWS * XYRB, v); }
    template <int ACT>
    __device__ __forceinline__ Tiles3 feval() {
        bf16x8 lring[XRING][XTILES];
        ring_prime(fl, lring);
        __syncthreads();
        Tiles3 z = mfma_streamed<3>(wh, fl, smem + buf * BUF, lring, boff);
        buf ^= 1;
#pragma unroll
        for (int t = 0; t < XTILES; ++t) {
            z.t[t] = act4<ACT>(z.t[t] + *(const f32x4*)(sbias + nf + 16 * t));
            __builtin_amdgcn_sched_barrier(0);      // one tile at a time (twelve interleaved sigmoid divisions cost scratch)
        }
        return z;
    }
};

// ---- The forward driver, once for both widths and every Tableau TB: first step size, stages 2 .. S - 1, stage S (the FSAL
// stage) with the error ratio, accept / reject
// and the step factor, the interpolant at t = 1, the NaN fill of a failed solve, the control block.  Its shape is the one a
// lane with several feature tiles needs: the stage combinations run one feature tile at a time (put), then ONE evaluation
// (feval), and stage S forms its error sum AFTER the evaluation from the ring (y1 is already in entry n + 1), so nothing
// state-sized waits in registers across an evaluation; with TILES = 1 the same loops are the four-features-per-lane walk.
// The sched_barrier(0) after each feature tile and the scalar (readfirstlane) coefficients are there because their removal
// spilled at 384 columns.
// Two places know that a lane may own a single feature tile (if constexpr, TILES == 1); both were forced by a measurement
// of the plain form at 256 columns (MI355X, dopri5, relu, tol 1e-3, captured solve; the two-kernel build 115.89 / 346.96 us at
// b = 16 / 64, spread 0.05 / 0.30):
//   - stage S HOLDS y, y1 and the error sum of stages 1 .. S - 1 in registers across the evaluation and stores y1 behind it.
//     Read back from the ring -- what a lane with three tiles must do -- the solve took 116.95 / 372.36 us (+0.9 / +7.3 %:
//     eight more 16-byte loads per lane, row tile and attempt); held, but with y1 stored ahead of the evaluation, 347.80 us
//     at b = 64 (the store then sits right before the evaluation's barrier).  As it stands: 109.39 / 337.04 us.
//   - the interpolant's S weights are computed by every lane, not one per thread through LDS: sbeta would add 32 B to
//     the 256 engine's static LDS (51168 B against 51136).  (Behind the step loop the per-lane form does not spill as it
//     did inside it; at 384 columns the weights keep going through LDS, as they did.)
template <class E, class TB, int ACT>
__global__ __launch_bounds__(E::THREADS) void fcode_adaptive_kernel(const float* __restrict__ x, const float* __restrict__ add1,
                                                                   const float* __restrict__ add2,
                                                                   typename E::Plane __restrict__ w_hi,
                                                                   typename E::Plane __restrict__ w_lo,
                                                                   const float* __restrict__ bias, int b, double rtol,
                                                                   double atol, int max_steps, float* ring, int nring,
                                                                   float* __restrict__ yout, OdeCtrl* __restrict__ ctrl) {
    constexpr int D = E::D, TILES = E::TILES, S = TB::S;
    static_assert(S >= 3 && S <= 7, "a ring entry has eight sub-planes: y and at most seven stages");
    __shared__ double red[2][E::WAVES];
    __shared__ StepCoef<TB> coef;
    __shared__ float sbeta[S];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = (b + FROWS - 1) / FROWS;
    const double count = (double)b * D;
    const float rtolf = (float)rtol, atolf = (float)atol;

    E eng;
    eng.init(w_hi, w_lo, bias, tid, lane, wave);
    auto feval = [&]() -> Tiles<TILES> { return eng.template feval<ACT>(); };
    // ring[entry][sub][row][D]: sub 0 = y, 1 + j = k_{j+1}.  A uniform base plus this lane's 32-bit offset; tile t at + 16 t.
    const size_t plane = (size_t)b * D;
    const int loff = (lane & 15) * D + eng.nf;
    auto at = [&](int entry, int sub, int T) -> float* {
        return ring + ((size_t)(entry * 8 + sub) * plane + (size_t)T * (FROWS * D)) + loff;
    };
    // sums of two per-thread values over the workgroup, the same bits in every thread
    auto block_sum2 = [&](double& u, double& v) {
        u = wave_sum_f64(u);
        v = wave_sum_f64(v);
        __syncthreads();                      // the previous sums have been read
        if (lane == 0) { red[0][wave] = u; red[1][wave] = v; }
        __syncthreads();
        u = 0.; v = 0.;
        for (int w = 0; w < E::WAVES; ++w) { u += red[0][w]; v += red[1][w]; }
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- first step size (torchdiffeq _select_initial_step; the exponent is 1 / ORDER)
    double sq0 = 0., sq1 = 0.;
    for (int T = 0; T < nt; ++T) {
        const bool live = T * FROWS + (lane & 15) < b;
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            f32x4 yv = zero4;
            if (live) {
                const size_t g = (size_t)T * (FROWS * D) + loff + 16 * t;
                yv = *(const f32x4*)(x + g);
                if (add1) yv += *(const f32x4*)(add1 + g);
                if (add2) yv += *(const f32x4*)(add2 + g);
                *(f32x4*)(at(0, 0, T) + 16 * t) = yv;
            }
            eng.put(t, yv);
            __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
        }
        const Tiles<TILES> f0 = feval();
        if (live) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
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
            for (int t = 0; t < TILES; ++t) {
                f32x4 s = zero4;
                if (live) s = *(const f32x4*)(at(0, 0, T) + 16 * t) + h0f * *(const f32x4*)(at(0, 1, T) + 16 * t);
                eng.put(t, s);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles<TILES> f1 = feval();
            if (live) {
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
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
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : (dm < 1e298 ? inv_root<TB::ORDER>(dm * 100.) : 0.);
        publish_step(coef, fmin(100. * h0, h1));
    }
    __syncthreads();

    // stage I (0-based, 1 .. S - 2): k_{I+1} = f(y + dt sum_{j < I} A[I][j] k_{j+1})
    auto stage = [&](auto Ic, int cur) {
        constexpr int I = decltype(Ic)::value;
        float cf[I];
#pragma unroll
        for (int j = 0; j < I; ++j) cf[j] = uniform_f(coef.a[I - 1][j]);
        for (int T = 0; T < nt; ++T) {
            const bool live = T * FROWS + (lane & 15) < b;
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                f32x4 s = zero4;
                if (live) {
                    f32x4 kk[I];
                    s = *(const f32x4*)(at(cur, 0, T) + 16 * t);
#pragma unroll
                    for (int j = 0; j < I; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * t);
#pragma unroll
                    for (int j = 0; j < I; ++j) s += cf[j] * kk[j];
                }
                eng.put(t, s);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles<TILES> k = feval();
            if (live) {
#pragma unroll
                for (int t = 0; t < TILES; ++t) *(f32x4*)(at(cur, 1 + I, T) + 16 * t) = k.t[t];
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
        static_for<1, S - 2>([&](auto Ic) { stage(Ic, cur); });
        // stage S: y1, kS = f(y1) and the error ratio
        double sq = 0., sqx = 0.;
        {
            float cs[S - 1];
            double ce[S];
#pragma unroll
            for (int j = 0; j < S - 1; ++j) cs[j] = uniform_f(coef.cs[j]);
#pragma unroll
            for (int j = 0; j < S; ++j) ce[j] = uniform_d(coef.ce[j]);
            constexpr bool HOLD = TILES == 1;      // (see the kernel's head)
            // the cancelling sum in fp64, stages 1 .. S - 1
            auto err_head = [&](const f32x4 (&kk)[S - 1], int r) -> double {
                double e = 0.;
#pragma unroll
                for (int j = 0; j < S - 1; ++j) e += ce[j] * (double)kk[j][r];
                return e;
            };
            for (int T = 0; T < nt; ++T) {
                const bool live = T * FROWS + (lane & 15) < b;
                [[maybe_unused]] f32x4 yv_held = zero4, y1_held = zero4;
                [[maybe_unused]] double e_held[4] = {0., 0., 0., 0.};
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    f32x4 y1 = zero4;
                    if (live) {
                        f32x4 kk[S - 1];
                        const f32x4 yv = *(const f32x4*)(at(cur, 0, T) + 16 * t);
#pragma unroll
                        for (int j = 0; j < S - 1; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * t);
                        y1 = yv;
#pragma unroll
                        for (int j = 0; j < S - 1; ++j) y1 += cs[j] * kk[j];
                        if constexpr (HOLD) {
                            yv_held = yv;
                            y1_held = y1;
#pragma unroll
                            for (int r = 0; r < 4; ++r) e_held[r] = err_head(kk, r);
                        } else {
                            *(f32x4*)(at(nxt, 0, T) + 16 * t) = y1;
                        }
                    }
                    eng.put(t, y1);
                    __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
                }
                const Tiles<TILES> kS = feval();
                if (live) {
#pragma unroll
                    for (int t = 0; t < TILES; ++t) {
                        *(f32x4*)(at(cur, S, T) + 16 * t) = kS.t[t];
                        *(f32x4*)(at(nxt, 1, T) + 16 * t) = kS.t[t];
                        f32x4 yv = yv_held, y1 = y1_held;
                        double e[4] = {e_held[0], e_held[1], e_held[2], e_held[3]};
                        if constexpr (HOLD) {
                            *(f32x4*)(at(nxt, 0, T) + 16 * t) = y1;
                        } else {
                            f32x4 kk[S - 1];
                            yv = *(const f32x4*)(at(cur, 0, T) + 16 * t);
                            y1 = *(const f32x4*)(at(nxt, 0, T) + 16 * t);
#pragma unroll
                            for (int j = 0; j < S - 1; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * t);
#pragma unroll
                            for (int r = 0; r < 4; ++r) e[r] = err_head(kk, r);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            // the quotient in fp32 (1e-7 relative: nothing next to the k's own rounding)
                            const float ef = (float)(e[r] + ce[S - 1] * (double)kS.t[t][r]);
                            const double q = (double)(ef / (atolf + rtolf * fmaxf(fabsf(yv[r]), fabsf(y1[r]))));
                            sq += q * q;
                        }
                        __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
                    }
                }
            }
        }
        nfe += S - 1;
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
        // every wave has read this attempt's constants (the barriers of stage S lie behind their last read)
        if (tid == 0) {
            double fac = 10.;
            if (ratio != 0.) fac = fmin(10., fmax(ratio < 1e300 ? 0.9 * inv_root<TB::ORDER>(ratio) : 0., ratio < 1. ? 1. : 0.2));
            publish_step(coef, dt * fac);
        }
        __syncthreads();
    }
    if (status == 0) {     // the quartic interpolant of the last step at time 1 (behind the loop: inside it the quartic's fp64
                           // constants are hoisted out of the loop and spilled)
        const double dt = uniform_d(coef.dt);
        const int cur = __builtin_amdgcn_readfirstlane((acc - 1) % nring);
        const double xs = (1. - t) / (t_end - t);
        float be[S];
        if constexpr (TILES == 1) {      // (see the kernel's head)
#pragma unroll
            for (int j = 0; j < S; ++j) be[j] = uniform_f((float)(dt * rk_beta<TB>(j, xs)));
        } else {     // one weight per thread
            if (tid < S) sbeta[tid] = (float)(dt * rk_beta<TB>(tid, xs));
            __syncthreads();
#pragma unroll
            for (int j = 0; j < S; ++j) be[j] = uniform_f(sbeta[j]);
        }
        for (int T = 0; T < nt; ++T) {
            if (T * FROWS + (lane & 15) < b) {
#pragma unroll
                for (int tt = 0; tt < TILES; ++tt) {
                    f32x4 o = *(const f32x4*)(at(cur, 0, T) + 16 * tt);
                    f32x4 kk[S];
#pragma unroll
                    for (int j = 0; j < S; ++j) kk[j] = *(const f32x4*)(at(cur, 1 + j, T) + 16 * tt);
#pragma unroll
                    for (int j = 0; j < S; ++j) o += be[j] * kk[j];
                    *(f32x4*)(yout + (size_t)T * (FROWS * D) + loff + 16 * tt) = o;
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
                for (int tt = 0; tt < TILES; ++tt)
                    *(f32x4*)(yout + (size_t)T * (FROWS * D) + loff + 16 * tt) = f32x4{qnan, qnan, qnan, qnan};
            }
        t_end = t;
    }
    // the unused tail of the control block is zero: two equal solves leave equal blocks
    for (int i = tid; i < 3 * max_steps; i += E::THREADS)
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

// ---- Backward.  The two state kernels keep their own recursions (the S stage adjoints in registers at 256 columns, in the
// workspace at 384); what they and the three sum kernels share is below.

// the outcome of the solve a control block records, as uniform values: its status and its accepted steps, clamped to the cap
struct Solved {
    int status, N;
};
__device__ __forceinline__ Solved read_solved(const OdeCtrl* ctrl, int max_steps) {
    const int status = __builtin_amdgcn_readfirstlane(ctrl->status);
    const int N = __builtin_amdgcn_readfirstlane(ctrl->accepted);
    return {status, N < 0 ? 0 : (N > max_steps ? max_steps : N)};
}

// the constants of accepted step n of N into bc[NA + S], NA = S (S - 1) / 2: dt A[i][j] at i (i - 1) / 2 + j (i = 1 .. S - 1,
// j < i), dt w_j at NA + j (dopri5: 21 + 7, bosh3: 6 + 4).
// One constant per thread (computed by every lane they are hoisted as fp64 and spilled), between two barriers: the step
// before has read its constants, this step's are published.
template <class TB>
struct BwdCoef {
    static constexpr int NA = TB::S * (TB::S - 1) / 2, COUNT = NA + TB::S;
};
template <class TB>
__device__ __forceinline__ void publish_bwd_step(float (&bc)[BwdCoef<TB>::COUNT], const OdeCtrl* ctrl, int n, int N, int tid) {
    constexpr int NA = BwdCoef<TB>::NA;
    __syncthreads();
    if (tid < NA + TB::S) {
        const double dt = ctrl->dt[n];
        double c;
        if (tid < NA) {
            int i = 1;
            while ((i + 1) * i / 2 <= tid) ++i;
            c = TB::A(i, tid - i * (i - 1) / 2);
        } else {
            c = TB::CS(tid - NA);
            if (n == N - 1) {       // the last step ends at its interpolant
                const double t0 = ctrl->t0, t1 = ctrl->t1;
                c = rk_beta<TB>(tid - NA, (1. - t0) / (t1 - t0));
            }
        }
        bc[tid] = (float)(dt * c);
    }
    __syncthreads();
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
// (i = 2 .. S, A_S = CS), out = y + dt sum_j w_j k_j with w = CS (out = s_S) or, for the last step, w = beta(x).
// k_1 of step n + 1 IS k_S of step n (FSAL), so the adjoint of k_1 is carried into the step before (gfsal).  With a = dL/d out:
//     gk_j = dt w_j a (+ gfsal for j = S);  for i = S .. 2: gz_i = gk_i act'(k_i), gs_i = gz_i W, a += gs_i,
//     gk_j += dt A_ij gs_i (j < i);  gfsal <- gk_1;  at step 0: gz_1 = gk_1 act'(k_1), a += gz_1 W.
// Every gz_i goes to the workspace, row block (S - 1) n + (i - 2), the one of step 0's k_1 to block (S - 1) N; the stage
// inputs s_i the weight gradient pairs them with are rebuilt by adaptive_stage_inputs_kernel (the recursion itself does
// not need them).
template <class TB, int ACT>
__global__ __launch_bounds__(FT) void fcode_adaptive_bwd_kernel(const float* __restrict__ traj,
                                                                const OdeCtrl* __restrict__ ctrl,
                                                                const float* __restrict__ gy,
                                                                const bf16_t* __restrict__ wt_hi,
                                                                const bf16_t* __restrict__ wt_lo, int b, int max_steps,
                                                                float* __restrict__ gx, float* __restrict__ GZ,
                                                                int Bp) {
    constexpr int S = TB::S, NA = BwdCoef<TB>::NA;
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * FROWS * AYRB];
    __shared__ float bc[BwdCoef<TB>::COUNT];      // this step's constants (publish_bwd_step)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int brow = blockIdx.x * FROWS + (lane & 15);
    const int nf = wave * 16 + (lane >> 4) * 4;
    const bool live = brow < b;
    const Solved solved = read_solved(ctrl, max_steps);
    const int status = solved.status, N = solved.N;
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
    f32x4 gfsal = zero4;
    for (int n = N - 1; n >= 0; --n) {
        publish_bwd_step<TB>(bc, ctrl, n, N, tid);
        f32x4 gk[S];
#pragma unroll
        for (int j = 0; j < S; ++j) gk[j] = uniform_f(bc[NA + j]) * a;
        gk[S - 1] += gfsal;
#pragma unroll
        for (int i = S - 1; i >= 1; --i) {
            const f32x4 gz = gk[i] * dact_out<ACT>(ld(n, 1 + i));
            emit((S - 1) * n + (i - 1), gz);
            const f32x4 gs = times_w(gz);
            a += gs;
#pragma unroll
            for (int j = 0; j < i; ++j) gk[j] += uniform_f(bc[i * (i - 1) / 2 + j]) * gs;
        }
        gfsal = gk[0];
        if (n == 0) {
            const f32x4 gz = gfsal * dact_out<ACT>(ld(0, 1));
            emit((S - 1) * N, gz);
            a += times_w(gz);
        }
    }
    if (N == 0) emit(0, zero4);
    if (live) *(f32x4*)(gx + (size_t)brow * AD + nf) = a;
}

// SI[(S - 1) n + i - 1] = y_n + dt_n sum_{j < i} A[i][j] k_{j+1} (i = 1 .. S - 1: the inputs of stages 2 .. S of accepted
// step n), SI[(S - 1) N] = y_0.  blockIdx.y = n; one thread per (row, four features); rows beyond b are zero like their gz.
// D = the width (256 or 384): the three kernels below are the same code at either, in the same fixed order; they walk
// the (S - 1) N + 1 row blocks of the Tableau TB's S stages.
template <int D, class TB>
__global__ __launch_bounds__(256) void adaptive_stage_inputs_kernel(const float* __restrict__ traj,
                                                                    const OdeCtrl* __restrict__ ctrl, int b, int max_steps,
                                                                    float* __restrict__ SI, int Bp) {
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
    auto st = [&](int blk, const f32x4& v) { *(f32x4*)(SI + ((size_t)blk * Bp + brow) * D + nf) = v; };
    constexpr int S = TB::S;
    if (n == 0) {
        const float qnan = __builtin_nanf("");
        st((S - 1) * N, status != 0 && live ? f32x4{qnan, qnan, qnan, qnan} : ld(0));
    }
    if (n >= N) return;
    const double dt = ctrl->dt[n];
    const f32x4 y = ld(0);
    f32x4 k[S - 1];
#pragma unroll
    for (int j = 0; j < S - 1; ++j) k[j] = ld(1 + j);
#pragma unroll
    for (int i = 1; i <= S - 1; ++i) {
        f32x4 s = y;
#pragma unroll
        for (int j = 0; j < i; ++j) s += (float)(dt * TB::A(i, j)) * k[j];
        st((S - 1) * n + i - 1, s);
    }
}

// C[D][D] = sum_r A[r][m] * B[r][n] over the R = ((S - 1) N + 1) Bp rows the state kernel wrote, N read from the control
// block (gemm_tn_f32_kernel of fusion_bwd.hip with a device-side row count; same tile shape, same fixed order).
template <int D, class TB>
__global__ __launch_bounds__(256) void adaptive_gw_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          float* __restrict__ C, const OdeCtrl* __restrict__ ctrl,
                                                          int max_steps, int Bp) {
    __shared__ float as[16][64 + 4], bs[16][64 + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    int N = ctrl->status != 0 ? 0 : ctrl->accepted;
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const int R = ((TB::S - 1) * N + 1) * Bp;      // a multiple of 16
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
template <int D, class TB>
__global__ __launch_bounds__(256) void adaptive_gb_kernel(const float* __restrict__ A, float* __restrict__ out,
                                                          const OdeCtrl* __restrict__ ctrl, int max_steps, int Bp) {
    __shared__ float redf[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    int N = ctrl->status != 0 ? 0 : ctrl->accepted;
    N = N < 0 ? 0 : (N > max_steps ? max_steps : N);
    const int R = ((TB::S - 1) * N + 1) * Bp;
    float s = 0.f;
    for (int r = w; r < R; r += 4) s += A[(size_t)r * D + c];
    redf[w][lane] = s;
    __syncthreads();
    if (w == 0) out[c] = ((redf[0][lane] + redf[1][lane]) + redf[2][lane]) + redf[3][lane];
}

// The backward at 384 columns: the recursion of fcode_adaptive_bwd_kernel, one workgroup (8 waves) per 16 rows, W^T's `hi`
// fragments resident and its `lo` fragments streamed, the adjoint product on two planes and three products as there.  A lane
// owns twelve features of its row, so the S stage adjoints gk_j (dopri5: 84 registers beside W's 144) do not stay in registers:
// they wait in the first S row blocks of SI, the half of the workspace adaptive_stage_inputs_kernel fills AFTER this
// kernel -- this workgroup's rows only, every lane re-reading only what it wrote itself, so no fence.  gk_1 of a step (the
// FSAL adjoint the step before adds to its gk_S) is read from its block before that step overwrites it.
template <class TB, int ACT>
__global__ __launch_bounds__(XT) void fcode_adaptive_wide_bwd_kernel(const float* __restrict__ traj,
                                                                     const OdeCtrl* __restrict__ ctrl,
                                                                     const float* __restrict__ gy,
                                                                     const bf16x8* __restrict__ wtf_hi,
                                                                     const bf16x8* __restrict__ wtf_lo, int b, int max_steps,
                                                                     float* __restrict__ gx, float* __restrict__ GZ,
                                                                     float* SI, int Bp) {
    constexpr int S = TB::S, NA = BwdCoef<TB>::NA;
    __shared__ __attribute__((aligned(16))) char smem[XPLANES_BWD];
    __shared__ float bc[BwdCoef<TB>::COUNT];      // this step's constants (publish_bwd_step)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int brow = blockIdx.x * FROWS + (lane & 15);
    const int nf = wave * (16 * XTILES) + (lane >> 4) * 4;
    const bool live = brow < b;
    const Solved solved = read_solved(ctrl, max_steps);
    const int status = solved.status, N = solved.N;
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
    auto gkp = [&](int j, int t) -> float* { return SI + ((size_t)j * Bp * XD + rbase) + lo + 16 * t; };

    Tiles3 a;
#pragma unroll
    for (int t = 0; t < XTILES; ++t) a.t[t] = live ? *(const f32x4*)(gy + rbase + loff + 16 * t) : zero4;
    for (int n = N - 1; n >= 0; --n) {
        publish_bwd_step<TB>(bc, ctrl, n, N, tid);
#pragma unroll
        for (int i = S - 1; i >= 1; --i) {
            asm volatile("" : "+v"(lo), "+v"(lk));
            // gz_{i+1} = gk_{i+1} act'(k_{i+1}); stage S's gk is dt w_S a plus the FSAL adjoint of the step after
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
                f32x4 gk;
                if (i == S - 1) {
                    gk = uniform_f(bc[NA + S - 1]) * a.t[t];
                    if (n != N - 1) gk += *(const f32x4*)gkp(0, t);
                } else {
                    gk = *(const f32x4*)gkp(i, t);
                }
                const f32x4 gz = sel(gk * dact_out<ACT>(ld(n, 1 + i, t)));
                emit((S - 1) * n + (i - 1), t, gz);
                put(t, gz);
                __builtin_amdgcn_sched_barrier(0);      // one feature tile at a time
            }
            const Tiles3 gs = times_w();
#pragma unroll
            for (int t = 0; t < XTILES; ++t) {
#pragma unroll
                for (int j = 0; j < i; ++j) {
                    const f32x4 base = i == S - 1 ? uniform_f(bc[NA + j]) * a.t[t] : *(const f32x4*)gkp(j, t);
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
                emit((S - 1) * N, t, gz);
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

// ---- host side: the entries without a width argument are the 256-column ones, the _wide entries take d and serve 384

static int64_t ring_floats(int b, int d, int max_steps, int want_traj) {
    if (b <= 0 || max_steps < 1) return 0;
    return (int64_t)(want_traj ? max_steps + 1 : 2) * 8 * b * d;
}
static int64_t bwd_workspace_bytes(int b, int d, int max_steps) {
    if (b <= 0 || max_steps < 1) return 0;
    const int64_t Bp = (b + FROWS - 1) / FROWS * FROWS;
    return 2 * (6 * (int64_t)max_steps + 1) * Bp * d * sizeof(float);
}

// the refusals of the four launch entries, in their order: a bad argument (have: every required pointer is there;
// tols_ok: the forward's tolerances), then a width d the entry is not built for
static int adaptive_refusal(bool have, int b, int d, int built_for, int act, int method, int max_steps, bool tols_ok) {
    if (!have || d <= 0 || b <= 0 || (method != Dopri5::METHOD && method != Bosh3::METHOD) || act < AGP_ACT_ID || act > AGP_ACT_SIGMOID || max_steps < 1 ||
        max_steps > AGP_ODE_MAX_STEPS_LIMIT)
        return AGP_E_BADARG;
    if (!tols_ok) return AGP_E_BADARG;
    return d != built_for ? AGP_E_UNSUPPORTED : AGP_OK;
}

// fn(std::integral_constant<int, ACT>{}) for a checked activation: one kernel instantiation each
template <class F>
static int by_act(int act, F&& fn) {
    switch (act) {
        case AGP_ACT_ID: return fn(std::integral_constant<int, AGP_ACT_ID>{});
        case AGP_ACT_RELU: return fn(std::integral_constant<int, AGP_ACT_RELU>{});
        case AGP_ACT_TANH: return fn(std::integral_constant<int, AGP_ACT_TANH>{});
        default: return fn(std::integral_constant<int, AGP_ACT_SIGMOID>{});
    }
}

// fn(TB{}) for a checked adaptive method's Tableau
template <class F>
static int by_method(int method, F&& fn) {
    return method == Bosh3::METHOD ? fn(Bosh3{}) : fn(Dopri5{});
}

template <class E>
static int adaptive_fwd(const float* x, const float* add1, const float* add2, const void* w_hi, const void* w_lo,
                        const float* bias, int b, int d, int act, int method, double rtol, double atol, int max_steps, float* y,
                        float* ring, int want_traj, void* ctrl, void* stream) {
    const bool tols_ok = rtol >= 0. && atol >= 0. && rtol + atol > 0.;
    if (const int rc = adaptive_refusal(x && w_hi && w_lo && y && ring && ctrl, b, d, E::D, act, method, max_steps, tols_ok)) return rc;
    static_assert(sizeof(agp_ode_stats) == 32 && offsetof(OdeCtrl, dt) == 32, "control block layout");
    const int nring = want_traj ? max_steps + 1 : 2;
    return by_method(method, [&](auto M) -> int {
        return by_act(act, [&](auto A) -> int {
            const auto kernel = fcode_adaptive_kernel<E, decltype(M), decltype(A)::value>;
            if constexpr (E::LDS_DYNAMIC != 0) {
                static std::atomic<uint64_t> attr_done;      // (one per instantiation of this lambda: per method and activation)
                if (!agp_lds_attr((const void*)kernel, E::LDS_DYNAMIC, attr_done)) return AGP_E_LAUNCH;
            }
            AGP_LAUNCH(kernel, dim3(1), dim3(E::THREADS), E::LDS_DYNAMIC, (hipStream_t)stream, x, add1, add2,
                       (typename E::Plane)w_hi, (typename E::Plane)w_lo, bias, b, rtol, atol, max_steps, ring, nring, y,
                       (OdeCtrl*)ctrl);
            AGP_CHECK_LAUNCH();
            return AGP_OK;
        });
    });
}

// the weight and bias gradients from the gz rows the state kernel left in GZ and the stage inputs rebuilt into S
template <int D, class TB>
static int adaptive_sums(const float* traj, const OdeCtrl* c, int b, int max_steps, float* gw, float* gb, float* GZ, float* S,
                         int Bp, hipStream_t s) {
    if (gw) {
        AGP_LAUNCH((adaptive_stage_inputs_kernel<D, TB>), dim3(Bp * (D / 4) / 256, max_steps), dim3(256), 0, s, traj, c, b, max_steps, S, Bp);
        AGP_CHECK_LAUNCH();
        AGP_LAUNCH((adaptive_gw_kernel<D, TB>), dim3(D / 64, D / 64), dim3(256), 0, s, GZ, S, gw, c, max_steps, Bp);
        AGP_CHECK_LAUNCH();
    }
    if (gb) {
        AGP_LAUNCH((adaptive_gb_kernel<D, TB>), dim3(D / 64), dim3(256), 0, s, GZ, gb, c, max_steps, Bp);
        AGP_CHECK_LAUNCH();
    }
    return AGP_OK;
}

template <int D>
static int adaptive_bwd(const float* traj, const void* ctrl, const float* gy, const void* wt_hi, const void* wt_lo, int b, int d,
                        int act, int method, int max_steps, float* gx, float* gw, float* gb, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    if (const int rc = adaptive_refusal(traj && ctrl && gy && wt_hi && wt_lo && gx && workspace, b, d, D, act, method, max_steps, true))
        return rc;
    if (workspace_bytes < bwd_workspace_bytes(b, D, max_steps)) return AGP_E_BADARG;
    const int Bp = (b + FROWS - 1) / FROWS * FROWS;
    float* GZ = (float*)workspace;
    // (the state kernel's scratch first, then the stage inputs; the halves are sized for seven stages, the most a Tableau has)
    float* S = GZ + (6 * (size_t)max_steps + 1) * Bp * D;
    hipStream_t s = (hipStream_t)stream;
    const OdeCtrl* c = (const OdeCtrl*)ctrl;
    const dim3 grid(Bp / FROWS);
    return by_method(method, [&](auto M) -> int {
        using TB = decltype(M);
        const int rc = by_act(act, [&](auto A) -> int {
            constexpr int ACT = decltype(A)::value;
            if constexpr (D == AD) {
                AGP_LAUNCH((fcode_adaptive_bwd_kernel<TB, ACT>), grid, dim3(FT), 0, s, traj, c, gy, (const bf16_t*)wt_hi,
                           (const bf16_t*)wt_lo, b, max_steps, gx, GZ, Bp);
            } else {
                AGP_LAUNCH((fcode_adaptive_wide_bwd_kernel<TB, ACT>), grid, dim3(XT), 0, s, traj, c, gy, (const bf16x8*)wt_hi,
                           (const bf16x8*)wt_lo, b, max_steps, gx, GZ, S, Bp);
            }
            AGP_CHECK_LAUNCH();
            return AGP_OK;
        });
        return rc != AGP_OK ? rc : adaptive_sums<D, TB>(traj, c, b, max_steps, gw, gb, GZ, S, Bp, s);
    });
}

extern "C" int64_t agp_fcode_adaptive_ctrl_bytes(int max_steps) {
    return max_steps < 1 ? 0 : (int64_t)sizeof(agp_ode_stats) + 3 * (int64_t)max_steps * sizeof(double);
}

extern "C" int64_t agp_fcode_adaptive_ring_floats(int b, int max_steps, int want_traj) {
    return ring_floats(b, AD, max_steps, want_traj);
}

extern "C" int agp_fcode_adaptive_fwd(const float* x, const float* add1, const float* add2, const void* w_hi,
                                      const void* w_lo, const float* bias, int b, int act, int method, double rtol,
                                      double atol, int max_steps, float* y, float* ring, int want_traj, void* ctrl,
                                      void* stream) {
    return adaptive_fwd<Resident256>(x, add1, add2, w_hi, w_lo, bias, b, AD, act, method, rtol, atol, max_steps, y, ring, want_traj,
                                     ctrl, stream);
}

extern "C" int64_t agp_fcode_adaptive_bwd_workspace_bytes(int b, int max_steps) { return bwd_workspace_bytes(b, AD, max_steps); }

extern "C" int agp_fcode_adaptive_bwd(const float* traj, const void* ctrl, const float* gy, const void* wt_hi,
                                      const void* wt_lo, int b, int act, int method, int max_steps, float* gx, float* gw,
                                      float* gb, void* workspace, int64_t workspace_bytes, void* stream) {
    return adaptive_bwd<AD>(traj, ctrl, gy, wt_hi, wt_lo, b, AD, act, method, max_steps, gx, gw, gb, workspace, workspace_bytes, stream);
}

extern "C" int64_t agp_fcode_adaptive_wide_ring_floats(int b, int d, int max_steps, int want_traj) {
    return d != XD ? 0 : ring_floats(b, d, max_steps, want_traj);
}

extern "C" int agp_fcode_adaptive_wide_fwd(const float* x, const float* add1, const float* add2, const void* wf_hi,
                                           const void* wf_lo, const float* bias, int b, int d, int act, int method,
                                           double rtol, double atol, int max_steps, float* y, float* ring, int want_traj,
                                           void* ctrl, void* stream) {
    return adaptive_fwd<Streamed384>(x, add1, add2, wf_hi, wf_lo, bias, b, d, act, method, rtol, atol, max_steps, y, ring, want_traj,
                                     ctrl, stream);
}

extern "C" int64_t agp_fcode_adaptive_wide_bwd_workspace_bytes(int b, int d, int max_steps) {
    return d != XD ? 0 : bwd_workspace_bytes(b, d, max_steps);
}

extern "C" int agp_fcode_adaptive_wide_bwd(const float* traj, const void* ctrl, const float* gy, const void* wtf_hi,
                                           const void* wtf_lo, int b, int d, int act, int method, int max_steps, float* gx,
                                           float* gw, float* gb, void* workspace, int64_t workspace_bytes, void* stream) {
    return adaptive_bwd<XD>(traj, ctrl, gy, wtf_hi, wtf_lo, b, d, act, method, max_steps, gx, gw, gb, workspace, workspace_bytes,
                            stream);
}
