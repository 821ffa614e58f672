// Batched triplet mining: the reference builds one faiss index per query
// (8000 per cache refresh, datasets/datasets_ws_nuscenes.py:1241-1258).  The hardest negatives
// are one agp_knn_search over the sampled database rows (host: agplace_amd/mining.py); this file
// holds the best-positive search over RAGGED per-query candidate lists, and the exact top-k over a per-query candidate TABLE
// (agp_mine_topk_listed) that the `full` mining mode needs: every query searches its own sample (:1295-1322).
#include "common.hpp"

namespace agp_mining {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per query: exact fp64 squared distances from the fp32 vectors, first minimum in list
// order (faiss keeps the earlier of two equal distances)
__global__ void best_positive_kernel(const float* __restrict__ xq, int64_t nq, const float* __restrict__ xb, int64_t nb,
                                     int d, const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
                                     int64_t* __restrict__ out_best, float* __restrict__ out_dist) {
    const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (q >= nq) return;
    const float* qv = xq + q * d;
    double best = 1.0e300;
    int64_t best_i = -1;
    for (int64_t j = off[q]; j < off[q + 1]; ++j) {
        const int64_t r = idx[j];
        double s = 0.0;
        if (r >= 0 && r < nb) {
            const float* dv = xb + r * d;
            for (int k = lane; k < d; k += 64) {
                const double t = (double)qv[k] - (double)dv[k];
                s += t * t;
            }
            s = wave_sum_f64(s);
        } else {
            s = 1.0e300;
        }
        if (s < best) { best = s; best_i = r; }
    }
    if (lane == 0) {
        out_best[q] = best_i;
        if (out_dist) out_dist[q] = best_i >= 0 ? (float)best : 3.4028234663852886e38f;
    }
}

// ---- agp_mine_topk_listed: the k nearest DISTINCT database rows out of a per-query candidate table
//
// One 256-thread workgroup per query, three phases over LDS images of the query's row of the table:
//   1. validity, one column per thread: s_row[c] = the database row, or -1 for an entry outside [0, nb) or (from column
//      exempt_cols on) one found in the query's ascending exclusion list by a binary search of fixed length;
//   2. distances, one column per group of 16 lanes (16 columns per step): exact fp64 squared distance from the fp32 vectors,
//      each lane summing elements l, l + 16, ... in order, then a fixed butterfly over the 16 lanes.  The same database row gives
//      the same bits wherever it is listed;
//   3. k rounds of "the smallest (distance, row) pair strictly greater than the pair taken last": a lexicographic minimum over
//      the LDS image, per thread, per wave (shuffles), across the four waves (one LDS slot per wave, two sets used in turn so
//      that one barrier per round suffices).  Strictly greater is what drops a row listed twice, and the order on pairs is total
//      over distinct rows, so the result does not depend on the order of the columns.
// The order: a squared distance is never negative, so the bit pattern of a finite one orders as an unsigned integer; every
// non-finite one (+inf, NaN) has bits >= those of +inf and is clamped to them: behind every finite distance, by row among
// themselves.  Every loop's trip count follows from ncols, d, k and the length of the exclusion list.
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_SCRATCH = 128;                                   // bytes behind the two images: [2][4] bits, [2][4] rows
constexpr unsigned long long TOPK_INF = 0x7FF0000000000000ull;
constexpr long long TOPK_NONE = 0x7FFFFFFFFFFFFFFFll;               // no valid row: valid ones lie below nb

__device__ __forceinline__ bool pair_less(unsigned long long ab, long long ar, unsigned long long bb, long long br) {
    const unsigned long long ka = ab < TOPK_INF ? ab : TOPK_INF, kb = bb < TOPK_INF ? bb : TOPK_INF;
    return ka < kb || (ka == kb && ar < br);
}

// is `v` in the ascending list a[lo .. hi), hi > lo?  `steps` = the bit length of hi - lo: the halving below needs no more
__device__ __forceinline__ bool listed_in_steps(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int steps, int64_t v) {
    int64_t base = lo, n = hi - lo;
    for (int s = 0; s < steps; ++s) {
        if (n > 1) {                                                // the last entry <= v, if there is one, stays in [base, base + n)
            const int64_t half = n >> 1;
            if (a[base + half] <= v) base += half;
            n -= half;
        }
    }
    return a[base] == v;
}

__global__ void __launch_bounds__(TOPK_THREADS)
topk_listed_kernel(const float* __restrict__ xq, const float* __restrict__ xb, int64_t nb, int d, const int64_t* __restrict__ cand,
                   int ncols, const int64_t* __restrict__ row_of_q, const int64_t* __restrict__ excl_off,
                   const int64_t* __restrict__ excl_idx, int exempt_cols, int k, int64_t* __restrict__ out_idx,
                   float* __restrict__ out_dist, int32_t* __restrict__ filled) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* s_bits = (unsigned long long*)smem;                                  // [ncols] distance bits
    long long* s_row = (long long*)(smem + (size_t)ncols * 8);                               // [ncols] database row, -1 = none
    unsigned long long* s_wbits = (unsigned long long*)(smem + (size_t)ncols * 16);          // [2][4] the waves' minima
    long long* s_wrow = (long long*)(smem + (size_t)ncols * 16 + 64);                        // [2][4]
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;

    int64_t lo = 0, hi = 0;
    if (row_of_q) {
        const int64_t er = row_of_q[q];
        lo = excl_off[er];
        hi = excl_off[er + 1];
    }
    const int steps = hi > lo ? 64 - __builtin_clzll((unsigned long long)(hi - lo)) : 0;
    const int64_t* crow = cand + q * ncols;
    for (int c = tid; c < ncols; c += TOPK_THREADS) {
        const int64_t r = crow[c];
        bool ok = r >= 0 && r < nb;
        if (ok && steps && c >= exempt_cols) ok = !listed_in_steps(excl_idx, lo, hi, steps, r);
        s_row[c] = ok ? r : -1;
    }
    __syncthreads();

    const int g = tid >> 4, l = tid & 15;
    const float* qv = xq + q * d;
    for (int c0 = 0; c0 < ncols; c0 += TOPK_THREADS / 16) {
        const int c = c0 + g;
        const int64_t r = c < ncols ? s_row[c] : -1;
        double s = 0.0;
        if (r >= 0) {
            const float* dv = xb + r * d;
            for (int j = l; j < d; j += 16) {
                const double t = (double)qv[j] - (double)dv[j];
                s += t * t;
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        if (l == 0 && c < ncols) s_bits[c] = (unsigned long long)__double_as_longlong(s);
    }
    __syncthreads();

    const int lane = tid & 63, w = tid >> 6;
    unsigned long long last_b = 0;
    long long last_r = -1;                                          // below every valid pair
    int found = 0;
    for (int i = 0; i < k; ++i) {
        unsigned long long bb = ~0ull;
        long long br = TOPK_NONE;                                   // above every valid pair
        for (int c = tid; c < ncols; c += TOPK_THREADS) {
            const long long r = s_row[c];
            const unsigned long long b = s_bits[c];
            if (r >= 0 && pair_less(last_b, last_r, b, r) && pair_less(b, r, bb, br)) {
                bb = b;
                br = r;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_xor(bb, o, 64);
            const long long orow = __shfl_xor(br, o, 64);
            if (pair_less(ob, orow, bb, br)) {
                bb = ob;
                br = orow;
            }
        }
        const int set = (i & 1) * 4;
        if (lane == 0) {
            s_wbits[set + w] = bb;
            s_wrow[set + w] = br;
        }
        __syncthreads();
        bb = s_wbits[set];
        br = s_wrow[set];
#pragma unroll
        for (int j = 1; j < TOPK_THREADS / 64; ++j) {
            const unsigned long long ob = s_wbits[set + j];
            const long long orow = s_wrow[set + j];
            if (pair_less(ob, orow, bb, br)) {
                bb = ob;
                br = orow;
            }
        }
        const bool got = br != TOPK_NONE;
        if (tid == 0) {
            out_idx[q * k + i] = got ? (int64_t)br : -1;
            if (out_dist) out_dist[q * k + i] = got ? (float)__longlong_as_double((long long)bb) : 3.4028234663852886e38f;
        }
        if (got) {                                                  // once a round finds nothing, so do the ones after it
            last_b = bb;
            last_r = br;
            ++found;
        }
    }
    if (tid == 0) filled[q] = found;
}

}  // namespace agp_mining

extern "C" int agp_mine_topk_listed(const float* xq, int64_t nq, const float* xb, int64_t nb, int d, const int64_t* cand, int ncols,
                                    const int64_t* row_of_q, const int64_t* excl_off, const int64_t* excl_idx, int exempt_cols, int k,
                                    int64_t* out_idx, float* out_dist, int32_t* filled, void* stream) {
    const int given = (row_of_q != nullptr) + (excl_off != nullptr) + (excl_idx != nullptr);
    if (!xq || !cand || !out_idx || !filled || (!xb && nb > 0) || nq < 0 || nq > 2147483647ll - 64 || nb < 0 || d <= 0 || k < 1 ||
        k > AGP_MINE_MAX_K || ncols < 1 || ncols > AGP_MINE_MAX_COLS || exempt_cols < 0 || (given != 0 && given != 3))
        return AGP_E_BADARG;
    if (nq == 0) return AGP_OK;
    static std::atomic<uint64_t> attr_done{0};
    if (!agp_lds_attr((const void*)agp_mining::topk_listed_kernel, AGP_MINE_MAX_COLS * 16 + agp_mining::TOPK_SCRATCH, attr_done))
        return AGP_E_LAUNCH;
    const unsigned lds = (unsigned)ncols * 16u + agp_mining::TOPK_SCRATCH;
    AGP_LAUNCH(agp_mining::topk_listed_kernel, dim3((unsigned)nq), dim3(agp_mining::TOPK_THREADS), lds, (hipStream_t)stream, xq, xb,
               nb, d, cand, ncols, row_of_q, excl_off, excl_idx, exempt_cols, k, out_idx, out_dist, filled);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_mine_best_positive(const float* xq, int64_t nq, const float* xb, int64_t nb, int d,
                                      const int64_t* pos_off, const int64_t* pos_idx, int64_t* out_best, float* out_dist,
                                      void* stream) {
    if (!xq || !xb || !pos_off || !out_best || nq < 0 || d <= 0) return AGP_E_BADARG;
    if (nq == 0) return AGP_OK;
    const int64_t blocks = (nq * 64 + 255) / 256;
    AGP_LAUNCH(agp_mining::best_positive_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xq, nq, xb, nb, d,
               pos_off, pos_idx, out_best, out_dist);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}
