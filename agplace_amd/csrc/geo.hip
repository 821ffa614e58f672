// Geographic positives on the device (agplace_amd/geo.py): the radius search that builds the per-query lists of database rows
// within r metres (reference datasets/datasets_ws_nuscenes.py:907-912, 1032-1037: sklearn radius_neighbors over 2-D UTM
// coordinates), and the two consumers of such a list kept as a CSR (offsets int64 [n + 1], indices int64, every row ASCENDING):
// the first-hit column behind recall@N (reference test.py:73-83) and the miner's "drop the soft positives" step
// (:1394-1404).  Every kernel: wave64, ONE WAVE PER QUERY ROW, four rows per 256-thread block, no atomics -- a row is written by
// its own wave in a fixed order, so two runs give the same bytes -- no allocation, no synchronisation, the caller's stream.
#include "common.hpp"

namespace agp_geo {

// THE predicate, shared by the count and the fill so that they cannot disagree: squared planar distance <= r2 in fp64, each
// operation rounded on its own (no fma: numpy's `dx*dx + dy*dy <= r*r` has none), inclusive at the boundary.  A NaN anywhere
// makes the comparison false; an infinite coordinate gives inf or NaN on the left: neither is anybody's neighbour.
__device__ __forceinline__ bool within(double qx, double qy, double bx, double by, double r2) {
#pragma clang fp contract(off)
    const double dx = qx - bx, dy = qy - by;
    const double xx = dx * dx, yy = dy * dy;
    return xx + yy <= r2;
}

__device__ __forceinline__ int lanes_below(uint64_t m, int lane) { return __builtin_popcountll(m & ((1ull << lane) - 1ull)); }

// FILL = false: counts[q] = how many database rows lie within the radius of query q.
// FILL = true : idx[offsets[q] ..) = those rows, ascending: the database is streamed 64 rows per step, the step's hits are
//               compacted in lane order (ballot + the count of hit lanes below) behind a running base.  A row never writes at or
//               past offsets[q + 1], whatever the caller's offsets say.
template <bool FILL>
__global__ void __launch_bounds__(256) radius_kernel(const double* __restrict__ q, int nq, const double* __restrict__ db, int nb,
                                                     double r2, int64_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                     int64_t* __restrict__ idx) {
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;
    const double qx = q[2 * (int64_t)row], qy = q[2 * (int64_t)row + 1];
    int64_t base = FILL ? offsets[row] : 0;
    const int64_t end = FILL ? offsets[row + 1] : 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;           // b0 <= nb - 1 < 2^31 - 1 and lane < 64: no overflow as long as nb <= 2^31 - 64 (host)
        bool hit = false;
        if (b < nb) {
            const double2 p = *(const double2*)(db + 2 * (int64_t)b);
            hit = within(qx, qy, p.x, p.y, r2);
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        if (FILL) {
            const int64_t at = base + lanes_below(m, lane);
            if (hit && at < end) idx[at] = b;
        }
        base += __builtin_popcountll(m);
    }
    if (!FILL && lane == 0) counts[row] = base;
}

// is `v` in the ascending list a[lo .. hi)?
__device__ __forceinline__ bool listed(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t x = a[mid];
        if (x == v) return true;
        if (x < v) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// first[q] = the smallest column j with pred[q][j] in row q of the CSR, k if there is none.  Columns in ascending blocks of 64,
// one binary search per lane; the first block with a hit decides.  Negative entries (faiss's -1 padding) match nothing.
__global__ void __launch_bounds__(256) first_hit_kernel(const int64_t* __restrict__ pred, int64_t nq, int k,
                                                        const int64_t* __restrict__ off, const int64_t* __restrict__ idx,
                                                        int32_t* __restrict__ first) {
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;
    const int64_t lo = off[row], hi = off[row + 1];
    int found = k;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        bool hit = false;
        if (j < k) {
            const int64_t v = pred[row * k + j];
            hit = v >= 0 && listed(idx, lo, hi, v);
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
        if (m) {
            found = j0 + __builtin_ctzll(m);
            break;
        }
    }
    if (lane == 0) first[row] = found;
}

// out[q][0 .. negs) = the first `negs` of cand[I[q][:]] whose database row is NOT in CSR row row_of_q[q], in I's order;
// filled[q] = how many were found (< negs when the k columns did not suffice; the rest of out[q] is then left unwritten).
// An entry of I outside [0, nc) (the search's -1 beyond ntotal) is no candidate.  Stops at the block that fills the row.
__global__ void __launch_bounds__(256) drop_listed_kernel(const int64_t* __restrict__ I, int64_t nq, int k,
                                                          const int64_t* __restrict__ cand, int64_t nc,
                                                          const int64_t* __restrict__ row_of_q, const int64_t* __restrict__ off,
                                                          const int64_t* __restrict__ idx, int negs, int64_t* __restrict__ out,
                                                          int32_t* __restrict__ filled) {
    const int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;
    const int64_t r = row_of_q[row];
    const int64_t lo = off[r], hi = off[r + 1];
    int base = 0;
    for (int j0 = 0; j0 < k && base < negs; j0 += 64) {
        const int j = j0 + lane;
        bool keep = false;
        int64_t dbrow = -1;
        if (j < k) {
            const int64_t p = I[row * k + j];
            if (p >= 0 && p < nc) {
                dbrow = cand[p];
                keep = !listed(idx, lo, hi, dbrow);
            }
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
        const int at = base + lanes_below(m, lane);
        if (keep && at < negs) out[row * negs + at] = dbrow;
        base += __builtin_popcountll(m);
    }
    if (lane == 0) filled[row] = base < negs ? base : negs;
}

static inline bool rows_ok(int64_t n) { return n >= 0 && n <= 2147483647ll - 64; }

}  // namespace agp_geo

extern "C" int agp_radius_count(const double* q, int64_t nq, const double* db, int64_t nb, double r2, int64_t* counts,
                                void* stream) {
    if (!q || !db || !counts || !agp_geo::rows_ok(nq) || !agp_geo::rows_ok(nb)) return AGP_E_BADARG;
    if (nq == 0 || nb == 0) return AGP_OK;
    AGP_LAUNCH(agp_geo::radius_kernel<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q, (int)nq, db,
               (int)nb, r2, counts, (const int64_t*)nullptr, (int64_t*)nullptr);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_radius_fill(const double* q, int64_t nq, const double* db, int64_t nb, double r2, const int64_t* offsets,
                               int64_t* idx, void* stream) {
    if (!q || !db || !offsets || !idx || !agp_geo::rows_ok(nq) || !agp_geo::rows_ok(nb)) return AGP_E_BADARG;
    if (nq == 0 || nb == 0) return AGP_OK;
    AGP_LAUNCH(agp_geo::radius_kernel<true>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q, (int)nq, db,
               (int)nb, r2, (int64_t*)nullptr, offsets, idx);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_recall_first_hit(const int64_t* pred, int64_t nq, int k, const int64_t* pos_off, const int64_t* pos_idx,
                                    int32_t* first, void* stream) {
    if (!pred || !pos_off || !pos_idx || !first || !agp_geo::rows_ok(nq) || k < 1 || k > AGP_KNN_MAX_K) return AGP_E_BADARG;
    if (nq == 0) return AGP_OK;
    AGP_LAUNCH(agp_geo::first_hit_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pred, nq, k, pos_off,
               pos_idx, first);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_mine_drop_listed(const int64_t* I, int64_t nq, int k, const int64_t* cand, int64_t nc, const int64_t* row_of_q,
                                    const int64_t* pos_off, const int64_t* pos_idx, int negs, int64_t* out, int32_t* filled,
                                    void* stream) {
    if (!I || !cand || !row_of_q || !pos_off || !pos_idx || !out || !filled || !agp_geo::rows_ok(nq) || nc < 0 || k < 1 ||
        k > AGP_KNN_MAX_K || negs < 1 || negs > AGP_KNN_MAX_K)
        return AGP_E_BADARG;
    if (nq == 0) return AGP_OK;
    AGP_LAUNCH(agp_geo::drop_listed_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, I, nq, k, cand, nc,
               row_of_q, pos_off, pos_idx, negs, out, filled);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}
