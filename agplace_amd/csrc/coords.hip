// Coordinate manager of the sparse-voxel branch on the device, WITHOUT host synchronisation (the part of
// MinkowskiEngine's CoordinateManager the path uses: reference network_mm/mm.py:86-87 `ME.SparseTensor(features,
// coordinates)`, models/minkfpn.py:53 stride-2 convolutions; semantics restated in agplace_amd/sparse/coords.py).
//
// Capacity mode: a level of `cap` rows (cap = the number of INPUT points, an upper bound for every level) holds
//   keys[cap]      sorted unique int64 keys (batch, x, y, z: 16-bit biased fields), rows >= n padded with SENT
//   seg_off[B+1]   first row of every batch sample; seg_off[B] = n, the number of valid rows -- the device-side count every
//                  row-wise kernel of the branch reads instead of a host integer (no .item(), no torch.unique)
//   bidx[cap]      batch index of a row
//
// Round 4: the batch index is the top key field, so a level is B independent sorts of a few thousand keys.  ONE workgroup
// sorts one sample's keys in LDS (bitonic network over <= 16384 eight-byte keys = 128 KB of the CU's 160 KB), removes the
// duplicates and counts; a second kernel places the samples behind each other.  A coarser level = 2 launches, the input level
// = 5 (+ 2 memsets) -- rounds 2-3 ran rocPRIM's device-wide radix sort per level: ~27 launches of ~5 us each, 130 launches
// per forward, most of them 1024-thread grids that queued behind the image network's convolutions when two steps were in
// flight.  No library primitive is left in this file.
//   input level  : keys + per-sample histogram (wave-aggregated atomics) -> exclusive scan -> scatter into per-sample buckets
//                  (the order inside a bucket is whatever the atomics gave: the sort below makes it irrelevant) -> sort
//                  (x, y, z | bucket slot) per sample, duplicates of a voxel merged in INPUT-ROW order (mean of their
//                  features: deterministic whatever the bucket order was) -> placement
//   coarser level: sort (key & mask) per sample of the finer level's rows -> placement
// A sample of more than 16384 rows is sorted by the same network in global memory (slow, correct); a sample of more than
// 65536 input points does not fit the 16-bit slot field: its build is FLAGGED (bit 1 of the range flag) like an out-of-range
// coordinate.  All launches go to the caller's stream, temporary storage is the caller's workspace: hipGraph-capturable.
#include <cstring>

#include "common.hpp"

namespace agp_coords {

constexpr int64_t SENT = 0x7fffffffffffffffLL;          // padding key: sorts after every real key
constexpr uint64_t USENT = ~0ull;                        // padding inside the sort (unsigned compare)
constexpr int BITS = 16, OFF = 1 << 15;
constexpr int ST = 1024;                                 // threads of a segment workgroup
constexpr int LDS_KEYS = 16384;                          // keys a workgroup sorts in LDS
constexpr int MAX_SLOT = 65536;                          // input points of one sample (16-bit bucket slot beside the 48-bit voxel)
constexpr int CUR_STRIDE = 32;                           // (builds from points) int32 words between two samples' bucket cursors: one 128-byte line each

// coords [n][4] (batch, x, y, z) as int64 (kind 0), float32 (kind 1) or float64 (kind 2; floored like ME does for floating
// coordinates) -> key (input order) + the per-sample histogram.  Out-of-range coordinates (|c| >= 32512: kernel offsets need
// headroom) send their point to the sample's origin voxel, a batch index outside [0, nbatch) is clamped; both are flagged; the flag word describes THIS build (agp_sparse_build
// zeroes it first).  A workgroup owns PB consecutive points; clouds arrive sample after sample, so nearly every workgroup sees
// ONE batch index and adds its whole count with one atomic (same-address atomics serialise in L2: one per wave cost 48 us
// for 64 x 8000 points, one per point would cost milliseconds).
constexpr int PB = 1024;
__global__ void __launch_bounds__(256) keys_hist_kernel(const void* __restrict__ coords, int kind, int64_t n, int nbatch,
                                                        int64_t* __restrict__ keys, int32_t* __restrict__ hist, int32_t* __restrict__ flag) {
    const int64_t base = (int64_t)blockIdx.x * PB;
    const int b_first = [&] {
        int64_t c0;
        if (kind == 0) c0 = ((const int64_t*)coords)[base * 4];
        else if (kind == 1) c0 = (int64_t)floorf(((const float*)coords)[base * 4]);
        else c0 = (int64_t)floor(((const double*)coords)[base * 4]);
        return (int)(c0 < 0 ? 0 : (c0 >= nbatch ? nbatch - 1 : c0));
    }();
    int bs[PB / 256];
    bool uniform = true;
#pragma unroll
    for (int u = 0; u < PB / 256; ++u) {
        const int64_t i = base + u * 256 + threadIdx.x;
        bs[u] = -1;
        if (i >= n) continue;
        int64_t c[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (kind == 0) c[a] = ((const int64_t*)coords)[i * 4 + a];
            else if (kind == 1) c[a] = (int64_t)floorf(((const float*)coords)[i * 4 + a]);
            else c[a] = (int64_t)floor(((const double*)coords)[i * 4 + a]);
        }
        // (a batch index >= nbatch would index the per-sample tables of the segment kernels out of bounds: clamped and flagged too)
        bool bad = c[0] < 0 || c[0] >= nbatch;
        bool far = false;
#pragma unroll
        for (int a = 1; a < 4; ++a) far = far || c[a] > OFF - 257 || c[a] < -(OFF - 257);
        if (far) {
            // a point outside the key range joins the ORIGIN voxel of its sample (the sensor position, inside every LiDAR sweep) --
            // not a voxel at the edge of the range: the build is flagged either way, and an isolated voxel tens of thousands of
            // cells from the cloud is exactly the input the flag exists to keep out of the kernels behind it
            c[1] = c[2] = c[3] = 0;
            bad = true;
        }
        if (c[0] < 0) c[0] = 0;
        if (c[0] >= nbatch) c[0] = nbatch - 1;
        if (bad) atomicOr(flag, 1);
        int64_t k = c[0];
#pragma unroll
        for (int a = 1; a < 4; ++a) k = (k << BITS) | (c[a] + OFF);
        keys[i] = k;
        bs[u] = (int)c[0];
        uniform = uniform && bs[u] == b_first;
    }
    if (__syncthreads_and(uniform ? 1 : 0)) {
        if (threadIdx.x == 0) atomicAdd(&hist[b_first], (int)(n - base < PB ? n - base : PB));
    } else {
        // a block that straddles samples: one atomic per distinct batch index of a wave (a same-address atomic per POINT cost 0.3 us each)
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int u = 0; u < PB / 256; ++u) {
            uint64_t todo = __builtin_amdgcn_ballot_w64(bs[u] >= 0);
            while (todo) {
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const int b0 = __shfl(bs[u], leader, 64);
                const uint64_t same = __builtin_amdgcn_ballot_w64(bs[u] == b0);
                if (lane == leader) atomicAdd(&hist[b0], __popcll(same));
                todo &= ~same;
            }
        }
    }
}

// block-wide exclusive scan of one int per thread (ST threads); returns the exclusive prefix, *total = block sum
__device__ __forceinline__ int block_excl_scan(int v, int* total) {
    __shared__ int wsum[ST / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < ST / 64; ++w) {
        if (w < wave) base += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// one workgroup: pseg = exclusive scan of the histogram (pseg[B] = n), cursor = its copy (the scatter's running positions)
__global__ void __launch_bounds__(ST) scan_hist_kernel(const int32_t* __restrict__ hist, int nbatch, int64_t* __restrict__ pseg,
                                                       int32_t* __restrict__ cursor) {
    __shared__ int carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nbatch; b0 += ST) {
        const int b = b0 + threadIdx.x;
        const int v = b < nbatch ? hist[b] : 0;
        int tot;
        const int ex = block_excl_scan(v, &tot);
        const int carry = carry_s;
        if (b < nbatch) { pseg[b] = carry + ex; cursor[b] = carry + ex; }
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) pseg[nbatch] = carry_s;
}

// points -> their sample's bucket: bkeys / brow [pseg[b], pseg[b+1]).  The same workgroups of PB points: one atomic claims the
// whole block's range when it holds one sample (its points keep their input order and the stores coalesce).
__global__ void __launch_bounds__(256) scatter_kernel(const int64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ cursor,
                                                      int64_t* __restrict__ bkeys, int32_t* __restrict__ brow) {
    __shared__ int s_base;
    const int64_t base = (int64_t)blockIdx.x * PB;
    const int b_first = (int)(keys[base] >> (3 * BITS));
    int64_t ks[PB / 256];
    bool uniform = true;
#pragma unroll
    for (int u = 0; u < PB / 256; ++u) {
        const int64_t i = base + u * 256 + threadIdx.x;
        ks[u] = i < n ? keys[i] : -1;
        uniform = uniform && (i >= n || (int)(ks[u] >> (3 * BITS)) == b_first);
    }
    if (__syncthreads_and(uniform ? 1 : 0)) {
        if (threadIdx.x == 0) s_base = atomicAdd(&cursor[b_first], (int)(n - base < PB ? n - base : PB));
        __syncthreads();
        const int pb = s_base;
#pragma unroll
        for (int u = 0; u < PB / 256; ++u) {
            const int64_t i = base + u * 256 + threadIdx.x;
            if (i < n) { bkeys[pb + (i - base)] = ks[u]; brow[pb + (i - base)] = (int32_t)i; }
        }
    } else {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int u = 0; u < PB / 256; ++u) {
            const int64_t i = base + u * 256 + threadIdx.x;
            const int b = i < n ? (int)(ks[u] >> (3 * BITS)) : -1;
            uint64_t todo = __builtin_amdgcn_ballot_w64(b >= 0);
            while (todo) {
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const int b0 = __shfl(b, leader, 64);
                const uint64_t same = __builtin_amdgcn_ballot_w64(b == b0);
                int pb = 0;
                if (lane == leader) pb = atomicAdd(&cursor[b0], __popcll(same));
                pb = __shfl(pb, leader, 64);
                if (b == b0) {
                    const int pos = pb + __popcll(same & ((1ull << lane) - 1ull));
                    bkeys[pos] = ks[u];
                    brow[pos] = (int32_t)i;
                }
                todo &= ~same;
            }
        }
    }
}

// the key array of a sort: in LDS one key of padding follows every 32 (a thread's chunk of C consecutive keys starts C * 8 bytes
// after its neighbour's: 16 lanes on one bank pair without it), in global memory plain
template <bool PAD>
struct KeyArr {
    uint64_t* p;
    __device__ __forceinline__ uint64_t& operator[](int i) const { return p[PAD ? i + (i >> 5) : i]; }
};

// ascending bitonic network over s[0, P) (P a power of two), all ST threads of the workgroup.  A pass moves every key through
// LDS once (8192 keys x 91 passes = 12 MB: the kernel is bound by that, not by its barriers), so the passes whose partner
// distance fits a thread's own C = P / ST consecutive keys run in registers: one load + store per size k instead of log2(C).
template <int C, class PTR>
__device__ __forceinline__ void bitonic_sort_c(PTR s, int P) {
    const int tid = threadIdx.x;
    uint64_t e[C];
    static_assert(C <= 32, "a thread's chunk lies inside one padding group");
    auto local = [&](int k_lo, int k_hi) {          // every pass with j < C of the sizes k_lo .. k_hi (k_hi <= C: whole sizes)
#pragma unroll
        for (int r = 0; r < C; ++r) e[r] = s[tid * C + r];
        for (int k = k_lo; k <= k_hi; k <<= 1) {
#pragma unroll
            for (int j = C >> 1; j > 0; j >>= 1) {
                if (j >= k) continue;
#pragma unroll
                for (int r = 0; r < C; ++r) {
                    if (r & j) continue;
                    const bool up = ((tid * C + r) & k) == 0;
                    const uint64_t a = e[r], b = e[r | j];
                    if ((a > b) == up) { e[r] = b; e[r | j] = a; }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < C; ++r) s[tid * C + r] = e[r];
        __syncthreads();
    };
    if (C > 1) local(2, C);
    for (int k = 2 * C; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= C; j >>= 1) {
            uint64_t a[(C + 1) / 2], b[(C + 1) / 2];
#pragma unroll
            for (int u = 0; u < (C + 1) / 2; ++u) {
                const int t = tid + u * ST;
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                a[u] = s[i]; b[u] = s[i | j];
            }
#pragma unroll
            for (int u = 0; u < (C + 1) / 2; ++u) {
                const int t = tid + u * ST;
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool up = (i & k) == 0;
                if ((a[u] > b[u]) == up) { s[i] = b[u]; s[i | j] = a[u]; }
            }
            __syncthreads();
        }
        if (C > 1) local(k, k);
    }
}

template <class PTR>
__device__ __forceinline__ void bitonic_sort(PTR s, int P) {
    const int tid = threadIdx.x;
    if (P == 16 * ST) return bitonic_sort_c<16>(s, P);
    if (P == 8 * ST) return bitonic_sort_c<8>(s, P);
    if (P == 4 * ST) return bitonic_sort_c<4>(s, P);
    if (P == 2 * ST) return bitonic_sort_c<2>(s, P);
    for (int k = 2; k <= P; k <<= 1)                  // a small sample (P <= ST) or a huge one in global memory
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += ST) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = s[i], b = s[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
}

// One workgroup per batch sample: sort the sample's keys, drop the duplicates, count.
//   L0 = false: in = the finer level's keys, rows [seg[b], seg[b+1]); the sorted value is key & mask
//   L0 = true : in = bkeys (bucket order), the sorted value is (x, y, z) << 16 | bucket slot; the duplicates of a voxel are merged
//               in input-row order: f_tmp = mean of their feature rows
// unique keys -> uniq_tmp[seg[b] ...), their count -> cnt[b]
template <bool L0, class PTR>
__device__ __forceinline__ void seg_sort_body(PTR s, const int64_t* __restrict__ in, int64_t r0, int n, int P, int64_t mask, int b,
                                              const int32_t* __restrict__ brow, const float* __restrict__ f, int cf,
                                              int64_t* __restrict__ uniq_tmp, float* __restrict__ f_tmp, int32_t* __restrict__ cnt) {
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += ST) {
        uint64_t v = USENT;
        if (i < n) {
            const uint64_t k = (uint64_t)in[r0 + i];
            v = L0 ? (((k & 0xffffffffffffull) << 16) | (uint64_t)i) : (k & (uint64_t)mask);
        }
        s[i] = v;
    }
    __syncthreads();
    bitonic_sort(s, P);
    const int per = (P + ST - 1) / ST, i0 = tid * per;
    auto vox = [&](int i) -> uint64_t { const uint64_t v = s[i]; return L0 ? (v >> 16) : v; };
    int c = 0;
    for (int u = 0; u < per; ++u) {
        const int i = i0 + u;
        if (i < n && (i == 0 || vox(i) != vox(i - 1))) ++c;
    }
    int tot;
    int pos = block_excl_scan(c, &tot);
    for (int u = 0; u < per; ++u) {
        const int i = i0 + u;
        if (!(i < n && (i == 0 || vox(i) != vox(i - 1)))) continue;
        const uint64_t v = vox(i);
        uniq_tmp[r0 + pos] = L0 ? (int64_t)(((uint64_t)b << (3 * BITS)) | v) : (int64_t)v;
        if (L0 && f_tmp) {
            int e = i + 1;
            while (e < n && vox(e) == v) ++e;
            if (e == i + 1) {
                const int row = brow[r0 + (int)(s[i] & 0xffffull)];
                for (int ch = 0; ch < cf; ++ch) f_tmp[(size_t)(r0 + pos) * cf + ch] = f[(size_t)row * cf + ch];
            } else {
                // the voxel's points in ascending input row (a handful: selection by repeated minimum), summed in that order
                const float dup = (float)(e - i);
                for (int ch = 0; ch < cf; ++ch) {
                    float sum = 0.f;
                    int last = -1;
                    for (int t = i; t < e; ++t) {
                        int m = 0x7fffffff;
                        for (int jj = i; jj < e; ++jj) {
                            const int row = brow[r0 + (int)(s[jj] & 0xffffull)];
                            if (row > last && row < m) m = row;
                        }
                        sum += f[(size_t)m * cf + ch];
                        last = m;
                    }
                    f_tmp[(size_t)(r0 + pos) * cf + ch] = sum / dup;
                }
            }
        }
        ++pos;
    }
    if (tid == 0) cnt[b] = tot;
}

template <bool L0>
__global__ void __launch_bounds__(ST) seg_sort_kernel(const int64_t* __restrict__ in, const int64_t* __restrict__ seg, int64_t mask,
                                                      const int32_t* __restrict__ brow, const float* __restrict__ f, int cf,
                                                      int64_t* __restrict__ uniq_tmp, float* __restrict__ f_tmp, int32_t* __restrict__ cnt,
                                                      uint64_t* __restrict__ gscr, int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sk[];
    const int b = blockIdx.x;
    const int64_t r0 = seg[b];
    const int64_t nn = seg[b + 1] - r0;
    if (nn <= 0) { if (threadIdx.x == 0) cnt[b] = 0; return; }
    if (L0 && nn > MAX_SLOT) {          // (uniform) the slot field cannot number this sample's points: empty sample, flagged
        if (threadIdx.x == 0) { cnt[b] = 0; atomicOr(flag, 2); }
        return;
    }
    const int n = (int)nn;
    int P = 2;
    while (P < n) P <<= 1;
    if (n <= LDS_KEYS) seg_sort_body<L0>(KeyArr<true>{sk}, in, r0, n, P, mask, b, brow, f, cf, uniq_tmp, f_tmp, cnt);
    else seg_sort_body<L0>(KeyArr<false>{gscr + 2 * r0}, in, r0, n, P, mask, b, brow, f, cf, uniq_tmp, f_tmp, cnt);     // P < 2 n: inside [2 r0, 2 r1)
}

// placement: sample b's unique keys go to rows [off_b, off_b + cnt[b]) with off = exclusive scan of cnt; batch indices, segment
// offsets (seg_off[B] = n), padding of rows >= n; optional feature rows.  CHK = false (agp_sparse_build, agp_sparse_coarsen,
// agp_sparse_build_points): sum(cnt) <= cap holds by construction and rows are written unchecked.  CHK = true (the level-capacity
// build from points): `cap` is the caller's bound, so the total is compared with it BEFORE any row is written -- a build whose
// overflow word is set, or whose total exceeds cap, places nothing: every sample empty, all cap rows padding, bit 2 of the flag.
template <bool CHK>
__device__ __forceinline__ void place_body(const int64_t* __restrict__ uniq_tmp, const float* __restrict__ f_tmp, int cf,
                                           const int64_t* __restrict__ seg_in, const int32_t* __restrict__ cnt, int nbatch,
                                           int64_t cap, int64_t* __restrict__ keys_out, float* __restrict__ f_out,
                                           int64_t* __restrict__ seg_off, int32_t* __restrict__ bidx, const int32_t* __restrict__ ovf,
                                           const int32_t* __restrict__ inserts, int32_t* __restrict__ flag) {
    __shared__ int64_t red[CHK ? 3 : 2][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t pre = 0, all = 0, ins = 0;
    for (int a = tid; a < nbatch; a += 256) {
        const int c = cnt[a];
        all += c;
        if (a < b) pre += c;
        if (CHK) ins += inserts[(size_t)a * CUR_STRIDE];     // (the counter beside sample a's bucket cursor)
    }
    red[0][tid] = pre; red[1][tid] = all;
    if (CHK) red[2][tid] = ins;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o];
            if (CHK) red[2][tid] += red[2][tid + o];
        }
        __syncthreads();
    }
    int64_t off = red[0][0], tot = red[1][0];
    const int64_t r0 = seg_in[b];
    int c = cnt[b];
    if (CHK && (*ovf != 0 || red[2][0] > cap || tot > cap)) {                  // (uniform over the grid: every workgroup reads the same words)
        if (b == 0 && tid == 0) atomicOr(flag, 4);
        off = 0; tot = 0; c = 0;
    }
    for (int j = tid; j < c; j += 256) {
        keys_out[off + j] = uniq_tmp[r0 + j];
        bidx[off + j] = b;
        if (f_out)
            for (int ch = 0; ch < cf; ++ch) f_out[(size_t)(off + j) * cf + ch] = f_tmp[(size_t)(r0 + j) * cf + ch];
    }
    if (tid == 0) {
        seg_off[b] = off;
        if (b == nbatch - 1) seg_off[nbatch] = tot;
    }
    const int64_t lo = cap * b / nbatch, hi = cap * (b + 1) / nbatch;
    for (int64_t i = (lo > tot ? lo : tot) + tid; i < hi; i += 256) { keys_out[i] = SENT; bidx[i] = 0; }
}

__global__ void __launch_bounds__(256) place_kernel(const int64_t* __restrict__ uniq_tmp, const float* __restrict__ f_tmp, int cf,
                                                    const int64_t* __restrict__ seg_in, const int32_t* __restrict__ cnt, int nbatch,
                                                    int64_t cap, int64_t* __restrict__ keys_out, float* __restrict__ f_out,
                                                    int64_t* __restrict__ seg_off, int32_t* __restrict__ bidx) {
    place_body<false>(uniq_tmp, f_tmp, cf, seg_in, cnt, nbatch, cap, keys_out, f_out, seg_off, bidx, nullptr, nullptr, nullptr);
}

// Row order for the gather-GEMM: inside every batch sample, rows grouped by z-plane (stable: (x, y) order inside a plane).  Rows
// sort (x, y, z) with z FASTEST, so a 128-row tile of the natural order holds every z-plane of its columns and therefore needs
// every tap; a tile of ONE plane at the bottom (top) of the sample has no dz = -1 (+1) neighbour at all, and the gather-GEMM's
// per-tile tap list drops those 9 of 27 taps.  A coarse LiDAR level is 1-3 voxels thick: a third of its MFMAs.
// One workgroup per sample: z values present -> LDS bitmap -> ascending list (<= 64 planes, else the identity order) -> per plane
// one block scan over the threads' row chunks (samples of more than 16384 rows keep the natural order).  perm[m] = the output row
// GEMM row m computes; identity past the valid rows.
__global__ void __launch_bounds__(ST) zplane_perm_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ seg_off, int nbatch,
                                                         int64_t cap, int32_t* __restrict__ perm) {
    __shared__ uint32_t bm[2048];
    __shared__ int zs[64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t r0 = seg_off[b], n_total = seg_off[nbatch];
    const int n = (int)(seg_off[b + 1] - r0);
    {
        const int64_t lo = cap * b / nbatch, hi = cap * (b + 1) / nbatch;
        for (int64_t i = (lo > n_total ? lo : n_total) + tid; i < hi; i += ST) perm[i] = (int32_t)i;
    }
    if (n <= 0) return;
    bm[tid] = 0u; bm[tid + ST] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += ST) {
        const uint32_t z = (uint32_t)(keys[r0 + i] & 0xffff);
        atomicOr(&bm[z >> 5], 1u << (z & 31));
    }
    __syncthreads();
    const uint32_t w0 = bm[2 * tid], w1 = bm[2 * tid + 1];
    int tot;
    int pos = block_excl_scan(__popc(w0) + __popc(w1), &tot);
    if (tot > 64) {                                         // (uniform) too many planes to be worth grouping
        for (int i = tid; i < n; i += ST) perm[r0 + i] = (int32_t)(r0 + i);
        return;
    }
    for (uint32_t m = w0; m; m &= m - 1) zs[pos++] = 64 * tid + __builtin_ctz(m);
    for (uint32_t m = w1; m; m &= m - 1) zs[pos++] = 64 * tid + 32 + __builtin_ctz(m);
    __syncthreads();
    // a thread's rows' z values stay in registers over the plane loop (<= 16 rows per thread; a larger sample keeps its natural order)
    constexpr int ZR = LDS_KEYS / ST;
    const int per = (n + ST - 1) / ST, i0 = tid * per;
    if (per > ZR) {
        for (int i = tid; i < n; i += ST) perm[r0 + i] = (int32_t)(r0 + i);
        return;
    }
    int zv[ZR];
#pragma unroll
    for (int u = 0; u < ZR; ++u) zv[u] = (u < per && i0 + u < n) ? (int)(keys[r0 + i0 + u] & 0xffff) : -1;
    int base = 0;
    for (int pl = 0; pl < tot; ++pl) {
        const int zp = zs[pl];
        int c = 0;
#pragma unroll
        for (int u = 0; u < ZR; ++u) c += zv[u] == zp ? 1 : 0;
        int total;
        int at = base + block_excl_scan(c, &total);
#pragma unroll
        for (int u = 0; u < ZR; ++u)
            if (zv[u] == zp) perm[r0 + at++] = (int32_t)(r0 + i0 + u);
        base += total;
    }
}

inline int64_t al(int64_t v) { return (v + 255) / 256 * 256; }
struct Ws { int64_t keys, bkeys, brow, uniq, ftmp, gscr, hist, pseg, cursor, cnt, total; };
inline Ws layout(int64_t cap, int nbatch, int cf) {
    Ws w;
    w.keys = 0;
    w.bkeys = al(w.keys + cap * 8);
    w.brow = al(w.bkeys + cap * 8);
    w.uniq = al(w.brow + cap * 4);
    w.ftmp = al(w.uniq + cap * 8);
    w.gscr = al(w.ftmp + cap * 4 * (int64_t)(cf > 0 ? cf : 0));
    w.hist = al(w.gscr + 2 * cap * 8);
    w.pseg = al(w.hist + (int64_t)nbatch * 4);
    w.cursor = al(w.pseg + (int64_t)(nbatch + 1) * 8);
    w.cnt = al(w.cursor + (int64_t)nbatch * 4);
    w.total = al(w.cnt + (int64_t)nbatch * 4);
    return w;
}
inline dim3 grid_rows(int64_t n) { return dim3((unsigned)((n + PB - 1) / PB)); }

template <bool L0>
static int launch_seg_sort(const int64_t* in, const int64_t* seg, int64_t mask, const int32_t* brow, const float* f, int cf,
                           int64_t* uniq, float* ftmp, int32_t* cnt, uint64_t* gscr, int32_t* flag, int nbatch, hipStream_t s) {
    constexpr int lds = (LDS_KEYS + LDS_KEYS / 32) * 8;
    static std::atomic<uint64_t> attr_done{0};
    if (!agp_lds_attr((const void*)seg_sort_kernel<L0>, lds, attr_done)) return AGP_E_LAUNCH;
    AGP_LAUNCH(seg_sort_kernel<L0>, dim3(nbatch), dim3(ST), lds, s, in, seg, mask, brow, f, cf, uniq, ftmp, cnt, gscr, flag);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

__global__ void zero_words_kernel(int32_t* flag, int32_t* hist, int nbatch) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *flag = 0;
    if (i < nbatch) hist[i] = 0;
}

}  // namespace agp_coords
using namespace agp_coords;

extern "C" int64_t agp_sparse_coords_workspace_bytes(int64_t cap, int nbatch, int cfeat) {
    if (cap < 1) cap = 1;
    if (nbatch < 1) nbatch = 1;
    return layout(cap, nbatch, cfeat).total;
}

extern "C" int agp_sparse_build(const void* coords, int kind, int64_t n, const float* feats, int cfeat, int nbatch, int64_t* keys,
                                float* feats_out, int64_t* seg_off, int32_t* bidx, int32_t* range_flag, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    if (!coords || !keys || !seg_off || !bidx || !range_flag || !workspace || n <= 0 || n >= (1ll << 30) || nbatch <= 0 ||
        nbatch >= 0x7fff || kind < 0 || kind > 2 || (feats && (!feats_out || cfeat <= 0)))
        return AGP_E_BADARG;
    const int cf = feats ? cfeat : 0;
    const Ws w = layout(n, nbatch, cf);
    if (workspace_bytes < w.total) return AGP_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* hist = (int32_t*)(ws + w.hist);
    // the flag of THIS build, not of an earlier one; the histogram.  A KERNEL, not hipMemsetAsync: this entry point is captured into
    // hipGraphs (MM.forward_q from coords), and a captured memset node of ROCm 7.2 is not safe beside eager memsets issued between
    // replays -- found in round 6: after an eager 4-byte memset of another buffer the replayed graph's memset node left 0x01010101
    // in a word it had no business with (or faulted on a wild address) in every run; the same graph with this kernel: clean
    // (profiles/README.md, round 6).  No library entry point that may be captured issues a memset any more.
    AGP_LAUNCH(zero_words_kernel, dim3((nbatch + 255) / 256), dim3(256), 0, s, range_flag, hist, nbatch);
    AGP_CHECK_LAUNCH();
    AGP_LAUNCH(keys_hist_kernel, grid_rows(n), dim3(256), 0, s, coords, kind, n, nbatch, (int64_t*)(ws + w.keys), hist, range_flag);
    AGP_CHECK_LAUNCH();
    AGP_LAUNCH(scan_hist_kernel, dim3(1), dim3(ST), 0, s, hist, nbatch, (int64_t*)(ws + w.pseg), (int32_t*)(ws + w.cursor));
    AGP_CHECK_LAUNCH();
    AGP_LAUNCH(scatter_kernel, grid_rows(n), dim3(256), 0, s, (const int64_t*)(ws + w.keys), n, (int32_t*)(ws + w.cursor),
               (int64_t*)(ws + w.bkeys), (int32_t*)(ws + w.brow));
    AGP_CHECK_LAUNCH();
    const int rc = launch_seg_sort<true>((const int64_t*)(ws + w.bkeys), (const int64_t*)(ws + w.pseg), 0, (const int32_t*)(ws + w.brow),
                                         feats, cf, (int64_t*)(ws + w.uniq), cf ? (float*)(ws + w.ftmp) : nullptr,
                                         (int32_t*)(ws + w.cnt), (uint64_t*)(ws + w.gscr), range_flag, nbatch, s);
    if (rc != AGP_OK) return rc;
    AGP_LAUNCH(place_kernel, dim3(nbatch), dim3(256), 0, s, (const int64_t*)(ws + w.uniq), cf ? (const float*)(ws + w.ftmp) : nullptr,
               cf, (const int64_t*)(ws + w.pseg), (const int32_t*)(ws + w.cnt), nbatch, n, keys, cf ? feats_out : nullptr, seg_off, bidx);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_sparse_coarsen(const int64_t* keys, const int64_t* seg_off_in, int64_t cap, int stride, int nbatch,
                                  int64_t* keys_out, int64_t* seg_off, int32_t* bidx, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    if (!keys || !seg_off_in || !keys_out || !seg_off || !bidx || !workspace || cap <= 0 || cap >= (1ll << 30) || nbatch <= 0 ||
        nbatch >= 0x7fff || stride < 1 || stride > 4096 || (stride & (stride - 1)))
        return AGP_E_BADARG;
    const Ws w = layout(cap, nbatch, 0);
    if (workspace_bytes < w.total) return AGP_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int64_t low = 2 * stride - 1;
    const int64_t mask = ~((low << (2 * BITS)) | (low << BITS) | low);     // floor(c / 2s) * 2s per axis on 2^15-biased fields
    const int rc = launch_seg_sort<false>(keys, seg_off_in, mask, nullptr, nullptr, 0, (int64_t*)(ws + w.uniq), nullptr,
                                          (int32_t*)(ws + w.cnt), (uint64_t*)(ws + w.gscr), nullptr, nbatch, s);
    if (rc != AGP_OK) return rc;
    AGP_LAUNCH(place_kernel, dim3(nbatch), dim3(256), 0, s, (const int64_t*)(ws + w.uniq), (const float*)nullptr, 0, seg_off_in,
               (const int32_t*)(ws + w.cnt), nbatch, cap, keys_out, (float*)nullptr, seg_off, bidx);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int agp_sparse_zplane_perm(const int64_t* keys, const int64_t* seg_off, int nbatch, int64_t cap, int32_t* perm, void* stream) {
    if (!keys || !seg_off || !perm || nbatch <= 0 || cap <= 0 || cap >= (1ll << 31)) return AGP_E_BADARG;
    AGP_LAUNCH(zplane_perm_kernel, dim3(nbatch), dim3(ST), 0, (hipStream_t)stream, keys, seg_off, nbatch, cap, perm);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Level 0 from RAW lidar points (the reference's host chain: ME.utils.sparse_quantize per scan in __getitem__,
// batched_coordinates + PCRandomRotation in the collate function, then ME.SparseTensor's floor + merge; specification in
// DESIGN.md section 1c).  A raw scan has 35 k - 120 k points that fall into a few thousand voxels, so the points are deduplicated
// BEFORE anything is sorted: one pass quantises every row and inserts (sample, qx, qy, qz) into an open-addressing table of the
// workspace (64-bit keys, 64-bit atomicCAS, linear probing, >= 2 slots per input row); only the thread whose insert succeeded
// goes on -- it rotates its voxel, forms the final key and appends it to its sample's bucket.  A sample's bucket is the row range
// its points occupy in the input ([off[b], off[b+1]): never too small), so no histogram and no scan precede the append: 4 launches
// (clear, voxelise, per-sample sort, placement; the last two are the bodies of the coarser-level build above on whole keys).
// The features of the level are all ones (reference: feats = torch.ones([n, 1])), the mean of merged ones is 1: nothing is
// gathered.  The table is cleared by a kernel, never by a memset node (see agp_sparse_build).
namespace agp_coords {

constexpr uint64_t HEMPTY = ~0ull;                       // an empty table slot: no key (sample < 0x7fff) equals it

__device__ __forceinline__ uint64_t hash_mix64(uint64_t k) {          // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

// slots of the table for `nvalid` rows inside the offsets: a power of two >= 2 nvalid (>= 64), never more than the workspace holds
__device__ __forceinline__ uint64_t table_slots(int64_t nvalid, uint64_t tsize_max) {
    uint64_t t = 64;
    while (t < 2 * (uint64_t)nvalid && t < tsize_max) t <<= 1;
    return t;
}

// The level-capacity build (agp_sparse_build_points_cap): the level has `lcap` rows, an upper bound the CALLER gives for the
// number of voxels of the whole batch, independent of the `cap` point rows.  Two words of the workspace carry its state:
//   total  a LOWER bound of the keys that entered the table so far: every sample counts its inserts beside its bucket cursor
//          (cursor[b * CUR_STRIDE + 1], one atomic per workgroup) and passes them on in quanta of lcap / (2 nbatch), so total
//          lags the truth by less than lcap / 2
//   ovf    != 0 once the build is KNOWN to overflow: an insert found no slot, or total passed lcap
// The table in use has table_slots(min(rows inside the offsets, lcap)) slots.  If no insert fails, total ends at A = the number of
// If no insert fails and no thread saw ovf, the per-sample counters sum to A = the number of distinct (sample, quantised voxel)
// cells; A <= lcap keeps the load <= 1/2, so no insert fails, total <= A never passes lcap and ovf stays 0.  ovf is only ever set
// when more than lcap keys exist (total is a lower bound; a failed insert means a full table).  The placement therefore decides
// "ovf != 0 or sum of the counters > lcap", which is A > lcap: a function of the input alone.  ovf rises by 1.5 lcap inserts at
// the latest (load 3/4: probes still short); what threads do once they SEE it (drop their row unprobed) only saves work.
__device__ __forceinline__ int64_t level_rows(int64_t nvalid, int64_t lcap) { return nvalid < lcap ? nvalid : lcap; }

// table (the slots in use) <- empty, cursors <- 0, flag <- 0, features of the rows inside the offsets <- 1, poff <- the caller's
// offsets clamped into [0, cap].  CAP: the table and the features follow the level capacity lcap, total and ovf <- 0.
template <bool CAP>
__device__ __forceinline__ void points_init_body(const int64_t* __restrict__ off, int nbatch, int64_t cap, int64_t lcap, uint64_t tsize,
                                                 uint64_t* __restrict__ table, int64_t* __restrict__ poff, int32_t* __restrict__ cursor,
                                                 int32_t* __restrict__ flag, float* __restrict__ feats_out, int32_t* __restrict__ total,
                                                 int32_t* __restrict__ ovf) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x, gsz = (uint64_t)gridDim.x * 256;
    typedef __attribute__((ext_vector_type(2))) unsigned long long u64x2;
    const u64x2 e2 = {HEMPTY, HEMPTY};
    const int64_t o_end = off[nbatch];
    const int64_t nvalid = o_end < 0 ? 0 : (o_end > cap ? cap : o_end);        // = poff[nbatch]; valid rows of the level <= nvalid
    const int64_t nrows = CAP ? level_rows(nvalid, lcap) : nvalid;
    const uint64_t tuse = table_slots(nrows, tsize);
    for (uint64_t i = gid; i < tuse / 2; i += gsz) ((u64x2*)table)[i] = e2;
    for (uint64_t i = gid; i < (uint64_t)nrows; i += gsz) feats_out[i] = 1.f;
    for (uint64_t i = gid; i <= (uint64_t)nbatch; i += gsz) {
        const int64_t o = off[i];
        poff[i] = o < 0 ? 0 : (o > cap ? cap : o);
        if (i < (uint64_t)nbatch) {
            cursor[i * CUR_STRIDE] = 0;
            if (CAP) cursor[i * CUR_STRIDE + 1] = 0;
        }
    }
    if (gid == 0) {
        *flag = 0;
        if (CAP) { *total = 0; *ovf = 0; }
    }
}

__global__ void __launch_bounds__(256) points_init_kernel(const int64_t* __restrict__ off, int nbatch, int64_t cap, uint64_t tsize,
                                                          uint64_t* __restrict__ table, int64_t* __restrict__ poff,
                                                          int32_t* __restrict__ cursor, int32_t* __restrict__ flag,
                                                          float* __restrict__ feats_out) {
    points_init_body<false>(off, nbatch, cap, 0, tsize, table, poff, cursor, flag, feats_out, nullptr, nullptr);
}

__global__ void __launch_bounds__(256) points_init_cap_kernel(const int64_t* __restrict__ off, int nbatch, int64_t cap, int64_t lcap,
                                                              uint64_t tsize, uint64_t* __restrict__ table, int64_t* __restrict__ poff,
                                                              int32_t* __restrict__ cursor, int32_t* __restrict__ flag,
                                                              float* __restrict__ feats_out, int32_t* __restrict__ total,
                                                              int32_t* __restrict__ ovf) {
    points_init_body<true>(off, nbatch, cap, lcap, tsize, table, poff, cursor, flag, feats_out, total, ovf);
}

// One thread per input row.  Row i belongs to the sample b with poff[b] <= i < poff[b+1]; rows outside [poff[0], poff[nbatch]) are
// not looked at (the tail of a fixed-capacity buffer).  Dropped and flagged (bit 0): a row with a non-finite component, with
// |q| >= 32512 on an axis, or whose ROTATED voxel leaves that range.  The quotient is the correctly rounded fp32 one: the library
// is compiled without -ffast-math and hipcc's default keeps fp32 division correctly rounded (v_div_scale / v_div_fmas /
// v_div_fixup), __fdiv_rn says so and stays right if OCML's rounded operations are ever switched on.  The rotation is row vector
// x matrix in fp64, (qx R0j + qy R1j) + qz R2j: |q| < 2^15 times an fp32 value is exact in fp64, so the floored result is
// defined bit for bit.  The hash table in use has table_slots(poff[nbatch]) slots: a short scan in a large buffer clears and
// probes a table of its own size.
// CAP (level capacity lcap, words total / ovf: see above): the table has table_slots(min(poff[nbatch], lcap)) slots, so a probe
// sequence may find NO slot -- the loop is bounded by the table size either way, and a thread that runs it out sets ovf.  A thread
// that sees ovf set (before its first probe, and every 64 probes) drops its row; its finite / range test still raises bit 0.
template <bool CAP>
__device__ __forceinline__ void points_voxelize_body(const float* __restrict__ pts, const int64_t* __restrict__ poff, int nbatch,
                                                     float quant, const float* __restrict__ rot, int rot_per_sample,
                                                     uint64_t* __restrict__ table, uint64_t tsize, int32_t* __restrict__ cursor,
                                                     int64_t* __restrict__ bkeys, int32_t* __restrict__ flag, int64_t lcap,
                                                     int64_t quantum, int32_t* __restrict__ total, int32_t* __restrict__ ovf) {
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t base = (int64_t)blockIdx.x * ST, i = base + tid;
    const int64_t n_end = poff[nbatch];
    if (base >= n_end) return;                              // (uniform) a block of tail rows
    const uint64_t tmask = table_slots(CAP ? level_rows(n_end, lcap) : n_end, tsize) - 1;
    auto overflowed = [&] { return CAP && __hip_atomic_load(ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; };
    auto sample_of = [&](int64_t r) {                       // the last b in [0, nbatch) with poff[b] <= r (0 if there is none)
        int lo = 0, hi = nbatch;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (poff[mid] <= r) lo = mid; else hi = mid;
        }
        return lo;
    };
    const int b_first = sample_of(base);
    int b = -1;
    bool win = false, bad = false, ins = false;
    uint64_t key = 0;
    if (i < n_end) {
        const int bb = i < poff[b_first + 1] ? b_first : sample_of(i);
        if (poff[bb] <= i && i < poff[bb + 1]) b = bb;      // (offsets that do not ascend own no rows: nothing is written for them)
    }
    if (b >= 0) {
        float qf[3];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p = pts[i * 3 + a];
            qf[a] = floorf(__fdiv_rn(p, quant));
            ok = ok && __builtin_isfinite(p) && fabsf(qf[a]) < (float)(OFF - 256);
        }
        if (!ok) {
            bad = true;
        } else if (!overflowed()) {
            const int q0 = (int)qf[0], q1 = (int)qf[1], q2 = (int)qf[2];
            const uint64_t hk = ((uint64_t)b << (3 * BITS)) | ((uint64_t)(q0 + OFF) << (2 * BITS)) | ((uint64_t)(q1 + OFF) << BITS) |
                                (uint64_t)(q2 + OFF);
            uint64_t h = hash_mix64(hk) & tmask;
            // a voxel already in the table costs a load, not an atomic: 70 000 points of one voxel do one CAS per wave that sees
            // the slot empty, then read.  The table holds at most tsize / 2 keys, so a probe sequence always meets an empty slot.
            bool settled = false;                           // (CAP) the key is in the table, or the row was dropped on seeing ovf
            for (uint64_t step = 0; step <= tmask; ++step) {
                if (CAP && (step & 63) == 63 && overflowed()) { settled = true; break; }
                const uint64_t cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == hk) { settled = true; break; }
                if (cur == HEMPTY) {
                    const uint64_t prev = atomicCAS((unsigned long long*)&table[h], (unsigned long long)HEMPTY, (unsigned long long)hk);
                    if (prev == HEMPTY) { win = true; settled = true; break; }
                    if (prev == hk) { settled = true; break; }
                }
                h = (h + 1) & tmask;
            }
            if (CAP && !settled) atomicOr(ovf, 1);           // every slot holds another key: more than lcap keys
            ins = win;
            key = hk;
            if (win && rot) {
                const float* R = rot + (rot_per_sample ? (size_t)b * 9 : 0);
                uint64_t k = (uint64_t)b;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double c = floor(__dadd_rn(__dadd_rn(__dmul_rn((double)q0, (double)R[j]), __dmul_rn((double)q1, (double)R[3 + j])),
                                                     __dmul_rn((double)q2, (double)R[6 + j])));
                    if (!(fabs(c) < (double)(OFF - 256))) { bad = true; win = false; }
                    k = (k << BITS) | (uint64_t)((bad ? 0 : (int)c) + OFF);
                }
                key = k;
            }
        }
    }
    {
        const uint64_t anybad = __builtin_amdgcn_ballot_w64(bad);
        if (anybad && lane == __builtin_ctzll(anybad)) atomicOr(flag, 1);
    }
    if (CAP) {
        // the keys this workgroup put into the table (counted before the rotation drops any) join the insert counter beside its
        // first sample's cursor (same 128-byte line; only the SUM over the samples is used, so a workgroup that straddles samples
        // may book all of them there).  One counter for the whole batch would serialise a returning atomic per workgroup in L2 --
        // measured: +0.06 ms at 7500 workgroups -- so only the whole quanta a counter crosses go on to the global total.
        const int nins = __syncthreads_count(ins ? 1 : 0);
        if (tid == 0 && nins) {
            const int before = atomicAdd(&cursor[(size_t)b_first * CUR_STRIDE + 1], nins);
            const int64_t crossed = ((int64_t)before + nins) / quantum - (int64_t)before / quantum;
            if (crossed) {
                const int g = atomicAdd(total, (int)(crossed * quantum));
                if ((int64_t)g + crossed * quantum > lcap) atomicOr(ovf, 1);
            }
        }
    }
    // append to the sample's bucket bkeys[poff[b] + slot]: a block inside ONE sample claims its slots with one atomic
    const bool uniform = !win || b == b_first;
    if (__syncthreads_and(uniform ? 1 : 0)) {
        int tot;
        const int pos = block_excl_scan(win ? 1 : 0, &tot);
        if (tid == 0) s_base = tot ? atomicAdd(&cursor[(size_t)b_first * CUR_STRIDE], tot) : 0;
        __syncthreads();
        if (win) bkeys[poff[b_first] + s_base + pos] = (int64_t)key;
    } else {
        const int bw = win ? b : -1;
        uint64_t todo = __builtin_amdgcn_ballot_w64(bw >= 0);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int b0 = __shfl(bw, leader, 64);
            const uint64_t same = __builtin_amdgcn_ballot_w64(bw == b0);
            int pb = 0;
            if (lane == leader) pb = atomicAdd(&cursor[(size_t)b0 * CUR_STRIDE], __popcll(same));
            pb = __shfl(pb, leader, 64);
            if (bw == b0) bkeys[poff[b0] + pb + __popcll(same & ((1ull << lane) - 1ull))] = (int64_t)key;
            todo &= ~same;
        }
    }
}

__global__ void __launch_bounds__(ST) points_voxelize_kernel(const float* __restrict__ pts, const int64_t* __restrict__ poff, int nbatch,
                                                             float quant, const float* __restrict__ rot, int rot_per_sample,
                                                             uint64_t* __restrict__ table, uint64_t tsize, int32_t* __restrict__ cursor,
                                                             int64_t* __restrict__ bkeys, int32_t* __restrict__ flag) {
    points_voxelize_body<false>(pts, poff, nbatch, quant, rot, rot_per_sample, table, tsize, cursor, bkeys, flag, 0, 1, nullptr, nullptr);
}

__global__ void __launch_bounds__(ST) points_voxelize_cap_kernel(const float* __restrict__ pts, const int64_t* __restrict__ poff, int nbatch,
                                                                 float quant, const float* __restrict__ rot, int rot_per_sample,
                                                                 uint64_t* __restrict__ table, uint64_t tsize,
                                                                 int32_t* __restrict__ cursor, int64_t* __restrict__ bkeys,
                                                                 int32_t* __restrict__ flag, int64_t lcap, int64_t quantum,
                                                                 int32_t* __restrict__ total, int32_t* __restrict__ ovf) {
    points_voxelize_body<true>(pts, poff, nbatch, quant, rot, rot_per_sample, table, tsize, cursor, bkeys, flag, lcap, quantum, total, ovf);
}

// seg_sort_kernel<false> for buckets given as (first row, count): sample b's keys are bkeys[poff[b] .. + cursor[b]), sorted whole
// (mask = all ones).  More than 65536 VOXELS in one sample: empty sample, flagged (bit 1) like the input-point limit of
// agp_sparse_build -- the rows a sample may own downstream are the same.  CAP: a build that overflowed sorts nothing (the placement
// empties it); bit 1 is still reported for the buckets as they stand.
template <bool CAP>
__device__ __forceinline__ void seg_sort_points_body(uint64_t* sk, const int64_t* __restrict__ bkeys, const int64_t* __restrict__ poff,
                                                     const int32_t* __restrict__ cursor, int64_t* __restrict__ uniq_tmp,
                                                     int32_t* __restrict__ cnt, uint64_t* __restrict__ gscr, int32_t* __restrict__ flag,
                                                     const int32_t* __restrict__ ovf) {
    const int b = blockIdx.x;
    const int64_t r0 = poff[b];
    const int n = cursor[(size_t)b * CUR_STRIDE];
    if (n <= 0) { if (threadIdx.x == 0) cnt[b] = 0; return; }
    if (n > MAX_SLOT) {
        if (threadIdx.x == 0) { cnt[b] = 0; atomicOr(flag, 2); }
        return;
    }
    if (CAP && *ovf != 0) { if (threadIdx.x == 0) cnt[b] = 0; return; }          // (uniform)
    int P = 2;
    while (P < n) P <<= 1;
    if (n <= LDS_KEYS) seg_sort_body<false>(KeyArr<true>{sk}, bkeys, r0, n, P, (int64_t)-1, b, nullptr, nullptr, 0, uniq_tmp, nullptr, cnt);
    else seg_sort_body<false>(KeyArr<false>{gscr + 2 * r0}, bkeys, r0, n, P, (int64_t)-1, b, nullptr, nullptr, 0, uniq_tmp, nullptr, cnt);
}

__global__ void __launch_bounds__(ST) seg_sort_points_kernel(const int64_t* __restrict__ bkeys, const int64_t* __restrict__ poff,
                                                             const int32_t* __restrict__ cursor, int64_t* __restrict__ uniq_tmp,
                                                             int32_t* __restrict__ cnt, uint64_t* __restrict__ gscr,
                                                             int32_t* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sk[];
    seg_sort_points_body<false>(sk, bkeys, poff, cursor, uniq_tmp, cnt, gscr, flag, nullptr);
}

__global__ void __launch_bounds__(ST) seg_sort_points_cap_kernel(const int64_t* __restrict__ bkeys, const int64_t* __restrict__ poff,
                                                                 const int32_t* __restrict__ cursor, int64_t* __restrict__ uniq_tmp,
                                                                 int32_t* __restrict__ cnt, uint64_t* __restrict__ gscr,
                                                                 int32_t* __restrict__ flag, const int32_t* __restrict__ ovf) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sk[];
    seg_sort_points_body<true>(sk, bkeys, poff, cursor, uniq_tmp, cnt, gscr, flag, ovf);
}

__global__ void __launch_bounds__(256) place_cap_kernel(const int64_t* __restrict__ uniq_tmp, const int64_t* __restrict__ seg_in,
                                                        const int32_t* __restrict__ cnt, int nbatch, int64_t lcap,
                                                        int64_t* __restrict__ keys_out, int64_t* __restrict__ seg_off,
                                                        int32_t* __restrict__ bidx, const int32_t* __restrict__ ovf,
                                                        const int32_t* __restrict__ inserts, int32_t* __restrict__ flag) {
    place_body<true>(uniq_tmp, nullptr, 0, seg_in, cnt, nbatch, lcap, keys_out, nullptr, seg_off, bidx, ovf, inserts, flag);
}

// Workspace of the builds from points.  `cap` = point rows, `lcap` = rows of the level (the uncapped build: lcap = cap).  The TABLE
// follows lcap (a power of two >= 2 lcap, >= 64 slots): it is the part that is cleared and probed on every call.  The per-sample
// buckets (bkeys), the unique keys (uniq) and the scratch of the global-memory sort (gscr) stay addressed by POINT rows -- a sample's
// bucket is the row range its points occupy, which is what makes the append need no scan; they are written for winners only, so
// their size costs address space, not traffic.  total / ovf: the two state words of the capped build, a 128-byte line each.
struct PWs { int64_t table, bkeys, uniq, gscr, poff, cursor, cnt, count, ovf, total; uint64_t tsize; };
inline PWs points_layout(int64_t cap, int64_t lcap, int nbatch, bool capped) {
    PWs w;
    w.tsize = 64;
    while (w.tsize < 2 * (uint64_t)lcap) w.tsize <<= 1;
    w.table = 0;
    w.bkeys = al(w.table + (int64_t)w.tsize * 8);
    w.uniq = al(w.bkeys + cap * 8);
    w.gscr = al(w.uniq + cap * 8);
    w.poff = al(w.gscr + 2 * cap * 8);
    w.cursor = al(w.poff + (int64_t)(nbatch + 1) * 8);
    w.cnt = al(w.cursor + (int64_t)nbatch * CUR_STRIDE * 4);
    w.count = al(w.cnt + (int64_t)nbatch * 4);
    w.ovf = capped ? al(w.count + 4) : w.count;
    w.total = capped ? al(w.ovf + 4) : w.count;          // (the uncapped build has no state words: its size is what it was)
    return w;
}
inline unsigned points_init_blocks(uint64_t tsize) {
    const uint64_t blocks = (tsize / 2 + 256 * 8 - 1) / (256 * 8);
    return (unsigned)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

}  // namespace agp_coords

extern "C" int64_t agp_sparse_points_workspace_bytes(int64_t cap, int nbatch) {
    if (cap < 1) cap = 1;
    if (cap >= (1ll << 30)) cap = (1ll << 30) - 1;
    if (nbatch < 1) nbatch = 1;
    return points_layout(cap, cap, nbatch, false).total;
}

extern "C" int agp_sparse_build_points(const float* points, const int64_t* point_offsets, int64_t cap, int nbatch, float quant_size,
                                       const float* rotation, int rot_per_sample, int64_t* keys, float* feats_out, int64_t* seg_off,
                                       int32_t* bidx, int32_t* range_flag, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!points || !point_offsets || !keys || !feats_out || !seg_off || !bidx || !range_flag || !workspace || cap <= 0 ||
        cap >= (1ll << 30) || nbatch <= 0 || nbatch >= 0x7fff || !(quant_size > 0.f) || !(quant_size <= 3.4e38f) ||
        rot_per_sample < 0 || rot_per_sample > 1)
        return AGP_E_BADARG;
    const PWs w = points_layout(cap, cap, nbatch, false);
    if (workspace_bytes < w.total) return AGP_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint64_t* table = (uint64_t*)(ws + w.table);
    int64_t* poff = (int64_t*)(ws + w.poff);
    int32_t* cursor = (int32_t*)(ws + w.cursor);
    AGP_LAUNCH(points_init_kernel, dim3(points_init_blocks(w.tsize)), dim3(256), 0, s, point_offsets, nbatch, cap, w.tsize, table, poff,
               cursor, range_flag, feats_out);
    AGP_CHECK_LAUNCH();
    AGP_LAUNCH(points_voxelize_kernel, dim3((unsigned)((cap + ST - 1) / ST)), dim3(ST), 0, s, points, (const int64_t*)poff, nbatch,
               quant_size, rotation, rot_per_sample, table, w.tsize, cursor, (int64_t*)(ws + w.bkeys), range_flag);
    AGP_CHECK_LAUNCH();
    {
        constexpr int lds = (LDS_KEYS + LDS_KEYS / 32) * 8;
        static std::atomic<uint64_t> attr_done{0};
        if (!agp_lds_attr((const void*)seg_sort_points_kernel, lds, attr_done)) return AGP_E_LAUNCH;
        AGP_LAUNCH(seg_sort_points_kernel, dim3(nbatch), dim3(ST), lds, s, (const int64_t*)(ws + w.bkeys), (const int64_t*)poff,
                   (const int32_t*)cursor, (int64_t*)(ws + w.uniq), (int32_t*)(ws + w.cnt), (uint64_t*)(ws + w.gscr), range_flag);
        AGP_CHECK_LAUNCH();
    }
    AGP_LAUNCH(place_kernel, dim3(nbatch), dim3(256), 0, s, (const int64_t*)(ws + w.uniq), (const float*)nullptr, 0, (const int64_t*)poff,
               (const int32_t*)(ws + w.cnt), nbatch, cap, keys, (float*)nullptr, seg_off, bidx);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

extern "C" int64_t agp_sparse_points_cap_workspace_bytes(int64_t npoints, int64_t level_cap, int nbatch) {
    if (npoints < 1) npoints = 1;
    if (npoints >= (1ll << 30)) npoints = (1ll << 30) - 1;
    if (level_cap < 1) level_cap = 1;
    if (level_cap >= (1ll << 30)) level_cap = (1ll << 30) - 1;
    if (nbatch < 1) nbatch = 1;
    return points_layout(npoints, level_cap, nbatch, true).total;
}

// agp_sparse_build_points with a level of `level_cap` rows: the same four launches on the capped instantiations.  The init grid is
// sized by the table of level_cap (its loops stride over the features and the offsets), the voxelise grid by the point rows.
extern "C" int agp_sparse_build_points_cap(const float* points, const int64_t* point_offsets, int64_t npoints, int64_t level_cap,
                                           int nbatch, float quant_size, const float* rotation, int rot_per_sample, int64_t* keys,
                                           float* feats_out, int64_t* seg_off, int32_t* bidx, int32_t* range_flag, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    if (!points || !point_offsets || !keys || !feats_out || !seg_off || !bidx || !range_flag || !workspace || npoints <= 0 ||
        npoints >= (1ll << 30) || level_cap < 1 || level_cap >= (1ll << 30) || nbatch <= 0 || nbatch >= 0x7fff ||
        !(quant_size > 0.f) || !(quant_size <= 3.4e38f) || rot_per_sample < 0 || rot_per_sample > 1)
        return AGP_E_BADARG;
    const PWs w = points_layout(npoints, level_cap, nbatch, true);
    if (workspace_bytes < w.total) return AGP_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint64_t* table = (uint64_t*)(ws + w.table);
    int64_t* poff = (int64_t*)(ws + w.poff);
    int32_t* cursor = (int32_t*)(ws + w.cursor);
    int32_t* total = (int32_t*)(ws + w.count);
    int32_t* ovf = (int32_t*)(ws + w.ovf);
    const int64_t quantum = level_cap / (2 * (int64_t)nbatch) > 0 ? level_cap / (2 * (int64_t)nbatch) : 1;
    AGP_LAUNCH(points_init_cap_kernel, dim3(points_init_blocks(w.tsize)), dim3(256), 0, s, point_offsets, nbatch, npoints, level_cap,
               w.tsize, table, poff, cursor, range_flag, feats_out, total, ovf);
    AGP_CHECK_LAUNCH();
    AGP_LAUNCH(points_voxelize_cap_kernel, dim3((unsigned)((npoints + ST - 1) / ST)), dim3(ST), 0, s, points, (const int64_t*)poff, nbatch,
               quant_size, rotation, rot_per_sample, table, w.tsize, cursor, (int64_t*)(ws + w.bkeys), range_flag, level_cap, quantum, total, ovf);
    AGP_CHECK_LAUNCH();
    {
        constexpr int lds = (LDS_KEYS + LDS_KEYS / 32) * 8;
        static std::atomic<uint64_t> attr_done{0};
        if (!agp_lds_attr((const void*)seg_sort_points_cap_kernel, lds, attr_done)) return AGP_E_LAUNCH;
        AGP_LAUNCH(seg_sort_points_cap_kernel, dim3(nbatch), dim3(ST), lds, s, (const int64_t*)(ws + w.bkeys), (const int64_t*)poff,
                   (const int32_t*)cursor, (int64_t*)(ws + w.uniq), (int32_t*)(ws + w.cnt), (uint64_t*)(ws + w.gscr), range_flag,
                   (const int32_t*)ovf);
        AGP_CHECK_LAUNCH();
    }
    AGP_LAUNCH(place_cap_kernel, dim3(nbatch), dim3(256), 0, s, (const int64_t*)(ws + w.uniq), (const int64_t*)poff,
               (const int32_t*)(ws + w.cnt), nbatch, level_cap, keys, seg_off, bidx, (const int32_t*)ovf, (const int32_t*)cursor + 1, range_flag);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}
