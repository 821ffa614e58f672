// igemm_kxrw.hip -- the WIDE form of the inference hot kernel (igemm_kxr2.hip): 3x3 / stride 1 / pad 1 convolution on fp16 maps
// with one fp16 MFMA product, for layers with cout % 128 == 0 (ResNet layers 2 and 3, the stage-2 BasicBlock): 256 x 128 tiles,
// four waves of 64 pixels x 128 channels.
//
// Same implicit GEMM over the padded-width raster, same phase pipeline (W taps through a 3-slot ring, X double-buffered, LDS-DMA
// issued two / three phases ahead, raw s_barrier + counted s_waitcnt vmcnt(N)) and the same line-layout epilogue as igemm_kxr2;
// what changes is the arithmetic per staged byte and per barrier:
//   * the X row block of a (ky, channel chunk) macro-step is staged ONCE for 128 output channels (kxr2: once per 64);
//   * a phase is 16 MFMAs per wave (kxr2: 8) on 12 LDS fragment reads (kxr2: 8): 0.75 instead of 1.0 ds_read_b128 per MFMA;
//   * 59 KB of stage + 16 KB of epilogue strips = 75 KB of LDS and ~220 VGPRs: two workgroups per CU = two waves per SIMD, each
//     with 512 MFMA cycles per phase.
// (The stride-2 entry kernel gained 18 % from the same change, igemm_s2.hip; round 3.)  POOL as in igemm_kxr2 (conv-epilogue pooling
// over image-aligned 64-row blocks).
//
// The residual comes in by LDS-DMA and takes no VGPR (the accumulators hold 128): a wave's tile row (32 pixels x 256 bytes = 8 KB =
// 8 pieces of 4 pixel lines) lands in the wave's own epilogue STRIP, from which the wave reads it in the accumulator layout, and into
// which it then writes the packed result.  Tile row 0's strips lie where nothing else lives during the last macro-step -- the X
// buffer that step does not read and the spare LDS behind the stage (KwShape::EPI_LDS) -- so its pieces are issued behind the MFMAs
// of the last macro-step's first two phases; tile row 1's strips are the other X buffer and the W ring, dead after the K loop: its
// pieces go out right after the final barrier and are waited for behind tile row 0's arithmetic.  A strip has no row pad (a DMA
// instruction lays its 64 lanes down contiguously): the 16-byte chunk index is XOR-swizzled with the pixel's low 4 bits on the
// GLOBAL side (eoff[], shared by the DMA and the output stores) and in the accumulator-layout accesses, so those stay conflict-free
// (a ds_read_b128 lane group holds 16 different pixels mod 16).  Pixels that are not stored read out of the buffer's range: zeros.
//
// vmcnt bookkeeping (per wave, issue order; NX = 5 X pieces, a W piece = 128 rows = NWP = 2 instructions per wave):
//     prologue          : X(0)[NX]  W(0,0)[2]  W(0,1)[2]
//     phase (st,0)      : W(st,2)[2]   X(st+1)[NX]
//     phase (st,1)      : W(st+1,0)[2]
//     phase (st,2)      : W(st+1,1)[2]
//   opens (st,1): W(st,1);            younger: W(st,2) X(st+1)        -> vmcnt(NX+2)
//   opens (st,2): W(st,2);            younger: X(st+1) W(st+1,0)      -> vmcnt(NX+2)
//   opens (st+1,0): W(st+1,0) X(st+1); younger: W(st+1,1)             -> vmcnt(2)
//   last macro-step L: opens (L,1): younger W(L,2) -> vmcnt(2); opens (L,2): nothing younger -> vmcnt(0).
//   last macro-step L of a tile WITH a residual (R0 = tile row 0's 8 pieces, R1 = tile row 1's, full tile only):
//     phase (L,0)       : W(L,2)[2]  R0[0..3]          phase (L,1) : R0[4..7]          after the final barrier: R1[8]
//   opens (L,1): W(L,1);  younger: W(L,2) R0[0..3]     -> vmcnt(6)
//   opens (L,2): W(L,2);  younger: R0[0..7]            -> vmcnt(8)
//   tile row 0 reads its strip: R0; younger: R1        -> vmcnt(8)   (half tile: vmcnt(0))
//   tile row 1 reads its strip: R1                     -> vmcnt(0), placed BEFORE tile row 0's stores (a store counts too)
//
// The residual COMPUTED from a second operand stream (RES = 2; the 1x1 / stride-2 downsample of a stage's first BasicBlock, whose
// map is then never stored): raster row (img, y, xq) reads pixel (img, 2 y, 2 (xq - 1)) of the stage's INPUT map (KxrwStream) and
// multiplies it with chunk-major 1x1 weights [cin2 / 32][N][32] that carry the downsample's BatchNorm scale (folded on the host,
// rounded once to fp16).  After the 3x3 K loop the accumulators are rescaled in place, acc = acc * scale[n] + shift'[n] (the
// epilogue's FMAs, moved earlier; shift' = the conv's shift + the downsample's), then nc2 = cin2 / 32 TRAILING phases T(0..nc2-1)
// follow, each one X2 block (rows + 0 only: 128 TM rows, NX2 = 4 / 2 pieces per wave) on one 8 KB weight chunk D(j), 16 MFMAs per
// wave into the SAME accumulators, and the epilogue runs without scale, shift or residual: the sum stays fp32 until the one store.
// The downsample's values are therefore no longer rounded to fp16 or clamped on their own; the range guard sees the block output.
// X2(j) lands in X buffer (xidle + j) & 1 (xidle = the buffer the last macro-step does not read), D(j) in ring slot j % 3:
//     phase (L,0)       : W(L,2)[2]  X2(0)[NX2]        phase (L,1) : D(0)[2]          phase (L,2) : D(1)[2] (nc2 = 1: D(0) again)
//     phase T(j)        : X2(j+1)[NX2]  D(j+2)[2]      (each only while it exists)
//   opens (L,1): W(L,1);        younger: W(L,2) X2(0)   -> vmcnt(NX2+2)
//   opens (L,2): W(L,2);        younger: X2(0) D(0)     -> vmcnt(NX2+2)
//   opens T(0) : X2(0) D(0);    younger: D(1)           -> vmcnt(2)
//   opens T(j+1): X2(j+1) D(j+1); younger: D(j+2)       -> vmcnt(2) while j + 2 < nc2, else vmcnt(0)
//   the epilogue's strips overlay both X buffers and the W ring: vmcnt(0) before its barrier (nc2 = 1 leaves the second D(0) open)
// Raster rows that are not stored (halo columns, rows >= M) read a neighbouring pixel of the plane or past its range (zeros).

#include <type_traits>

#include "conv_internal.hpp"

namespace agp_igemm {

struct KxrwGroup {
    IgemmParams p[KXRW_MAXP];
    int mt_end[KXRW_MAXP];
    int nprob, MT, NT, mt_chunk;
    // round 6, the launch's LAST round of workgroups as HALF tiles (128 rows): row tiles [MT_full, MT) of the global sequence are
    // not in the XCD-ordered part of the grid but follow it as 2 (MT - MT_full) NT blocks from block `half_bid0` on
    int MT_full, half_bid0;
    uint32_t* rflag;           // the fp16 range guard's word (agp_range_flag_get), read by the RG = true instantiations only
    uint32_t r_bytes[KXRW_MAXP];   // bytes of each problem's residual plane (the buffer range of its LDS-DMA)
};
constexpr uint32_t KXRW_ROOB = 0xffffff00u;      // a residual offset past every plane: the piece's lane reads zeros
__device__ __forceinline__ const KxrwStreams& kxrw_streams(const KxrwStreams& s) { return s; }

// Tile shapes (a wave = TM_ x TN_ MFMA tiles of 32 x 32, four waves stacked along the rows):
//   TM_ = 2, TN_ = 4: 256 rows x 128 channels -- the full tile of the WIDE form, cout % 128 == 0;
//   TM_ = 1, TN_ = 4: 128 rows x 128 channels -- its HALF tile, the launch's last round of workgroups (kxrw_plan).
// (The tall form, 512 x 64 tiles on 4 x 2 MFMA tiles per wave for cout = 64, was measured and retired: profiles/README.md,
// round 3, "What was measured this round"; the code is in the history before the commit that removed it.)
constexpr int KW_ROWB = 64;
template <int TM_, int TN_> struct KwShape {
    static constexpr int BM = 128 * TM_, BN = 32 * TN_, BMX = BM + 16;
    static constexpr int XBUF = BMX * KW_ROWB, WTAP = BN * KW_ROWB;
    static constexpr int LDS = 2 * XBUF + 3 * WTAP + 2 * BN * 4;
    // the epilogue strips (a wave's tile row, 32 pixels x 2 BN bytes): as many waves as fit use the idle X buffer, the others the
    // spare region behind the stage (a half tile: behind its 2 KB of pooling scratch)
    static constexpr int STRIP = 32 * 2 * BN, XWAVES = XBUF / STRIP, SPARE = LDS + (TM_ == 1 ? 2048 : 0);
    static constexpr int EPI_LDS = SPARE + (4 - XWAVES) * STRIP;
};

// One tile: rows [m0, m0 + 128 TM_) x columns [n0, n0 + 32 TN_) of problem g.p[pid]; RES: the problem has a residual (chosen per
// tile, outside the tile's code: a branch around the last macro-step's MFMAs would cost the accumulators a trip through scratch).
// RES: 0 none, 1 a stored plane by LDS-DMA, 2 computed from the second operand stream *sp (file header).
template <bool POOL, int TM_, int TN_, bool RG, int RES>
__device__ __forceinline__ void kxrw_tile(const KxrwGroup& g, const int pid, const int m0, const int n0, const KxrwStream* sp = nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)
    using SH = KwShape<TM_, TN_>;
    constexpr int BN = SH::BN, NW = 4, TM = TM_, TN = TN_, ROWB = KW_ROWB;
    constexpr int X_BUF = SH::XBUF, W_TAP = SH::WTAP;
    constexpr int XINS = SH::BMX / 16;                 // LDS-DMA pieces (16 rows x 64 B) per X block: 17 / 9
    constexpr int NX = (XINS + NW - 1) / NW;           // 5 / 3 per wave; pieces beyond XINS re-issue the last one
    constexpr int NWP = BN / (NW * 16);                // 2 instructions per wave and W piece
    static_assert(TN == 4 && (TM == 2 || TM == 1), "the full tile (256 x 128) and its half tile (128 x 128)");
    static_assert(NWP == 2 && (NX == 5 || NX == 3), "the vmcnt counts exist for these");
    constexpr int NX2 = SH::BM / (16 * NW);            // RES = 2: pieces per wave of an X2 block (rows + 0 only): 4 / 2
    static_assert(!(POOL && RES == 2), "the computed residual is not instantiated with the pooling epilogue");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ws = smem + 2 * X_BUF;
    float* const tab = (float*)(ws + 3 * W_TAP);       // [scale 128][shift 128]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const IgemmParams& p = g.p[pid];

    const FastDiv d_howo = p.d_howo, d_wo = p.d_wo;
    const int pM = p.M, pN = p.N, pKtot = p.Ktot;
    const uint32_t pR = (uint32_t)p.img_rows;
    const int x_sn = p.x_sn, x_sh_ = p.x_sh, x_sw = p.x_sw, x_base = p.x_base;
    const int o_sn = p.o_sn, o_sw = p.o_sw, o_base = p.o_base;
    const float* const pscale = p.scale;
    const float* const pshift = p.shift;

    // ---- LDS-DMA source offsets (bytes)
    const int lrow = lane >> 2, lpos = lane & 3;
    int xoff[NX], woff[NWP];
#pragma unroll
    for (int q = 0; q < NX; ++q) {
        int ins = wave + NW * q;
        ins = ins < XINS ? ins : XINS - 1;
        const int row = ins * 16 + lrow;
        const int m = m0 + row;                         // not clamped: rows past the last image read zeros (buffer range check)
        const uint32_t img = fdiv((uint32_t)m, d_howo);
        const uint32_t rem = (uint32_t)m - img * d_howo.d;
        const uint32_t y = fdiv(rem, d_wo);
        const uint32_t xq = rem - y * d_wo.d;
        const int el = (int)img * x_sn + (int)y * x_sh_ + (int)xq * x_sw + x_base;
        xoff[q] = el * 2 + ((lpos ^ swz32(row)) << 4);
    }
#pragma unroll
    for (int i = 0; i < NWP; ++i) {
        const int row = (wave + NW * i) * 16 + lrow;
        int n = n0 + row;
        n = n < pN ? n : pN - 1;
        woff[i] = (p.w_cm ? n * 64 : n * pKtot * 2) + ((lpos ^ swz32(row)) << 4);     // chunk-major W: [Ktot/32][N][32]
    }
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x_hi, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w_cm ? p.w_cm : p.w_hi), 0, p.w_bytes, 0x00020000);

    const int CK = __builtin_amdgcn_readfirstlane(p.CK), x_sh = __builtin_amdgcn_readfirstlane(x_sh_);
    const int cchunks = CK / 32;
    const int nsteps = 3 * cchunks;
    const int tapb = CK * 2;
    float tab_s = 1.f, tab_t = 0.f;
    if (tid < BN) {
        const int n = n0 + tid < pN ? n0 + tid : pN - 1;
        if (pscale) tab_s = pscale[n];
        if (pshift) tab_t = pshift[n];
    }
    // the GeM exponent is fetched here, with the table, and lives in an SGPR: its first use in the pooled sweep would otherwise be
    // a vmcnt(0) that also waits for the tile row's output stores
    float pool_pw_v = 1.f;
    if (POOL && p.pool_p) pool_pw_v = p.pool_p[0];
    auto load_x = [&](int buf, int ky_, int cc_) {
        const int xs = __builtin_amdgcn_readfirstlane((ky_ * x_sh + cc_ * 32) * 2);
        char* base_ = smem + buf * X_BUF;
#pragma unroll
        for (int q = 0; q < NX; ++q) {
            int ins = wave + NW * q;
            ins = ins < XINS ? ins : XINS - 1;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, LDS_PTR(base_ + ins * 1024), 16, xoff[q], xs, 0, 0);
        }
    };
    const int wmul = __builtin_amdgcn_readfirstlane(p.w_cm ? pN : 1);      // a 64-byte K chunk is N * 64 bytes on in the chunk-major plane
    auto load_w = [&](int slot, int wbytes) {
        const int so = __builtin_amdgcn_readfirstlane(wbytes * wmul);
#pragma unroll
        for (int i = 0; i < NWP; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, LDS_PTR(ws + slot * W_TAP + (wave + NW * i) * 1024), 16, woff[i], so, 0, 0);
    };
    load_x(0, 0, 0);
    load_w(0, 0);
    load_w(1, tapb);

    // ---- fragment read offsets
    const int l31 = lane & 31, lh = lane >> 5;
    int xrd[3][2], wrd[2];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int r = wave * (TM * 32) + l31 + kx;
            xrd[kx][ks] = r * ROWB + (((2 * ks + lh) ^ swz32(r)) << 4);
        }
    {
        // W rows permuted (bits 2 and 3 swapped): accumulator registers 8h .. 8h+7 of a lane are 8 consecutive channels of its pixel
        const int wrow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) wrd[ks] = wrow * ROWB + (((2 * ks + lh) ^ swz32(wrow)) << 4);
    }

    f32x16 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // ---- epilogue addressing, LINE layout: a pixel's 128 channels are 256 bytes = 16 lanes of 16 bytes; a store instruction
    // covers 4 pixels; 8 instructions per tile row of 32 pixels
    constexpr int LPP = BN / 8, PPI = 64 / LPP, NEI = 32 / PPI;
    int eoff[TM * NEI];
    {
        const uint32_t wlast = d_wo.d - 1;
        const int img_extra = o_sn - (int)d_howo.d * o_sw;
#pragma unroll
        for (int q = 0; q < TM * NEI; ++q) {
            const int m = m0 + wave * (TM * 32) + (q / NEI) * 32 + (q % NEI) * PPI + lane / LPP;
            const uint32_t mm = (uint32_t)(m < pM ? m : pM - 1);
            const uint32_t img = fdiv(mm, d_howo);
            const uint32_t rem = mm - img * d_howo.d;
            const uint32_t y = fdiv(rem, d_wo);
            const uint32_t xq = rem - y * d_wo.d;
            const bool ok = (m < pM) && rem < pR && xq != 0 && xq != wlast;
            // the lane's 16-byte chunk of the pixel line, swizzled with the pixel's row in the strip (file header)
            const int chunk = (lane % LPP) ^ (((q % NEI) * PPI + lane / LPP) & 15);
            eoff[q] = ok ? (int)mm * o_sw + (int)img * img_extra + o_base + n0 + 8 * chunk : -1;
        }
    }
    float* const ppart = POOL ? p.pool_partial : nullptr;
    // ---- epilogue strips (wave-private, file header) and the residual's LDS-DMA
    static_assert(LPP == 16 && PPI == 4 && NEI == 8 && SH::STRIP == NEI * 1024, "a tile row = 8 pieces of 4 pixel lines of 256 bytes");
    const int xidle = nsteps & 1;                      // the X buffer the last macro-step does not read
    char* const strip0 = wave < SH::XWAVES ? smem + xidle * X_BUF + wave * SH::STRIP : smem + SH::SPARE + (wave - SH::XWAVES) * SH::STRIP;
    char* const strip1 = wave < 2 ? smem + (xidle ^ 1) * X_BUF + wave * SH::STRIP : ws + (wave - 2) * SH::STRIP;      // full tile only
    static_assert(TM == 1 || (SH::XWAVES == 2 && 2 * SH::STRIP <= 3 * W_TAP), "tile row 1: two waves per X buffer, two in the W ring");
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)p.r_hi, 0, g.r_bytes[pid], 0x00020000);
    auto load_residual = [&](char* strip, int tm, int i) {
        const int off = eoff[tm * NEI + i];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, LDS_PTR(strip + i * 1024), 16, off >= 0 ? off * 2 : (int)KXRW_ROOB, 0, 0, 0);
    };

    // ---- the second operand stream (RES = 2): its per-lane offsets are filled in behind the main loop, when xoff[] / woff[] die
    int x2off[RES == 2 ? NX2 : 1], doff[RES == 2 ? NWP : 1];
    int nc2 = 0;
    __amdgpu_buffer_rsrc_t rx2 = rx, rd2 = rw;
    if constexpr (RES == 2) {
        nc2 = __builtin_amdgcn_readfirstlane(sp->nc);
        rx2 = __builtin_amdgcn_make_buffer_rsrc((void*)sp->x, 0, sp->x_bytes, 0x00020000);
        rd2 = __builtin_amdgcn_make_buffer_rsrc((void*)sp->w, 0, sp->w_bytes, 0x00020000);
    }
    auto load_x2 = [&](int buf, int j, int q) {         // piece q of this wave of X2(j): rows (wave + 4 q) * 16 .. of the tile
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx2, LDS_PTR(smem + buf * X_BUF + (wave + NW * q) * 1024), 16, x2off[q],
                                                 __builtin_amdgcn_readfirstlane(j * 64), 0, 0);
    };
    auto load_d = [&](int slot, int j, int i) {         // instruction i of this wave of D(j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rd2, LDS_PTR(ws + slot * W_TAP + (wave + NW * i) * 1024), 16, doff[i],
                                                 __builtin_amdgcn_readfirstlane(j * 64 * pN), 0, 0);
    };

    int ky = 0, cc = 0;
    wait_vm_lgkm<NWP>();
    __builtin_amdgcn_s_barrier();
    // ---- main loop: a phase's LDS-DMA pieces are spread AMONG its MFMAs (igroup pipeline: sched_group_barrier) instead
    // of in front of them: an LDS-DMA instruction costs ~60 cycles of issue between bare MFMAs against 100-185 at the head of
    // a phase beside the fragment reads (MI355X_MICROARCH.md), and in front of the MFMAs that time is on the wave's chain.
    // The loop body has no branch (one scheduling region per phase): the last macro-step is peeled.
    if (tid < BN) { tab[tid] = tab_s; tab[BN + tid] = tab_t; }
    const float pool_pw = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, pool_pw_v)));
    auto phase = [&](auto KX, auto LAST, const char* xb, int st_, int nky_, int ncc_, int wcur_, int wnext_) {
        constexpr int kx = decltype(KX)::value;
        constexpr bool last = decltype(LAST)::value;
        constexpr int nres = last && RES == 1 && kx < 2 ? NEI / 2 : 0;     // tile row 0's residual pieces of this phase
        const char* wb = ws + kx * W_TAP;
        bf16x8 xf[2][TM], wf[2][TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) xf[0][t] = *(const bf16x8*)(xb + xrd[kx][0] + t * (32 * ROWB));
#pragma unroll
        for (int t = 0; t < TN; ++t) wf[0][t] = *(const bf16x8*)(wb + wrd[0] + t * (32 * ROWB));
        constexpr int nstr = last && RES == 2 ? (kx == 0 ? NX2 : NWP) : 0;      // the stream's pieces of this phase (file header)
        constexpr int ndma = (kx == 0 ? (last ? NWP : NWP + NX) : (last ? 0 : NWP)) + nres + nstr;
        static_assert(ndma <= 8, "one piece per MFMA pair");
#pragma unroll
        for (int t = 0; t < TM; ++t) xf[1][t] = *(const bf16x8*)(xb + xrd[kx][1] + t * (32 * ROWB));
#pragma unroll
        for (int t = 0; t < TN; ++t) wf[1][t] = *(const bf16x8*)(wb + wrd[1] + t * (32 * ROWB));
        // piece i of this phase's LDS-DMA list, in the order the vmcnt counts assume: W pieces first, then X(st + 1)
        auto piece = [&](int i) {
            if (nres && i >= ndma - nres) {
                load_residual(strip0, 0, kx * (NEI / 2) + i - (ndma - nres));
            } else if (nstr && i >= ndma - nstr) {
                const int k = i - (ndma - nstr);
                if (kx == 0) load_x2(xidle, 0, k);
                else load_d(kx - 1, kx - 1 < nc2 ? kx - 1 : nc2 - 1, k);
            } else if (kx == 0) {
                if (i < NWP) {
                    const int so = __builtin_amdgcn_readfirstlane((wcur_ + 2 * tapb) * wmul);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, LDS_PTR(ws + 2 * W_TAP + (wave + NW * i) * 1024), 16, woff[i], so, 0, 0);
                } else {
                    const int q = i - NWP;
                    const int xs = __builtin_amdgcn_readfirstlane((nky_ * x_sh + ncc_ * 32) * 2);
                    int ins = wave + NW * q;
                    ins = ins < XINS ? ins : XINS - 1;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, LDS_PTR(smem + ((st_ + 1) & 1) * X_BUF + ins * 1024), 16, xoff[q], xs, 0, 0);
                }
            } else {
                const int so = __builtin_amdgcn_readfirstlane((wnext_ + (kx - 1) * tapb) * wmul);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, LDS_PTR(ws + (kx - 1) * W_TAP + (wave + NW * i) * 1024), 16, woff[i], so, 0, 0);
            }
        };
        // all 12 fragment reads first (an LDS-DMA write may not pass an LDS read in program order), then MFMA pairs with one
        // piece behind each until the pieces are out
        int ip = 0;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf[ks][tn]),
                                                                         __builtin_bit_cast(f16x8, xf[ks][tm]), acc[tn][tm], 0, 0, 0);
                    if ((TM == 1 || (tm & 1)) && ip < ndma) { piece(ip); ++ip; }     // behind every second MFMA (every one of a half tile's 8)
                }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * (TM + TN), 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, TM == 1 ? 1 : 2, 0);
            if (i < ndma) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
    using BF = std::false_type; using BT = std::true_type;
    for (int st = 0; st < nsteps - 1; ++st) {
        int nky = ky, ncc = cc + 1;
        if (ncc == cchunks) { ncc = 0; ++nky; }
        const int wcur = (ky * 3 * CK + cc * 32) * 2, wnext = (nky * 3 * CK + ncc * 32) * 2;
        const char* xb = smem + (st & 1) * X_BUF;
        phase(I0{}, BF{}, xb, st, nky, ncc, wcur, wnext);
        wait_vm_lgkm<NX + NWP>();
        __builtin_amdgcn_s_barrier();
        phase(I1{}, BF{}, xb, st, nky, ncc, wcur, wnext);
        wait_vm_lgkm<NX + NWP>();
        __builtin_amdgcn_s_barrier();
        phase(I2{}, BF{}, xb, st, nky, ncc, wcur, wnext);
        wait_vm_lgkm<NWP>();
        __builtin_amdgcn_s_barrier();
        ky = nky; cc = ncc;
    }
    if constexpr (RES == 2) {
        const int s_sn = sp->sn, s_sh = sp->sh, s_sw = sp->sw, s_base = sp->base;
#pragma unroll
        for (int q = 0; q < NX2; ++q) {
            const int row = (wave + NW * q) * 16 + lrow;
            const int m = m0 + row;                     // not clamped: rows past the last image read zeros (buffer range check)
            const uint32_t img = fdiv((uint32_t)m, d_howo);
            const uint32_t rem = (uint32_t)m - img * d_howo.d;
            const uint32_t y = fdiv(rem, d_wo);
            const uint32_t xq = rem - y * d_wo.d;
            const int el = (int)img * s_sn + (int)y * s_sh + (int)xq * s_sw + s_base;
            x2off[q] = el * 2 + ((lpos ^ swz32(row)) << 4);
        }
#pragma unroll
        for (int i = 0; i < NWP; ++i) {
            const int row = (wave + NW * i) * 16 + lrow;
            const int n = n0 + row < pN ? n0 + row : pN - 1;
            doff[i] = n * 64 + ((lpos ^ swz32(row)) << 4);
        }
    }
    {
        const int st = nsteps - 1;
        const int wcur = (ky * 3 * CK + cc * 32) * 2;
        const char* xb = smem + (st & 1) * X_BUF;
        phase(I0{}, BT{}, xb, st, 0, 0, wcur, 0);
        wait_vm_lgkm<NWP + (RES == 1 ? NEI / 2 : RES == 2 ? NX2 : 0)>();
        __builtin_amdgcn_s_barrier();
        phase(I1{}, BT{}, xb, st, 0, 0, wcur, 0);
        wait_vm_lgkm<(RES == 1 ? NEI : RES == 2 ? NX2 + NWP : 0)>();
        __builtin_amdgcn_s_barrier();
        phase(I2{}, BT{}, xb, st, 0, 0, wcur, 0);
    }
    if constexpr (RES == 2) {
        // ---- the accumulators take the conv's scale and the summed shift in place, then the trailing phases add the downsample
        {
            const float* tb = tab + 8 * lh;
#pragma unroll
            for (int jj = 0; jj < TN * 2; ++jj) {
                const f32x4 s0 = *(const f32x4*)(tb + 16 * jj), s1 = *(const f32x4*)(tb + 16 * jj + 4);
                const f32x4 h0 = *(const f32x4*)(tb + BN + 16 * jj), h1 = *(const f32x4*)(tb + BN + 16 * jj + 4);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        acc[jj >> 1][tm][8 * (jj & 1) + e] =
                            acc[jj >> 1][tm][8 * (jj & 1) + e] * (e < 4 ? s0[e & 3] : s1[e & 3]) + (e < 4 ? h0[e & 3] : h1[e & 3]);
            }
        }
        // MODE 2: X2(j + 1) and D(j + 2) go out among this phase's MFMAs, 1: X2(j + 1) only, 0: nothing (the last phase)
        auto tphase = [&](auto MODE, int j) {
            constexpr int mode = decltype(MODE)::value;
            const char* xb = smem + ((xidle + j) & 1) * X_BUF;
            const char* wb = ws + (j % 3) * W_TAP;
            bf16x8 xf[2][TM], wf[2][TN];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int t = 0; t < TM; ++t) xf[ks][t] = *(const bf16x8*)(xb + xrd[0][ks] + t * (32 * ROWB));
#pragma unroll
                for (int t = 0; t < TN; ++t) wf[ks][t] = *(const bf16x8*)(wb + wrd[ks] + t * (32 * ROWB));
            }
            constexpr int ndma = mode == 2 ? NX2 + NWP : (mode == 1 ? NX2 : 0);
            static_assert(ndma <= 8, "one piece per MFMA pair");
            int ip = 0;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) {
                        acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf[ks][tn]),
                                                                             __builtin_bit_cast(f16x8, xf[ks][tm]), acc[tn][tm], 0, 0, 0);
                        if ((TM == 1 || (tm & 1)) && ip < ndma) {
                            if (ip < NX2) load_x2((xidle + j + 1) & 1, j + 1, ip);
                            else load_d((j + 2) % 3, j + 2, ip - NX2);
                            ++ip;
                        }
                    }
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * (TM + TN), 0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, TM == 1 ? 1 : 2, 0);
                if (i < ndma) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        wait_vm_lgkm<NWP>();
        __builtin_amdgcn_s_barrier();
        int j = 0;
        for (; j + 2 < nc2; ++j) {
            tphase(I2{}, j);
            wait_vm_lgkm<NWP>();
            __builtin_amdgcn_s_barrier();
        }
        for (; j + 1 < nc2; ++j) {
            tphase(I1{}, j);
            wait_vm_lgkm<0>();
            __builtin_amdgcn_s_barrier();
        }
        tphase(I0{}, j);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // ---- epilogue: accumulator layout (a lane = one pixel, 8 x 8 consecutive channels) <-> line layout through the wave's strip of
    // 32 rows x 256 bytes (file header): row = pixel, 16-byte slot s of row r = chunk s ^ (r & 15) of the pixel's line.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (RES == 1) {
        if constexpr (TM == 2) {
#pragma unroll
            for (int i = 0; i < NEI; ++i) load_residual(strip1, 1, i);
            wait_vm_lgkm<NEI>();
        } else {
            wait_vm_lgkm<0>();
        }
    }
    // accumulator layout: pixel l31, chunks 2 jj + lh; line layout: piece i = rows 4 i .. 4 i + 3, lane = (row, slot)
    const int a_off = l31 * (2 * BN) + ((lh ^ (l31 & 1)) << 4), a_swz = (l31 >> 1) & 7;
    const int l_off = lane * 16;
    const float* tb = tab + 8 * lh;
    bf16_t* const ohi = (bf16_t*)p.o_hi;
    const float relu_lo = p.relu ? 0.f : -65504.f;
    RangeTrack<RG> rg;
    float psum[2][2] = {{0.f, 0.f}, {0.f, 0.f}};       // [channel half][stat]
    float psum0[2][2] = {{0.f, 0.f}, {0.f, 0.f}};      // a full tile: the sums of its tile row 0 (32 rows) while tile row 1 is swept
    const float* const ppp = POOL ? p.pool_p : nullptr;
    const float pool_eps = POOL ? p.pool_eps : 0.f;
    const bool pool_cube = pool_pw == 3.f;
    const bool pool_sq = POOL && p.pool_sq;           // stat 1 = sum of squares (BatchNorm statistics), no exponent tensor
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        char* const strip = tm == 0 ? strip0 : strip1;
        if constexpr (POOL && TM == 2) {
            // a 64-row block is summed as (rows 0..31) + (rows 32..63) in EVERY schedule: a half tile holds the two halves in two
            // waves (even + odd below), so a full tile keeps them apart as well -- an image's pooled values must not depend on
            // whether its rows fall into the launch's full or half tiles
            if (tm == 1) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) { psum0[a][b] = psum[a][b]; psum[a][b] = 0.f; }
            }
        }
        u32x4 rres[TN * 2];
        if constexpr (RES == 1) {
#pragma unroll
            for (int jj = 0; jj < TN * 2; ++jj) rres[jj] = *(const u32x4*)(strip + a_off + ((jj ^ a_swz) << 5));
        }
        u32x4 outv[TN * 2];
#pragma unroll
        for (int jj = 0; jj < TN * 2; ++jj) {           // channels 16 jj + 8 lh .. + 7 of the tile's 128 columns
            const f32x4 s0 = *(const f32x4*)(tb + 16 * jj), s1 = *(const f32x4*)(tb + 16 * jj + 4);
            const f32x4 h0 = *(const f32x4*)(tb + BN + 16 * jj), h1 = *(const f32x4*)(tb + BN + 16 * jj + 4);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if constexpr (RES == 2) v[e] = acc[jj >> 1][tm][8 * (jj & 1) + e];      // scaled and shifted before the trailing phases
                else v[e] = acc[jj >> 1][tm][8 * (jj & 1) + e] * (e < 4 ? s0[e & 3] : s1[e & 3]) + (e < 4 ? h0[e & 3] : h1[e & 3]);
            }
            if constexpr (RES == 1) {
                float r[8];
                unpack8_h(rres[jj], r);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += r[e];
            }
            rg.any8(v);
            outv[jj] = pack8_h_lo(v, relu_lo);
        }
#pragma unroll
        for (int jj = 0; jj < TN * 2; ++jj) *(u32x4*)(strip + a_off + ((jj ^ a_swz) << 5)) = outv[jj];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        u32x4 lines[NEI];
#pragma unroll
        for (int i = 0; i < NEI; ++i) lines[i] = *(const u32x4*)(strip + l_off + i * 1024);
        if constexpr (TM == 2) {
            // tile row 1's residual has had this tile row's arithmetic to land; the wait stands before the stores because a store
            // counts in vmcnt as well
            if (tm == 0 && RES == 1) wait_vm_lgkm<0>();
        }
#pragma unroll
        for (int i = 0; i < NEI; ++i) {
            const int off = eoff[tm * NEI + i];
            if (off >= 0) *(u32x4*)(ohi + off) = lines[i];
        }
        if constexpr (POOL) {
            if (ppart) {
                // the strip holds the tile row as stored: 32 pixels x 128 channels fp16; the sweep runs while the stores above drain.
                // Pixels that are not stored (halo columns, raster rows past the image) are ZEROED in the strip first (the lanes that
                // hold their lines, exec-masked 16-byte writes), so the sweep needs no per-element mask: a zero adds nothing to the
                // mean and eps^p ~ 1e-18 to the GeM sum.  lane = a PAIR of channels (2 lane, 2 lane + 1): one ds_read_b32 per pixel
                // covers the 128 channels.  The statistic is chosen ONCE per tile row (four straight-line bodies); every sum is a
                // separately rounded multiply / add chain over the pixels in ascending order (no contraction: the pooled values
                // are the same bits in every schedule and statistic body).
#pragma unroll
                for (int i = 0; i < NEI; ++i)
                    if (eoff[tm * NEI + i] < 0) *(u32x4*)(strip + l_off + i * 1024) = u32x4{0u, 0u, 0u, 0u};
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                auto sweep = [&](auto STAT) {
#pragma clang fp contract(off)
                    constexpr int stat = decltype(STAT)::value;     // 0 mean only, 1 squares, 2 GeM p = 3, 3 GeM any p
#pragma unroll
                    for (int p8 = 0; p8 < 32; p8 += 8) {
                        uint32_t w[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) w[u] = *(const uint32_t*)(strip + (p8 + u) * (2 * BN) + ((lane * 4) ^ (((p8 + u) & 15) << 4)));
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const float v0 = h2f((bf16_t)(w[u] & 0xffffu)), v1 = h2f((bf16_t)(w[u] >> 16));
                            psum[0][0] += v0;
                            psum[1][0] += v1;
                            if constexpr (stat == 1) {
                                psum[0][1] += v0 * v0;
                                psum[1][1] += v1 * v1;
                            } else if constexpr (stat >= 2) {
                                const float c0 = fmaxf(v0, pool_eps), c1 = fmaxf(v1, pool_eps);
                                psum[0][1] += stat == 2 ? c0 * c0 * c0 : __builtin_exp2f(pool_pw * __builtin_log2f(c0));
                                psum[1][1] += stat == 2 ? c1 * c1 * c1 : __builtin_exp2f(pool_pw * __builtin_log2f(c1));
                            }
                        }
                    }
                };
                using I3 = std::integral_constant<int, 3>;
                if (pool_sq) sweep(I1{});
                else if (!ppp) sweep(I0{});
                else if (pool_cube) sweep(I2{});
                else sweep(I3{});
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    if constexpr (POOL) {
        if (ppart) {
            if constexpr (TM == 2) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) psum[a][b] = psum0[a][b] + psum[a][b];
            }
            // [64-row block][stat][N]: a wave of a full tile IS a block; in a half tile (32 rows per wave) the odd wave hands its sums
            // to the even wave of its pair through LDS (fixed order: even + odd)
            if constexpr (TM == 1) {
                float* const scr = (float*)(ws + 3 * W_TAP) + 2 * BN;          // behind the scale / shift table
                if (wave & 1) *(f32x4*)(scr + ((wave >> 1) * 64 + lane) * 4) = f32x4{psum[0][0], psum[0][1], psum[1][0], psum[1][1]};
                __syncthreads();
                if (!(wave & 1)) {
                    const f32x4 o = *(const f32x4*)(scr + ((wave >> 1) * 64 + lane) * 4);
                    psum[0][0] += o[0]; psum[0][1] += o[1]; psum[1][0] += o[2]; psum[1][1] += o[3];
                }
            }
            if (TM == 2 || !(wave & 1)) {
                const int block = m0 / 64 + (TM == 2 ? wave : (wave >> 1));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int n = n0 + 2 * lane + h;          // psum[h]: channel 2 lane + h of the tile's 128 columns
                    if (n < pN) {
                        float* o = ppart + ((size_t)block * 2) * pN + n;      // [block][stat][N]
                        o[0] = psum[h][0];
                        if (ppp || pool_sq) o[pN] = psum[h][1];
                    }
                }
            }
        }
    }
    rg.flush(g.rflag, relu_lo);
#endif
}

// block -> (problem, row tile, column tile).  XCD x owns a contiguous chunk of the global row tiles [0, MT_full); MIX: the blocks
// from half_bid0 on are the HALF tiles (128 rows) of the row tiles [MT_full, MT) -- the launch's last, partial round of workgroups.
// They carry the highest block ids, so they are dispatched last: the long tiles first, the short ones fill the end.
// ds: the problems' second operand streams in the instantiations that hold the RES = 2 tile bodies (launch_kxrw_ds); the others
// are the kernels of every launch without such a problem, unchanged.
template <bool POOL, bool MIX, bool RG, class... DS>
__global__ void __launch_bounds__(256, 2) igemm_kxrw_kernel(KxrwGroup g, DS... ds) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int TM_ = 2, TN_ = 4;
    constexpr int BM = KwShape<TM_, TN_>::BM, BN = KwShape<TM_, TN_>::BN;
    const int bid = blockIdx.x;
    const int gNT = g.NT, gnprob = g.nprob;
    const int e0 = g.mt_end[0], e1 = g.mt_end[1], e2 = g.mt_end[2];
    int mt, nt, sub = 0;
    bool half = false;
    if (MIX && bid >= g.half_bid0) {
        const int h = bid - g.half_bid0;
        nt = h % gNT;
        const int hm = h / gNT;
        mt = g.MT_full + (hm >> 1);
        sub = hm & 1;
        half = true;
        if (mt >= g.MT) return;
    } else {
        const int xcd = bid & 7, j = bid >> 3;
        nt = j % gNT;
        mt = xcd * g.mt_chunk + j / gNT;
        if (mt >= g.MT_full) return;
    }
    const int pid = group_problem(mt, gnprob, e0, e1, e2);
    const int n0 = nt * BN;
    if constexpr (MIX) {
        if (half) {
            const int m0 = mt * BM + sub * (BM / 2);
            if (m0 >= g.p[pid].M) return;                  // the second half of a problem's last, partial row tile
            if constexpr (sizeof...(DS) != 0) {
                const KxrwStream* sp = &kxrw_streams(ds...).s[pid];
                if (sp->x) { kxrw_tile<POOL, 1, TN_, RG, 2>(g, pid, m0, n0, sp); return; }
            }
            if (g.p[pid].r_hi) kxrw_tile<POOL, 1, TN_, RG, 1>(g, pid, m0, n0);
            else kxrw_tile<POOL, 1, TN_, RG, 0>(g, pid, m0, n0);
            return;
        }
    }
    if constexpr (sizeof...(DS) != 0) {
        const KxrwStream* sp = &kxrw_streams(ds...).s[pid];
        if (sp->x) { kxrw_tile<POOL, TM_, TN_, RG, 2>(g, pid, mt * BM, n0, sp); return; }
    }
    if (g.p[pid].r_hi) kxrw_tile<POOL, TM_, TN_, RG, 1>(g, pid, mt * BM, n0);
    else kxrw_tile<POOL, TM_, TN_, RG, 0>(g, pid, mt * BM, n0);
#endif
}

// The tile schedule of a launch of MT x NT tiles: the XCD-chunked part [0, MT_full) and the half tiles that follow it.  The launch
// and agp_conv2d_tile_plan both take their numbers from here.
struct KxrwPlan {
    int MT_full, mt_chunk, half_bid0, half_tiles, blocks;
    bool mix;
};
inline KxrwPlan kxrw_plan(int MT, int NT) {
    KxrwPlan k = {};
    k.MT_full = MT;
    // ---- the last round of workgroups as half tiles.  512 workgroups are resident (two per CU); a launch of T tiles runs
    // ceil(T / 512) rounds and its last round holds `tail` tiles.  When that round would leave more than half of the CUs without
    // a workgroup (tail <= 128), its tiles run as twice as many 128-row tiles, each still alone on a CU: the round takes about half
    // as long (stage 2: 602 tiles = 512 + 90 -> 180 half tiles, 89.7 -> 80.1 us; a launch of <= 128 tiles -- the C1 / C2 shapes --
    // covers twice the CUs).  Measured and NOT done: a larger tail (layer 3: 714 = 512 + 202 -> 404 half tiles, two per CU) loses
    // 3-4 us per launch -- a lone 256-row workgroup already runs 1.65 x as fast as one of a pair, two half tiles per CU do not.
    const int slots = 512, T = MT * NT;
    const int tail = T - (T - 1) / slots * slots;         // 1 .. slots
    if (tail <= slots / 4 && tail % NT == 0) {
        k.MT_full = MT - tail / NT;
        k.mix = true;
    }
    const XcdGrid xg = xcd_grid(k.MT_full, NT);
    k.mt_chunk = xg.mt_chunk;
    k.half_bid0 = xg.blocks;
    k.half_tiles = k.mix ? 2 * (MT - k.MT_full) * NT : 0;
    k.blocks = k.half_bid0 + k.half_tiles;
    return k;
}

template <bool POOL, bool MIX, bool RG>
int launch_kxrw(KxrwGroup& g, const KxrwPlan& k, hipStream_t s) {
    constexpr int lds = KwShape<2, 4>::EPI_LDS;
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    static_assert(KwShape<1, 4>::EPI_LDS <= lds, "half tiles: their stage, the pooling scratch and their strips fit the full tile's LDS");
    static std::atomic<uint64_t> attr_done{0};
    if (!agp_lds_attr((const void*)igemm_kxrw_kernel<POOL, MIX, RG>, lds, attr_done)) return AGP_E_LAUNCH;
    AGP_LAUNCH((igemm_kxrw_kernel<POOL, MIX, RG>), dim3(MIX ? k.blocks : k.half_bid0), dim3(256), lds, s, g);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

template <bool MIX, bool RG>
int launch_kxrw_ds(KxrwGroup& g, const KxrwStreams& ds, const KxrwPlan& k, hipStream_t s) {
    constexpr int lds = KwShape<2, 4>::EPI_LDS;
    static std::atomic<uint64_t> attr_done{0};
    if (!agp_lds_attr((const void*)igemm_kxrw_kernel<false, MIX, RG, KxrwStreams>, lds, attr_done)) return AGP_E_LAUNCH;
    AGP_LAUNCH((igemm_kxrw_kernel<false, MIX, RG, KxrwStreams>), dim3(MIX ? k.blocks : k.half_bid0), dim3(256), lds, s, g, ds);
    AGP_CHECK_LAUNCH();
    return AGP_OK;
}

}  // namespace agp_igemm

// `ps[i]` arrive with the padded-width raster geometry of agp_internal_conv_kxr_geometry; all share N, CK, prec F16 and
// N % 128 == 0 (256 x 128 tiles).  ds != NULL: the problems' second operand streams (at least one with a plane; none of those
// problems has a residual plane or pools).
int agp_internal_conv_kxrw(agp_igemm::IgemmParams* ps, int n, hipStream_t s, agp_igemm::TilePlan* plan, const agp_igemm::KxrwStreams* ds) {
    using namespace agp_igemm;
    if (n < 1 || n > KXRW_MAXP || ps[0].N % 128) return AGP_E_BADARG;
    constexpr int bm = KwShape<2, 4>::BM, bn = KwShape<2, 4>::BN;
    KxrwGroup g = {};
    g.nprob = n;
    int mt = 0;
    bool pool = false;
    for (int i = 0; i < n; ++i) {
        if (ps[i].N != ps[0].N || ps[i].CK != ps[0].CK) return AGP_E_BADARG;
        g.p[i] = ps[i];
        mt += (ps[i].M + bm - 1) / bm;
        g.mt_end[i] = mt;
        pool = pool || ps[i].pool_partial != nullptr;
        // the residual plane has the output's geometry: M / (raster rows per image) images of o_sn elements
        const int64_t rb = (int64_t)(ps[i].M / (int)ps[i].d_howo.d) * ps[i].o_sn * 2;
        if (ps[i].r_hi && (rb <= 0 || rb > (int64_t)KXRW_ROOB)) return AGP_E_BADARG;
        g.r_bytes[i] = (uint32_t)rb;
    }
    g.MT = mt;
    g.NT = ps[0].N / bn;
    const KxrwPlan k = kxrw_plan(g.MT, g.NT);
    if (plan) {
        *plan = TilePlan{AGP_CONV_KERNEL_KXRW, bm, bn, g.MT, g.NT, k.MT_full, k.half_tiles, k.blocks};
        return AGP_OK;
    }
    const bool mix = k.mix;
    g.MT_full = k.MT_full;
    g.mt_chunk = k.mt_chunk;
    g.half_bid0 = k.half_bid0;
    g.rflag = agp_range_flag_get();
    if (ds) {
        if (pool) return AGP_E_UNSUPPORTED;
        return agp_rg_dispatch(g.rflag, [&](auto rg) {
            constexpr bool RG = decltype(rg)::value;
            return mix ? launch_kxrw_ds<true, RG>(g, *ds, k, s) : launch_kxrw_ds<false, RG>(g, *ds, k, s);
        });
    }
    return agp_rg_dispatch(g.rflag, [&](auto rg) {
        constexpr bool RG = decltype(rg)::value;
        if (mix) return pool ? launch_kxrw<true, true, RG>(g, k, s) : launch_kxrw<false, true, RG>(g, k, s);
        return pool ? launch_kxrw<true, false, RG>(g, k, s) : launch_kxrw<false, false, RG>(g, k, s);
    });
}
