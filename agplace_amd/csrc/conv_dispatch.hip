// Host-side routing of the dense convolutions (agp_conv2d_*, agp_stem_pool_*): which kernel runs a descriptor or a group, the
// generic geometry every launcher starts from, the size queries.  No kernel lives here (launchers: conv_internal.hpp).  Every
// eligibility rule is written once, below; a call site that asks for more than the shared rule adds terms of its own.
#include "conv_internal.hpp"
using namespace agp_igemm;

// A halo-1 plane [n][h + 2][w + 2][c] of 2-byte elements within 31-bit byte offsets.
static bool fits_31(int n, int h, int w, int c) { return (int64_t)n * (h + 2) * (w + 2) * c * 2 < (1ll << 31); }

// 3x3 / stride 1 / pad 1 on unpacked planes ...
static bool conv_3x3s1(const agp_conv_desc* d) {
    return d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && d->in_w_step == d->cin;
}
// ... that the 3x3 stride-1 family can address: 1-pixel halos on both maps, equal sizes, the input within 2^31 bytes
static bool conv_kxr_ok(const agp_conv_desc* d) {
    return conv_3x3s1(d) && d->pin == 1 && d->pout == 1 && d->hout == d->hin && d->wout == d->win && fits_31(d->n, d->hin, d->win, d->cin);
}

// A member of a one-launch group of 3x3 / stride-1 convs of `d0`'s channel shape (agp_internal_use_kxr2 implies AGP_PREC_F16).
static bool kxr2_member_ok(const agp_conv_desc* d, const agp_conv_desc* d0) {
    return d->in_hi && d->w_hi && d->out_hi && !d->in_lo && !d->out_lo && !d->res_lo && d->n > 0 &&
           d->cin % 32 == 0 && d->cout % 64 == 0 && conv_kxr_ok(d) && agp_internal_use_kxr2(d) &&
           d->cin == d0->cin && d->cout == d0->cout;
}

// The 3x3 / stride-2 conv of a stage entry as igemm_s2 runs it, of `d0`'s channel shape ...
static bool s2_conv_ok(const agp_conv_desc* c, const agp_conv_desc* d0) {
    return c->prec == AGP_PREC_F16 && c->in_hi && c->w_hi && c->out_hi && !c->in_lo && !c->out_lo && !c->res_hi &&
           !c->stat_partial && !c->pool_partial &&
           c->kh == 3 && c->kw == 3 && c->stride == 2 && c->pad == 1 && c->pin == 1 && c->pout == 1 && c->in_w_step == c->cin &&
           c->hout == (c->hin - 1) / 2 + 1 && c->wout == (c->win - 1) / 2 + 1 &&
           c->cin % 32 == 0 && c->cout % 64 == 0 && c->n > 0 && c->cin == d0->cin && c->cout == d0->cout &&
           fits_31(c->n, c->hin, c->win, c->cin) && fits_31(c->n, c->hout, c->wout, c->cout);
}
// ... and its 1x1 / stride-2 downsample partner `d`: the same input and geometry, no residual, no ReLU
static bool s2_downsample_ok(const agp_conv_desc* d, const agp_conv_desc* c) {
    return d->prec == AGP_PREC_F16 && d->w_hi && d->out_hi && !d->in_lo && !d->out_lo && !d->res_hi && !d->stat_partial && !d->pool_partial &&
           d->kh == 1 && d->kw == 1 && d->stride == 2 && d->pad == 0 && d->pin == 1 && d->pout == 1 && d->in_w_step == d->cin &&
           d->in_hi == c->in_hi && d->n == c->n && d->hin == c->hin && d->win == c->win && d->cin == c->cin &&
           d->cout == c->cout && d->hout == c->hout && d->wout == c->wout && !d->relu;
}

// The kernel of a single conv (AGP_CONV_KERNEL_GENERIC / _DIRECT_X / _KXR), from its geometry alone:
//   3x3 stride-1 pad-1 on 1-pixel-halo planes -> igemm_kxr.hip / igemm_kxr2.hip / igemm_kxrw.hip (horizontal-tap reuse in LDS)
//   packed stem (in_w_step != cin)             -> igemm_d16.hip (X straight into registers)
//   everything else (1x1, stride 2)            -> the generic LDS-staged kernel (igemm.hip)
// Development build: CONV_KERNEL = 1 generic / 2 direct-X / 3 3x3 kernel forces one where it is applicable.
static int conv_route(const agp_conv_desc* d) {
    const int force = AGP_TUNE("CONV_KERNEL", 0);
    if (force && force != AGP_CONV_KERNEL_KXR) return force;
    if (conv_kxr_ok(d)) return AGP_CONV_KERNEL_KXR;
    return d->in_w_step != d->cin ? AGP_CONV_KERNEL_DIRECT_X : AGP_CONV_KERNEL_GENERIC;
}

static int conv_launch(int which, IgemmParams& p, const agp_conv_desc* d, hipStream_t s, TilePlan* plan) {
    if (which == AGP_CONV_KERNEL_KXR) return agp_internal_conv_kxr(p, d, s, plan);
    if (which == AGP_CONV_KERNEL_DIRECT_X) return agp_internal_conv_d16(p, d->prec, s, plan);
    return agp_internal_conv_generic(p, d->prec, s, plan);
}

// Which convs come with per-tile channel statistics (agp_conv_desc::stat_partial): bf16-pair maps only; the packed stem on the
// direct-X kernel; the generic kernel for everything that is no 3x3 / stride-1 conv; igemm_kxr for those -- one whose planes
// igemm_kxr cannot address has none, although the generic kernel would run it.
static bool conv_emits_stats(const agp_conv_desc* d) {
    if (d->prec != AGP_PREC_BF16X3) return false;
    const int force = AGP_TUNE("CONV_KERNEL", 0);
    if (d->in_w_step != d->cin) return !force && d->cout % 64 == 0;
    if (d->cin % 32 || d->cout % 64) return false;
    if (!conv_3x3s1(d)) return !force && !AGP_TUNE("IGEMM_VARIANT", 0);
    return conv_kxr_ok(d) && (!force || force == AGP_CONV_KERNEL_KXR);
}

// ---- the generic geometry of `d` (every conv kernel starts from it)
static void conv_fill_geometry(const agp_conv_desc* d, IgemmParams& p) {
    const int hp = d->hin + 2 * d->pin, wp = d->win + 2 * d->pin;
    const int wstep = d->in_w_step;
    p.M = d->n * d->hout * d->wout;
    p.N = d->cout;
    p.KW = d->kw; p.CK = d->cin; p.ntaps = d->kh * d->kw;
    p.Ktot = d->kh * d->kw * d->cin;
    p.d_howo = make_fastdiv((uint32_t)(d->hout * d->wout));
    p.d_wo = make_fastdiv((uint32_t)d->wout);
    p.x_sw = wstep; p.x_sh = wp * wstep; p.x_sn = hp * wp * wstep;
    p.x_base = ((d->pin - d->pad) * wp + (d->pin - d->pad)) * wstep;
    p.sy = d->stride; p.sx = d->stride;
    const int hop = d->hout + 2 * d->pout, wop = d->wout + 2 * d->pout;
    p.o_sw = d->cout; p.o_sh = wop * d->cout; p.o_sn = hop * wop * d->cout;
    p.o_base = (d->pout * wop + d->pout) * d->cout;
}

// ... and its operands: planes, weights in the orders the kernels take, epilogue, the optional reductions.
static int conv_fill_params(const agp_conv_desc* d, IgemmParams& p) {
    // bytes of one plane; for the packed stem (in_w_step < cin) rows overlap, the plane
    // still has hp*wp pixels of in_w_step elements.
    const int64_t x_elems = (int64_t)d->n * (d->hin + 2 * d->pin) * (d->win + 2 * d->pin) * d->in_w_step;
    const int64_t w_elems = (int64_t)d->cout * d->kh * d->kw * d->cin;
    if (x_elems * 2 >= (1ll << 32) || w_elems * 2 >= (1ll << 31)) return AGP_E_BADARG;
    p.x_hi = d->in_hi; p.x_lo = d->in_lo; p.x_bytes = (uint32_t)(x_elems * 2);
    p.w_hi = d->w_hi; p.w_lo = d->w_lo; p.w_bytes = (uint32_t)(w_elems * 2);
    if (d->prec == AGP_PREC_F16W2 && d->w_q8) { p.w_q8 = d->w_q8; p.w_q8_exp = d->w_q8_exp; }
    if (d->prec == AGP_PREC_F16 && d->w_cm) p.w_cm = d->w_cm;
    // the two-plane modes (igemm_kxr: 3x3 stride-1 convs): both planes chunk-major
    if ((d->prec == AGP_PREC_F16W2 || d->prec == AGP_PREC_BF16X3) && d->w_cm && conv_3x3s1(d) &&
        (d->w_cm_lo || (d->hi_only && d->prec == AGP_PREC_BF16X3))) {
        p.w_cm = d->w_cm; p.w_cm_lo = d->w_cm_lo;
    }
    if (d->stat_partial) {
        if (agp_conv2d_stat_tiles(d) <= 0) return AGP_E_BADARG;      // only the kernels that can produce them
        p.stat_partial = d->stat_partial;
        if (d->bstat_z_hi) {
            // backward mode: the 3x3 stride-1 kernel only (the other kernels' tiles carry forward sums)
            // (bstat_z_lo NULL: z is ONE fp16 plane -- the output of a forward conv that ran as one fp16 product)
            if (!d->bstat_mean || !d->bstat_rstd || !conv_3x3s1(d)) return AGP_E_BADARG;
            p.bs_z_hi = d->bstat_z_hi; p.bs_z_lo = d->bstat_z_lo; p.bs_y_hi = d->bstat_y_hi;
            p.bs_mean = d->bstat_mean; p.bs_rstd = d->bstat_rstd;
        }
    } else if (d->bstat_z_hi) {
        return AGP_E_BADARG;
    }
    if (d->pool_partial) {
        if (agp_conv2d_pool_blocks(d) <= 0) return AGP_E_BADARG;
        if (d->pool_stat != 0 && d->pool_stat != 1) return AGP_E_BADARG;
        p.pool_partial = d->pool_partial; p.pool_p = d->pool_stat ? nullptr : d->pool_p; p.pool_eps = d->pool_eps; p.pool_sq = d->pool_stat;
    }
    conv_fill_geometry(d, p);
    p.o_hi = d->out_hi; p.o_lo = d->out_lo;
    p.r_hi = d->res_hi; p.r_lo = d->res_lo;
    p.scale = d->scale; p.shift = d->shift; p.relu = d->relu;
    p.dbg = AGP_TUNE("IGEMM_DBG", 0);
    return AGP_OK;
}

static int conv_fill_group(const agp_conv_desc* descs, int n, IgemmParams* ps, bool kxr_geometry) {
    for (int i = 0; i < n; ++i) {
        ps[i] = IgemmParams{};
        const int rc = conv_fill_params(descs + i, ps[i]);
        if (rc != AGP_OK) return rc;
        if (kxr_geometry) agp_internal_conv_kxr_geometry(ps[i], descs + i);
    }
    return AGP_OK;
}

// ---- the size queries
// Row tiles of the kernel that would run `d`, if that kernel can emit per-tile channel statistics: MT of the plan the single-conv
// route makes for `d`'s geometry (the statistics buffer has one row per tile the kernel walks).  Looks at no pointer of `d`.
extern "C" int agp_conv2d_stat_tiles(const agp_conv_desc* d) {
    if (!d || !conv_emits_stats(d) || d->n <= 0 || d->hout <= 0 || d->wout <= 0) return 0;
    agp_conv_desc q = *d;           // (asked without the request itself, as the callers that size the buffer ask)
    q.stat_partial = nullptr;
    q.bstat_z_hi = q.bstat_z_lo = q.bstat_y_hi = nullptr; q.bstat_mean = q.bstat_rstd = nullptr;
    IgemmParams p = {};
    conv_fill_geometry(&q, p);
    TilePlan tp = {};
    return conv_launch(conv_route(&q), p, &q, nullptr, &tp) == AGP_OK ? tp.MT : 0;
}

// 64-row blocks of agp_conv_desc::pool_partial: the AGP_PREC_F16 3x3 stride-1 kernel (igemm_kxr2, 256-row tiles of four
// 64-row wave blocks) over a raster that gives every image a multiple of 64 rows.
extern "C" int agp_conv2d_pool_blocks(const agp_conv_desc* d) {
    if (!d || d->prec != AGP_PREC_F16 || d->in_lo || d->out_lo || d->cin % 32 || d->cout % 64 || d->n <= 0) return 0;
    if (!conv_kxr_ok(d) || !agp_internal_use_kxr2(d) || AGP_TUNE("CONV_KERNEL", 0) || AGP_TUNE("NO_CONV_POOL", 0)) return 0;
    const int64_t rp = ((int64_t)d->hin * (d->win + 2) + 63) / 64 * 64;
    if ((int64_t)d->n * rp >= (1ll << 31)) return 0;
    return (int)(((int64_t)d->n * rp + 511) / 512 * 8);      // (64-row blocks of 256- or 512-row tiles: the larger count)
}

// ---- one conv
// `plan` != NULL (agp_conv2d_tile_plan): the same decisions, reported instead of launched.
static int conv2d_fwd_one(const agp_conv_desc* d, void* stream, TilePlan* plan) {
    if (!d || !d->in_hi || !d->w_hi || !d->out_hi) return AGP_E_BADARG;
    // storage format follows the precision: BF16X3 = bf16 plane pairs everywhere; F16W2 / F16 = one
    // fp16 activation plane (lo pointers NULL) and an fp16 weight pair / single plane
    if (d->prec == AGP_PREC_BF16X3) {
        if ((!d->hi_only && (!d->in_lo || !d->w_lo)) || !d->out_lo || (d->res_hi && !d->res_lo)) return AGP_E_BADARG;
    } else if (d->prec == AGP_PREC_F16W2 || d->prec == AGP_PREC_F16) {
        if (d->in_lo || d->out_lo || d->res_lo) return AGP_E_BADARG;
        if (d->prec == AGP_PREC_F16W2 && !d->w_lo) return AGP_E_BADARG;
    } else {
        return AGP_E_BADARG;
    }
    if (d->cin % 32 || d->cout % 64 || d->n <= 0) return AGP_E_BADARG;
    if (d->pin < d->pad && d->in_w_step == d->cin) return AGP_E_BADARG;
    IgemmParams p = {};
    if (const int rc = conv_fill_params(d, p); rc != AGP_OK) return rc;
#if defined(AGP_TUNING)
    if (p.dbg & 0x1000000) {   // census experiment (tools/census.py): the record buffer's address as two switch words
        const uint64_t a = ((uint64_t)(uint32_t)AGP_TUNE("CENSUS_BUF_HI", 0) << 32) | (uint32_t)AGP_TUNE("CENSUS_BUF_LO", 0);
        p.gmin = (float*)(uintptr_t)a;
        if (!p.gmin) p.dbg &= ~0x1000000;
    }
#endif
    const int which = conv_route(d);
    // the 3x3 stride-1 kernel's one-product form only
    if (d->hi_only && (d->prec != AGP_PREC_BF16X3 || which != AGP_CONV_KERNEL_KXR)) return AGP_E_BADARG;
    // w_cm == w_hi: the caller holds chunk-major planes ONLY (training planes written that way): every kernel but the 3x3 stride-1
    // one would read them as row-major -- refuse instead
    if (d->w_cm && d->w_cm == d->w_hi && (which != AGP_CONV_KERNEL_KXR || !p.w_cm)) return AGP_E_BADARG;
    return conv_launch(which, p, d, (hipStream_t)stream, plan);
}

extern "C" int agp_conv2d_fwd(const agp_conv_desc* d, void* stream) { return conv2d_fwd_one(d, stream, nullptr); }

// ---- groups (agp_conv2d_fwd_grouped): a route returns NOT_TAKEN, or the result of its launch
constexpr int NOT_TAKEN = -1;
// Route A: 2..4 3x3 / stride-1 convs of ONE channel shape, fp16 with one product, as ONE launch: the tiles of every problem form
// one grid (igemm_kxr2.hip / igemm_kxrw.hip).
static int group_route_kxr2(const agp_conv_desc* descs, int n, hipStream_t s, TilePlan* plan) {
    if (n < 2 || n > 4 || AGP_TUNE("CONV_KERNEL", 0)) return NOT_TAKEN;
    for (int i = 0; i < n; ++i)
        if (!kxr2_member_ok(descs + i, descs)) return NOT_TAKEN;
    IgemmParams ps[4];
    const int rc = conv_fill_group(descs, n, ps, true);
    return rc != AGP_OK ? rc : agp_internal_conv_kxr2(ps, n, s, plan);
}

// Route B: the stride-2 entry of a ResNet stage: [3x3/s2 conv of every trunk ..., its 1x1/s2 downsample of every trunk ...] on
// fp16 maps with one product -> ONE launch of igemm_s2.hip (the downsample rides on the 3x3's staged centre tap).
static int group_route_s2(const agp_conv_desc* descs, int n, hipStream_t s, TilePlan* plan) {
    if ((n != 2 && n != 4) || AGP_TUNE("CONV_KERNEL", 0) || AGP_TUNE("NO_S2", 0)) return NOT_TAKEN;
    const int h = n / 2;
    for (int i = 0; i < h; ++i)
        if (!s2_conv_ok(descs + i, descs) || !s2_downsample_ok(descs + h + i, descs + i)) return NOT_TAKEN;
    IgemmParams ps[2];
    if (const int rc = conv_fill_group(descs, h, ps, false); rc != AGP_OK) return rc;
    for (int i = 0; i < h; ++i) {
        const agp_conv_desc* d = descs + h + i;
        ps[i].w2_hi = d->w_hi; ps[i].w2_cm = d->w_cm; ps[i].scale2 = d->scale; ps[i].shift2 = d->shift; ps[i].o2_hi = d->out_hi;
    }
    return agp_internal_conv_s2(ps, descs, h, s, plan, false);
}

// Route C: 2..4 fp16 single-product convs of the generic kernel (1x1 and stride-2 convs) of one tile configuration, e.g. a stage
// entry that route B refused.
static int group_route_generic(const agp_conv_desc* descs, int n, hipStream_t s, TilePlan* plan) {
    if (n < 2 || n > 4 || AGP_TUNE("CONV_KERNEL", 0) || AGP_TUNE("NO_IGEMM_GROUP", 0)) return NOT_TAKEN;
    for (int i = 0; i < n; ++i) {
        const agp_conv_desc* d = descs + i;
        if (!(d->in_hi && d->w_hi && d->out_hi && !d->in_lo && !d->out_lo && !d->res_lo && d->n > 0 &&
              d->prec == AGP_PREC_F16 && !d->stat_partial && d->cin % 64 == 0 && d->cout % 128 == 0 &&
              !conv_kxr_ok(d) && d->in_w_step == d->cin && !(d->pin < d->pad)))
            return NOT_TAKEN;
    }
    IgemmParams ps[4];
    const int rc = conv_fill_group(descs, n, ps, false);
    return rc != AGP_OK ? rc : agp_internal_conv_generic_group(ps, n, s, plan);
}

// Groups no route takes run as `n` launches, in order.
static int conv2d_fwd_group(const agp_conv_desc* descs, int n, void* stream, TilePlan* plan) {
    if (!descs || n <= 0) return AGP_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = group_route_kxr2(descs, n, s, plan)) != NOT_TAKEN) return rc;
    if ((rc = group_route_s2(descs, n, s, plan)) != NOT_TAKEN) return rc;
    if ((rc = group_route_generic(descs, n, s, plan)) != NOT_TAKEN) return rc;
    if (plan && n > 1) return AGP_E_UNSUPPORTED;      // `n` launches: ask for each descriptor's plan
    rc = AGP_OK;
    for (int i = 0; i < n && rc == AGP_OK; ++i) rc = conv2d_fwd_one(descs + i, stream, plan);
    return rc;
}

extern "C" int agp_conv2d_fwd_grouped(const agp_conv_desc* descs, int n, void* stream) { return conv2d_fwd_group(descs, n, stream, nullptr); }

// The tile plan of the launch that agp_conv2d_fwd (n == 1) / agp_conv2d_fwd_grouped (n > 1) would make for these descriptors:
// the launch path itself, stopped in the launcher before anything touches the device.
extern "C" int agp_conv2d_tile_plan(const agp_conv_desc* descs, int n, int32_t plan[8]) {
    if (!descs || !plan || n <= 0) return AGP_E_BADARG;
    TilePlan tp = {};
    const int rc = n == 1 ? conv2d_fwd_one(descs, nullptr, &tp) : conv2d_fwd_group(descs, n, nullptr, &tp);
    if (rc != AGP_OK) return rc;
    const int32_t v[8] = {tp.kernel, tp.BM, tp.BN, tp.MT, tp.NT, tp.MT_full, tp.half_tiles, tp.grid};
    for (int i = 0; i < 8; ++i) plan[i] = v[i];
    return AGP_OK;
}

// ---- the stage entry without a stored downsample map (include/agplace_hip.h)
extern "C" int agp_conv2d_s2_fwd(const agp_conv_desc* descs, int n, void* stream) {
    if (!descs) return AGP_E_BADARG;
    if (n < 1 || n > 2 || AGP_TUNE("CONV_KERNEL", 0) || AGP_TUNE("NO_S2", 0)) return AGP_E_UNSUPPORTED;
    for (int i = 0; i < n; ++i) {
        const agp_conv_desc* c = descs + i;
        // (the five extra terms: this entry validates them, the group route of agp_conv2d_fwd_grouped does not)
        if (!s2_conv_ok(c, descs) || c->w_lo || c->res_lo || c->hi_only || c->hin <= 0 || c->win <= 0) return AGP_E_UNSUPPORTED;
    }
    IgemmParams ps[2];
    const int rc = conv_fill_group(descs, n, ps, false);
    return rc != AGP_OK ? rc : agp_internal_conv_s2(ps, descs, n, (hipStream_t)stream, nullptr, true);
}

// ---- 3x3 / stride-1 groups whose problems may compute their residual from a second operand stream (include/agplace_hip.h)
extern "C" int agp_conv2d_fwd_grouped2(const agp_conv_desc* descs, const agp_conv_stream2* s2, int n, void* stream) {
    if (!descs || !s2) return AGP_E_BADARG;
    if (n < 1 || n > 4 || AGP_TUNE("CONV_KERNEL", 0) || !AGP_TUNE("KXR_WIDE", 1)) return AGP_E_UNSUPPORTED;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const agp_conv_desc* d = descs + i;
        // (the extra terms: the wide kernel's 128-column tiles; w_lo and hi_only, which agp_conv2d_fwd_grouped does not look at)
        if (!kxr2_member_ok(d, descs) || d->w_lo || d->hi_only || d->cout % 128) return AGP_E_UNSUPPORTED;
        const agp_conv_stream2* t = s2 + i;
        if (!t->in_hi) continue;
        any = true;
        if (!t->w_cm || d->res_hi || d->pool_partial || t->n != d->n || t->cin <= 0 || t->cin % 32 || t->hin <= 0 || t->win <= 0 ||
            (t->hin - 1) / 2 + 1 != d->hout || (t->win - 1) / 2 + 1 != d->wout || !fits_31(t->n, t->hin, t->win, t->cin))
            return AGP_E_UNSUPPORTED;
    }
    IgemmParams ps[4];
    KxrwStreams ds = {};
    const int rc = conv_fill_group(descs, n, ps, true);
    if (rc != AGP_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const agp_conv_stream2* t = s2 + i;
        if (!t->in_hi) continue;
        const int wp = t->win + 2, hp = t->hin + 2;
        KxrwStream& k = ds.s[i];
        k.x = t->in_hi; k.w = t->w_cm;
        k.x_bytes = (uint32_t)((int64_t)t->n * hp * wp * t->cin * 2);
        k.w_bytes = (uint32_t)((int64_t)t->cin * descs[i].cout * 2);
        // raster row (img, y, xq) of the output reads input pixel (2 y, 2 (xq - 1)) = padded pixel (2 y + 1, 2 xq - 1)
        k.sn = hp * wp * t->cin; k.sh = 2 * wp * t->cin; k.sw = 2 * t->cin; k.base = (wp - 1) * t->cin;
        k.nc = t->cin / 32;
    }
    return agp_internal_conv_kxrw(ps, n, (hipStream_t)stream, nullptr, any ? &ds : nullptr);
}

// ---- packed 7x7/2 stem conv + BatchNorm + ReLU + MaxPool2d(3, 2, 1) in one kernel (fp16 maps).
// `d` describes the stem conv as for agp_conv2d_fwd (cin = 32, in_w_step = 4, kw = 1, stride 2, pad 3,
// cout = 64, relu = 1) except that out_* is the POOLED map [n][hp2][wp2][64] with halo d->pout and
// hout / wout are the POOLED sizes.
static int stem_pool_impl(const agp_conv_desc* d, int kind, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int ncam,
                          const float* mean3, const float* std3, void* stream) {
    if (!d || !d->in_hi || !d->w_hi || !d->out_hi || d->in_lo || d->out_lo || d->res_hi) return AGP_E_BADARG;
    if (d->prec != AGP_PREC_F16W2 && d->prec != AGP_PREC_F16) return AGP_E_BADARG;
    if (d->prec == AGP_PREC_F16W2 && !d->w_lo) return AGP_E_BADARG;
    if (d->cin != 32 || d->in_w_step != 4 || d->kw != 1 || d->kh != 7 || d->stride != 2 || d->pad != 3 || d->pin != 3 ||
        d->cout != 64 || !d->relu || d->n <= 0)
        return AGP_E_BADARG;
    const int h1 = (d->hin + 2 * 3 - 7) / 2 + 1, w1 = (d->win + 2 * 3 - 7) / 2 + 1;
    const int h2 = (h1 + 2 - 3) / 2 + 1, w2 = (w1 + 2 - 3) / 2 + 1;
    if (d->hout != h2 || d->wout != w2) return AGP_E_BADARG;
    IgemmParams p = {};
    const int hp = d->hin + 6, wp = d->win + 6;
    const int64_t x_elems = (int64_t)d->n * hp * wp * 4;
    const int64_t w_elems = (int64_t)64 * 7 * 32;
    if (kind == 0 && x_elems * 2 >= (1ll << 32)) return AGP_E_BADARG;
    p.x_hi = d->in_hi; p.x_lo = nullptr; p.x_bytes = (uint32_t)(x_elems * 2);
    p.w_hi = d->w_hi; p.w_lo = d->w_lo; p.w_bytes = (uint32_t)(w_elems * 2);
    p.M = d->n * h1 * w1; p.N = 64; p.Ktot = 7 * 32; p.KW = 1; p.CK = 32; p.ntaps = 7;
    p.d_howo = make_fastdiv((uint32_t)(h1 * w1)); p.d_wo = make_fastdiv((uint32_t)w1);
    p.x_sw = 4; p.x_sh = wp * 4; p.x_sn = hp * wp * 4; p.x_base = 0; p.sy = 2; p.sx = 2;
    const int hop = h2 + 2 * d->pout, wop = w2 + 2 * d->pout;
    p.o_hi = d->out_hi; p.o_lo = nullptr;
    p.o_sw = 64; p.o_sh = wop * 64; p.o_sn = hop * wop * 64; p.o_base = (d->pout * wop + d->pout) * 64;
    p.scale = d->scale; p.shift = d->shift; p.relu = 1;
    p.pool_h1 = h1; p.pool_w1 = w1; p.pool_h2 = h2; p.pool_w2 = w2;
    p.pool_ty = (h2 + 6) / 7; p.pool_tx = (w2 + 6) / 7;
    if (kind == 0) return agp_internal_conv_d16_pool(p, d->prec, (hipStream_t)stream);
    if (d->prec != AGP_PREC_F16) return AGP_E_BADARG;
    if (kind == 2 && (ncam <= 0 || d->win % ncam)) return AGP_E_BADARG;
    return agp_internal_stem_raw(p, kind, d->in_hi, sn, sc, sh, sw, d->hin, d->win, ncam, mean3, std3, (hipStream_t)stream);
}

extern "C" int agp_stem_pool_fwd(const agp_conv_desc* d, void* stream) {
    return stem_pool_impl(d, 0, 0, 0, 0, 0, 1, nullptr, nullptr, stream);
}

extern "C" int agp_stem_pool_raw_fwd(const agp_conv_desc* d, int kind, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int ncam,
                                     const float* mean3, const float* std3, void* stream) {
    if (kind != 1 && kind != 2) return AGP_E_BADARG;
    return stem_pool_impl(d, kind, sn, sc, sh, sw, ncam, mean3, std3, stream);
}
