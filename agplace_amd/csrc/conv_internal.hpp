// The host entry points that one conv translation unit calls in another, each declared here once; every .hip that defines or
// calls one includes this header.  `plan` != NULL: fill the tile plan from the launcher's own grid arithmetic and return before
// anything touches the device (igemm_params.hpp TilePlan).
#pragma once
#include "igemm_params.hpp"

// igemm.hip, the generic LDS-staged kernel: one conv; 2..4 fp16 single-product convs of one tile configuration as one grid
int agp_internal_conv_generic(agp_igemm::IgemmParams& p, int prec, hipStream_t s, agp_igemm::TilePlan* plan);
int agp_internal_conv_generic_group(agp_igemm::IgemmParams* ps, int n, hipStream_t s, agp_igemm::TilePlan* plan);
// igemm_d16.hip, the direct-X kernel (packed stem); the stem fused with its max-pool, from packed / from raw input
int agp_internal_conv_d16(agp_igemm::IgemmParams& p, int prec, hipStream_t s, agp_igemm::TilePlan* plan);
int agp_internal_conv_d16_pool(agp_igemm::IgemmParams& p, int prec, hipStream_t s);
int agp_internal_stem_raw(agp_igemm::IgemmParams& p, int kind, const void* x, long long sn, long long sc, long long sh, long long sw,
                          int h, int w, int ncam, const float* mean3, const float* std3, hipStream_t s);
// stem_walk.hip
int agp_internal_stem_walk(agp_igemm::IgemmParams& p, int kind, agp_igemm::StemRaw raw, hipStream_t s);
bool agp_internal_stem_walk_reads(const agp_igemm::StemRaw& raw, int n);
bool agp_internal_stem_walk_reads_u8(const agp_igemm::StemRaw& raw, int n);
// igemm_kxr.hip, 3x3 / stride 1 / pad 1 on 1-pixel-halo planes: the conv, its raster, whether igemm_kxr2 / igemm_kxrw take `d`
int agp_internal_conv_kxr(agp_igemm::IgemmParams& p, const agp_conv_desc* d, hipStream_t s, agp_igemm::TilePlan* plan);
void agp_internal_conv_kxr_geometry(agp_igemm::IgemmParams& p, const agp_conv_desc* d);
bool agp_internal_use_kxr2(const agp_conv_desc* d);
// igemm_kxr2.hip, igemm_kxrw.hip: 1..4 such convs of one channel shape, fp16 with one product, as one grid
int agp_internal_conv_kxr2(agp_igemm::IgemmParams* ps, int n, hipStream_t s, agp_igemm::TilePlan* plan);
int agp_internal_conv_kxrw(agp_igemm::IgemmParams* ps, int n, hipStream_t s, agp_igemm::TilePlan* plan, const agp_igemm::KxrwStreams* ds);
// igemm_s2.hip: the stage entry (3x3 / stride 2, with or without its 1x1 / stride-2 downsample) of 1..2 trunks
int agp_internal_conv_s2(agp_igemm::IgemmParams* ps, const agp_conv_desc* descs, int n, hipStream_t s, agp_igemm::TilePlan* plan, bool nods);
