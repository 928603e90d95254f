// Which kernel family serves a convolution: decided once, by conv_family() (conv_igemm.hip).  launch_conv and its refusals,
// conv_grid_rows (the statistics and fused BatchNorm-backward partials are sized from it), conv_tile_epilogue_ok,
// conv_mfma_bound and conv_acc_src_ok all ask it, so they cannot disagree.  Also the one place where the per-family
// predicates, row counts and launchers that live next to their kernels are declared.
#pragma once
#include "common.h"

namespace flair {

enum ConvFamily { CONV_STEM, CONV_HG, CONV_HALO, CONV_GATHER };   // stem.hip, conv_hg.hip, conv_halo.hip, conv_igemm.hip
// Pure function of the arguments: the first family, in the order above, whose *_applicable test passes.  A lazy BatchNorm + ReLU
// input (in_scale) is part of those tests (the stem refuses it, the halo-GEMM knows which of its kernels apply it).
ConvFamily conv_family(int dtype, const ConvArgs& a);
// true when launch_conv will pick a halo-tile kernel whose epilogue implements pool_c0 / out_skip
bool conv_tile_epilogue_ok(int dtype, const ConvArgs& a);
int conv_weight_rows_pad(int cout);   // rows of a packed weight: Cout up to whole column tiles of the gather-form kernel

bool conv_stem_applicable(int dtype, const ConvArgs& a);
int conv_stem_grid_rows(const ConvArgs& a);
int launch_conv_stem(const ConvArgs& a, hipStream_t s);
bool conv_hg_applicable(int dtype, const ConvArgs& a);
int conv_hg_grid_rows(int dtype, const ConvArgs& a);
int launch_conv_hg(int dtype, const ConvArgs& a, hipStream_t s);
bool conv_halo_applicable(const ConvArgs& a);
bool conv_halo_bnr_applicable(const ConvArgs& a);
int conv_halo_grid_rows(int dtype, const ConvArgs& a);
int launch_conv_halo(int dtype, const ConvArgs& a, hipStream_t s);

// the weight-gradient families launch_wgrad and wgrad_workspace_bytes walk (wgrad.hip): stem.hip, wgrad_hg.hip, wgrad_halo.hip
bool wgrad_stem_applicable(int dtype, const WgradArgs& a);
size_t wgrad_stem_workspace_bytes(const WgradArgs& a);
int launch_wgrad_stem(const WgradArgs& a, hipStream_t s);
bool wgrad_big_applicable(int dtype, const WgradArgs& a);
size_t wgrad_big_workspace_bytes(int dtype, const WgradArgs& a);
int launch_wgrad_big(int dtype, const WgradArgs& a, hipStream_t s);
bool wgrad_halo_applicable(const WgradArgs& a);
size_t wgrad_halo_workspace_bytes(int dtype, const WgradArgs& a);
int launch_wgrad_halo(int dtype, const WgradArgs& a, hipStream_t s);

}  // namespace flair
