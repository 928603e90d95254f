// Fused backward of a 3x3 / stride-1 / pad-1 convolution with 16 input and 16 (padded) output channels in bf16
// (bwd_halo16.hip): data gradient + fused BatchNorm-backward sums of the upstream unit + weight gradient (+ bias gradient)
// from ONE staging of the output gradient and of the lazy layer input per 8x32 tile.
#pragma once
#include "common.h"

namespace flair {

struct Bwd16Args {
  // output gradient [N][H][W][16].  Head flavour (gy == nullptr): `g` is the gradient as it stands.  Unit flavour: `g` is the
  // gradient w.r.t. the unit's ReLU output, `gy` the unit's pre-BatchNorm tensor, and the kernel stages
  //   dy = T(fmaf(k1, d, fmaf(k2, y, k3))),  d = fmaf(y, gmsc, gmsh) > 0 ? g : 0     (bn_bwd_apply_kernel, mask from y)
  const void* g;
  const void* gy;
  const float* gcoef;   // k1 | k2 | k3, 16 floats each (bn_bwd_finalize_kernel)
  const float* gmsc;
  const float* gmsh;
  // layer input: the producing unit's pre-BatchNorm tensor [N][H][W][16], consumed as relu(x * in_scale + in_shift)
  const void* x;
  const float* in_scale;
  const float* in_shift;
  const void* w;        // flipped / transposed data-gradient pack [16][Kpad]
  int Kpad;
  void* dx;             // [N][H][W][16]
  // BatchNorm-backward sums of the unit that produced x: sum(dx * m), sum(dx * m * x), m = fmaf(x, bnr_scale, bnr_shift) > 0,
  // as [2][bnr_C][bnr_cols] partials.  bnr_cols is the launch grid (one column per workgroup) or the tile count (one per tile:
  // the layout the separate data-gradient kernel leaves when it runs one tile per workgroup)
  const float* bnr_scale;
  const float* bnr_shift;
  float* bnr_partial;
  int bnr_C, bnr_cols;
  float* slabs;         // [grid][16][144] fp32, one slab per workgroup
  float* dw;            // OIHW fp32 [Cout][Cin_real][3][3]
  int Cout, Cin_real;
  float* dbias;         // optional [Cout] (head flavour) with dbias_partial [16][WGRAD_DBIAS_ROWS]
  float* dbias_partial;
  int N, H, W;
  int grid;             // workgroups: bwd16_grid()
};

// tune key FLAIR_BWD16_FUSE: 0 = the three separate kernels, 1 = both flavours fused, 2 = the head only, 3 = the unit only.
// Default 3: the unit flavour alone is a gain of more than three times the run-to-run spread, the head flavour alone is not
// (2.6 times; profiles/bwd16_fuse.json)
constexpr int FLAIR_BWD16_FUSE_DEFAULT = 3;
enum { BWD16_HEAD = 0, BWD16_UNIT = 1 };
// `a` / `w`: the data gradient (reduction attached) and the weight gradient the separate path would launch
bool bwd16_fusable(int dtype, int flavour, const ConvArgs& a, const WgradArgs& w);
// workgroups = slabs = bias-partial rows.  Default: the grid of the separate weight gradient `w` (wgrad3x3_halo_kernel's resident
// workgroups), so that tiles are dealt to workgroups, and every per-workgroup fp32 sum is formed, exactly as in the separate path:
// the step computes the same bits with the fused kernel on or off.  The kernel itself fits two workgroups per CU where that grid
// counts three, so a third of it runs as a second round.  FLAIR_BWD16_WGS > 0 sets another total (at most one per tile).
int bwd16_grid(const WgradArgs& w);
size_t bwd16_workspace_bytes(int grid);   // the slabs
int launch_bwd16(const Bwd16Args& a, hipStream_t s);   // kernel, slab reduce and bias-partial sum, all on s

}  // namespace flair
