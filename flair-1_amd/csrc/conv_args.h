// Builders of the launch descriptors: a layer's geometry is written down here once, and the executors (unet.hip, tf_exec.hip) and
// the operator entry points (capi.hip) describe their launches through it.  A builder zeroes the descriptor and fills the geometry;
// the caller then sets what is its own (packed weight, outputs, epilogue options, accumulate, bnr_*, cus, fuse_*, dbias).
// The parity-class rewrite of a stride-2 data gradient is conv_parity_args (parity_pack.h).
#pragma once
#include <string.h>

#include "common.h"

namespace flair {

// input of a convolution: [nearest-x2 upsample of x0 if up0] ++ x1 along the channels; x0 is stored [N][H][W][C0]
struct ConvInput {
  const void* x0; const void* x1;
  int C0, C1, up0;
  int N, H, W;
};

inline int conv_out_extent(int Hin, int R, int stride, int pad) { return (Hin + 2 * pad - R) / stride + 1; }
inline int conv_kpad(int dtype, int Kg) { return (int)round_up(Kg, dtype == DT_F32 ? 32 : 64); }   // whole K steps of the kernels

// forward convolution R x R / stride / pad to Cout channels
inline void conv_fwd_args(ConvArgs& a, int dtype, const ConvInput& in, int R, int stride, int pad, int Cout) {
  memset(&a, 0, sizeof(a));
  a.src0 = in.x0; a.src1 = in.x1; a.C0 = in.C0; a.C1 = in.C1; a.up0 = in.up0;
  a.N = in.N; a.Hin = in.up0 ? 2 * in.H : in.H; a.Win = in.up0 ? 2 * in.W : in.W;
  a.Hout = conv_out_extent(a.Hin, R, stride, pad); a.Wout = conv_out_extent(a.Win, R, stride, pad);
  a.R = R; a.S = R; a.out_mul = stride; a.pad = pad; a.in_div = 1;
  a.Cout = Cout;
  a.Kg = R * R * (in.C0 + in.C1); a.Kpad = conv_kpad(dtype, a.Kg);
}

// data gradient of a forward layer R x R / stride / pad in gather form: a convolution over dy (the layer's output gradient)
// with the flipped / transposed pack, to the Cin channels and Hx x Wx pixels of the layer's input
inline void conv_dgrad_args(ConvArgs& a, int dtype, const ConvInput& dy, int R, int stride, int pad, int Hx, int Wx, int Cin) {
  conv_fwd_args(a, dtype, dy, R, 1, R - 1 - pad, Cin);
  a.in_div = stride;
  a.Hout = Hx; a.Wout = Wx;
}

// weight gradient of the forward layer over `in`; dy rows of dy_ld stored channels, the first Cout used
inline void wgrad_args(WgradArgs& w, const ConvInput& in, int R, int stride, int pad, const void* dy, int dy_ld, int Cout, float* dw,
                       int Cin_real) {
  memset(&w, 0, sizeof(w));
  w.x0 = in.x0; w.x1 = in.x1; w.C0 = in.C0; w.C1 = in.C1; w.up0 = in.up0;
  w.N = in.N; w.Hin = in.up0 ? 2 * in.H : in.H; w.Win = in.up0 ? 2 * in.W : in.W;
  w.Hout = conv_out_extent(w.Hin, R, stride, pad); w.Wout = conv_out_extent(w.Win, R, stride, pad);
  w.R = R; w.S = R; w.stride = stride; w.pad = pad;
  w.dy = dy; w.dy_ld = dy_ld; w.Cout = Cout; w.dw = dw; w.Cin_real = Cin_real;
}

}  // namespace flair
