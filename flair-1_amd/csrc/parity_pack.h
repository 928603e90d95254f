// Parity classes of a 3x3 / stride-2 / pad-1 data gradient: output pixel (2 ho + py, 2 wo + px) of dX only receives the taps of its
// parity, so the gradient splits into four stride-1 convolutions over dY with 1, 2, 2 and 4 of the nine taps (class = 2 py + px).
// One place for the geometry, the tap subsets of the four packed copies and the launch descriptor: the network's arena plan,
// pack table and data gradient (UNet::begin, UNet::pack_dgrad_weights, UNet::unit_backward) and the operator entry point
// (flair_conv2d_ex, mode 2) all call it.
#pragma once
#include "ops.h"

namespace flair {

// K extent of class `cls` for dY rows of Cout_p stored channels: real (Kg) and padded to the K step of `dtype` (Kpad)
inline void parity_class_geom(int dtype, int Cout_p, int cls, int& Kg, int& Kpad) {
  const int kstep = dtype == DT_F32 ? 32 : 64;
  const int taps = ((cls >> 1) ? 2 : 1) * ((cls & 1) ? 2 : 1);
  Kg = taps * Cout_p;
  Kpad = (int)round_up(Kg, kstep);
}

// pack descriptor of class `cls`, derived from the layer's full transposed (data-gradient) descriptor
inline PackDesc parity_class_pack(const PackDesc& full, int cls, size_t dst_off, int Kpad) {
  // gather-form tap kr reads dY row (ho - 1 + kr) / 2: even output rows use kr = 1, odd rows kr = 0 and 2
  PackDesc e = full;
  e.dst_off = dst_off; e.Kpad = Kpad;
  const int py = cls >> 1, px = cls & 1;
  e.Rc = py ? 2 : 1; e.r0 = py ? 0 : 1; e.rstep = 2;
  e.Sc = px ? 2 : 1; e.s0 = px ? 0 : 1; e.sstep = 2;
  return e;
}

// Rewrite `a`, the gather-form data gradient (conv_dgrad_args) of an R x R stride-2 layer whose input is twice its output in
// both extents, by output parity class: stride-1 convolutions over dY, stores interleaved into dX (out_sub).  R == 3: the four
// classes (1, 2, 2 and 4 taps) ride in one launch, class = blockIdx.z; their packs (a.cls_w, a.w = the class-3 pack) are the
// caller's.  A 1x1 layer only reaches the (even, even) pixels: one class, the layer's own pack.
inline void conv_parity_args(ConvArgs& a, int dtype, int R) {
  a.Hout = a.Hin; a.Wout = a.Win; a.out_mul = 1; a.pad = 0; a.in_div = 1; a.out_sub = 1;
  if (R != 3) return;
  a.ncls = 4; a.R = 2; a.S = 2;
  int kg[4];
  for (int cls = 0; cls < 4; ++cls) parity_class_geom(dtype, a.C0, cls, kg[cls], a.cls_kpad[cls]);
  a.Kg = (kg[0] + kg[1] + kg[2] + kg[3]) / 4;   // mean over the classes (work accounting only)
  a.Kpad = a.cls_kpad[3];
}

}  // namespace flair
