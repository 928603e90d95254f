// Parity classes of a 3x3 / stride-2 / pad-1 data gradient: output pixel (2 ho + py, 2 wo + px) of dX only receives the taps of its
// parity, so the gradient splits into four stride-1 convolutions over dY with 1, 2, 2 and 4 of the nine taps (class = 2 py + px).
// One place for the geometry and the tap subsets of the four packed copies: the network's arena plan and pack table
// (UNet::begin, UNet::pack_dgrad_weights) and the operator entry point (flair_conv2d_ex, mode 2) both call it.
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

}  // namespace flair
