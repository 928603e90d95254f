// Where a zone_detect kernel (feed.hip detect_convert, zone_stitch.hip, zone_metrics.hip) or tta.hip's accumulate reads the logits of ONE window pixel:
// the kernels are templated on one of these and call src(c) once per class, everything after that load is shared text.
//   FullLogits     fp32 NCHW (B, C, S, S): the value stored at the pixel
//   QuarterLogits  fp32 NCHW (B, C, S/4, S/4), what the HuggingFace-provider models' classifiers write: the value
//                  bilinear_nchw_f32_kernel (segformer_ops.hip) would store at the pixel for a x4 resize, operation for operation
//                  (same bilinear_src text, same four-term expression), so the tile-sized fp32 tensor is never written.  The
//                  coordinates are computed once per pixel; per class it is four taps of a plane 16x smaller, which neighbouring
//                  lanes share (a wave's taps fall in one or two 64-byte rows).  Index arithmetic inside a window is 32-bit:
//                  C * (S/4)^2 <= 32 * 512^2.
//                  The files that instantiate it are built with -fno-slp-vectorize (build.py SOURCE_FLAGS says why).
#pragma once
#include "bilinear_src.h"

namespace flair {

struct FullLogits {
  static constexpr int UP = 1;
  const float* p;
  long SS;
  __device__ __forceinline__ FullLogits(const float* logits, int b, int C, int S, long SS_, int i, int j)
      : p(logits + (long)b * C * SS_ + (long)i * S + j), SS(SS_) {}
  // the same pixel for a caller that already holds pix = i * S + j, or the pixel's address in plane 0
  __device__ __forceinline__ FullLogits(const float* logits, int b, int C, int, long SS_, int, int, long pix)
      : p(logits + (long)b * C * SS_ + pix), SS(SS_) {}
  __device__ __forceinline__ FullLogits(const float* pixel, long SS_) : p(pixel), SS(SS_) {}
  __device__ __forceinline__ float operator()(int c) const { return p[(long)c * SS]; }
};

struct QuarterLogits {
  static constexpr int UP = 4;
  const float* p;
  int plane, o00, o01, o10, o11;
  float ly, lx;
  __device__ __forceinline__ QuarterLogits(const float* logits, int b, int C, int S, long SS_, int i, int j, long)
      : QuarterLogits(logits, b, C, S, SS_, i, j) {}
  __device__ __forceinline__ QuarterLogits(const float* logits, int b, int C, int S, long, int i, int j) {
    const int s = S >> 2;
    plane = s * s;
    p = logits + (long)b * C * plane;
    int y0, y1, x0, x1;
    bilinear_src(i, s, S, y0, y1, ly);
    bilinear_src(j, s, S, x0, x1, lx);
    o00 = y0 * s + x0; o01 = y0 * s + x1; o10 = y1 * s + x0; o11 = y1 * s + x1;
  }
  __device__ __forceinline__ float operator()(int c) const {
    const float* q = p + c * plane;
    return (1.f - ly) * ((1.f - lx) * q[o00] + lx * q[o01]) + ly * ((1.f - lx) * q[o10] + lx * q[o11]);
  }
};

}  // namespace flair
