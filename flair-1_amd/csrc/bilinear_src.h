// The source coordinate of a bilinear resize, one text for every kernel that resamples (segformer_ops.hip, swin_ops.hip) and for
// the zone_detect kernels that interpolate quarter-resolution logits in registers (logit_source.h): they must agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace flair {

// nn.functional.interpolate(mode='bilinear', align_corners=False): src = max(0, (dst + 0.5) * in / out - 0.5)
__device__ __forceinline__ void bilinear_src(int dst, int in, int out, int& i0, int& i1, float& l1) {
  float s = ((float)dst + 0.5f) * ((float)in / (float)out) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

}  // namespace flair
