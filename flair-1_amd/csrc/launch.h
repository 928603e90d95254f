// Host side of one kernel launch of the convolution / weight-gradient sources, written once: the dynamic-LDS limit of the kernel
// (raised at its first launch), the profile scope with the launch's algorithmic flops and bytes, the launch and its check.
#pragma once
#include "common.h"
#include "prof.h"

namespace flair {

struct ProfCost { double flops, bytes; };

// Algorithmic cost of a stride-1 convolution launch over elements of es bytes: the MACs, and every operand crossing HBM once
// (src0 at a quarter of the pixels under the fused upsample; the output twice when it accumulates).  c1: the kernel has a second
// source; nchw: it can write the fp32 NCHW copy.
inline ProfCost conv_prof_cost(const ConvArgs& a, size_t es, bool c1, bool nchw) {
  const long M = (long)a.N * a.Hout * a.Wout;
  ProfCost c;
  c.flops = 2.0 * (double)M * a.Cout * a.Kg;
  c.bytes = ((double)M / (a.up0 ? 4 : 1) * a.C0 + (c1 ? (double)M * a.C1 : 0.0) + (double)M * a.Cout * (a.accumulate ? 2 : 1)) * es +
            (double)a.Cout * a.Kg * es + ((nchw && a.out_nchw) ? (double)M * a.Cout * 4.0 : 0.0);
  return c;
}
// a 3x3 weight gradient: dY and X once
template <typename A>
inline ProfCost wgrad3x3_prof_cost(const A& h, size_t es) {
  const double M = (double)h.N * h.H * h.W;
  return ProfCost{2.0 * M * h.Cout * 9.0 * (h.C0 + h.C1), (M * h.dy_ld + M * (h.C0 / (h.up0 ? 4.0 : 1.0) + h.C1)) * es};
}

// Kern: the kernel, a template argument so that every kernel has its own "limit raised" flag
template <auto Kern, typename... Args>
int launch_kernel(const char* name, ProfCost cost, dim3 grid, dim3 block, int smem, hipStream_t s, const Args&... args) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  {
    ProfScope ps(name, cost.flops, cost.bytes, s);
    hipLaunchKernelGGL(Kern, grid, block, smem, s, args...);
  }
  FLAIR_CHECK_LAUNCH();
  return 0;
}

// Workgroups of a persistent kernel that are resident on a CU at once (registers and LDS), asked from the runtime once per kernel
// and capped; `fallback` without a device (planning on a CPU-only host)
template <auto Kern>
int resident_per_cu(int threads, int smem, int fallback, int cap) {
  static const int per_cu = [&] {
    int nb = 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kern, threads, smem) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      return fallback;
    }
    return nb > cap ? cap : nb;
  }();
  return per_cu;
}

}  // namespace flair
