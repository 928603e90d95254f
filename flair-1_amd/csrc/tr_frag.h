// MFMA operand fragments whose K dimension is the PIXEL index of a pixel-major LDS image (the weight-gradient products of
// wgrad_halo.hip and bwd_halo16.hip): bf16 through ds_read_b64_tr_b16, fp32 by dword reads.
#pragma once
#include "common.h"

namespace flair {

template <typename T> struct HFrag;
template <> struct HFrag<bf16_t> {
  static constexpr int KSTEP = 32;  // pixels per MFMA
  // 16 columns starting at byte cb, rows row0 + 0..31 (row stride STRIDE bytes)
  template <int STRIDE>
  __device__ static __forceinline__ u32x4 load(const unsigned char* img, int row0, int cb, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    typedef __attribute__((address_space(3))) s16x4_t* lds_p;
    // pixel -> K-slot map: the `lo` read takes the even pixels of the lane group's eight, the `hi` read the odd ones.  A
    // 32-lane half then reads eight rows 2 * STRIDE apart: with STRIDE = 48 or 80 bytes they fall on disjoint bank octets
    // (rows q, q + 4 put two rows on half of the banks: SQ_LDS_BANK_CONFLICT was half of SQ_LDS_IDX_ACTIVE, and the LDS was
    // active 45-62 % of these kernels' time).  Both operands use the same map, the products are unchanged.
    s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(img + (row0 + 8 * g + 2 * q) * STRIDE + cb + 8 * p));
    s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(img + (row0 + 8 * g + 2 * q + 1) * STRIDE + cb + 8 * p));
    u32x4 r;
    r.x = (unsigned)(unsigned short)lo[0] | ((unsigned)(unsigned short)lo[1] << 16);
    r.y = (unsigned)(unsigned short)lo[2] | ((unsigned)(unsigned short)lo[3] << 16);
    r.z = (unsigned)(unsigned short)hi[0] | ((unsigned)(unsigned short)hi[1] << 16);
    r.w = (unsigned)(unsigned short)hi[2] | ((unsigned)(unsigned short)hi[3] << 16);
    return r;
  }
};
template <> struct HFrag<float> {
  static constexpr int KSTEP = 16;
  template <int STRIDE>
  __device__ static __forceinline__ u32x4 load(const unsigned char* img, int row0, int cb, int lane) {
    const int g = lane >> 4, i = lane & 15;
    u32x4 r;
    r.x = *reinterpret_cast<const unsigned*>(img + (row0 + g) * STRIDE + cb + 4 * i);
    r.y = *reinterpret_cast<const unsigned*>(img + (row0 + 4 + g) * STRIDE + cb + 4 * i);
    r.z = *reinterpret_cast<const unsigned*>(img + (row0 + 8 + g) * STRIDE + cb + 4 * i);
    r.w = *reinterpret_cast<const unsigned*>(img + (row0 + 12 + g) * STRIDE + cb + 4 * i);
    return r;
  }
};

}  // namespace flair
