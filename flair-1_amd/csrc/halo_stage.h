// Halo staging shared by the 3x3 / stride-1 / pad-1 kernels that keep an input tile in LDS (conv_halo.hip, conv_hg.hip,
// wgrad_halo.hip): a workgroup of NT threads owns a TW x TH output tile and moves the (TH+2) x (TW+2) input halo, CPP 16-byte
// chunks per pixel, global -> registers (halo_gather, issued early) and registers -> LDS (halo_put, one phase later).  Thread t
// handles the items t + NT * k, item = (halo pixel, chunk) = divmod(item, CPP); pixels outside the image are read from a valid
// address and stored as zeros.  Everything here is forced inline: the callers' lambdas keep their per-kernel state and their
// scheduling fences, and their bodies are one call.  tile_decode also serves the other tile-walking kernels (wgrad_hg.hip,
// stem.hip).  A kernel joins a template here only if its registers, scratch and occupancy stay what they were: where the shared
// form moved them the kernel keeps its own loop (profiles/conv_tile_share.json).
#pragma once
#include "common.h"

namespace flair {

// tile -> image n and the first output row / column of the tile
template <int TW, int TH>
__device__ __forceinline__ void tile_decode(int tile, int tiles_x, int tiles_y, int& n, int& y0, int& x0) {
  n = tile / (tiles_x * tiles_y);
  const int trem = tile - n * tiles_x * tiles_y;
  y0 = (trem / tiles_x) * TH;
  x0 = (trem % tiles_x) * TW;
}

// Where a channel chunk of the concatenated input [up2(src0)] ++ src1 is read from: the tensor, its extent and channel count,
// the coordinate shift of the fused nearest x2 upsample and the chunk's first channel inside that tensor.
template <typename T>
struct HaloSrc {
  const T* __restrict__ base;
  int Hs, Ws, Cs, sh, coff;
};

// the chunk that starts at concatenated channel cbase; H x W is the logical (upsampled) input extent.  use0: it lies in src0
template <typename T>
__device__ __forceinline__ HaloSrc<T> halo_src(const void* src0, const void* src1, int C0, int C1, int up0, int H, int W, int cbase,
                                               bool use0) {
  HaloSrc<T> s;
  s.base = (const T*)(use0 ? src0 : src1);
  s.sh = (use0 && up0) ? 1 : 0;
  s.Hs = H >> s.sh;
  s.Ws = W >> s.sh;
  s.Cs = use0 ? C0 : C1;
  s.coff = use0 ? cbase : cbase - C0;
  return s;
}

// this thread's chunk column of the lazy BatchNorm + ReLU input transform (a thread always stages the same column: NT % CPP == 0);
// c0 = first channel of the staged chunk row in the coefficient vectors
template <typename T, int CPP>
__device__ __forceinline__ void lazy_coef_load(const float* in_scale, const float* in_shift, int c0, int t, float (&lsc)[Elem<T>::CH],
                                               float (&lsh)[Elem<T>::CH]) {
  constexpr int CH = Elem<T>::CH;
#pragma unroll
  for (int e = 0; e < CH; ++e) {
    lsc[e] = in_scale[c0 + (t % CPP) * CH + e];
    lsh[e] = in_shift[c0 + (t % CPP) * CH + e];
  }
}

// global -> registers; hbits bit k: item k is inside the image (and tok: the tile / chunk exists at all)
template <typename T, int TW, int TH, int CPP, int NT, int ITEMS>
__device__ __forceinline__ void halo_gather(const HaloSrc<T>& s, bool tok, int n, int y0, int x0, int H, int W, int t,
                                            u32x4 (&hreg)[ITEMS], unsigned& hbits) {
  constexpr int CH = Elem<T>::CH, HW_ = TW + 2, HPIX = (TH + 2) * HW_;
  static_assert(ITEMS * NT >= HPIX * CPP && ITEMS <= 32, "items cover the halo, one mask bit each");
  unsigned hb = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int it = t + NT * k;
    const int hp = it / CPP, ch = it - hp * CPP;
    const int hy = hp / HW_, hx = hp - hy * HW_;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = tok && (it < HPIX * CPP) && ((unsigned)iy < (unsigned)H) && ((unsigned)ix < (unsigned)W);
    const unsigned off = ok ? (unsigned)(((n * s.Hs + (iy >> s.sh)) * s.Ws + (ix >> s.sh)) * s.Cs + s.coff + ch * CH) : 0u;
    hreg[k] = *reinterpret_cast<const u32x4*>(s.base + off);
    hb |= (ok ? 1u : 0u) << k;
  }
  hbits = hb;
}

// LDS address of (halo pixel hp, chunk ch).  Rows of STRIDE bytes per pixel: conv_halo.hip (HaloCfg::PSTRIDE) and
// wgrad_halo.hip (WgHaloCfg::XSTRIDE), whose paddings serve their different fragment reads.
template <int STRIDE>
struct HaloRows {
  __device__ static __forceinline__ unsigned char* at(unsigned char* halo, int hp, int ch) { return halo + hp * STRIDE + ch * 16; }
};
// 128-byte pixels, the chunk XOR-swizzled with the halo column (conv_hg.hip: the fragment reads of 16 consecutive pixels)
template <int HW_>
struct HaloSwizzle {
  __device__ static __forceinline__ unsigned char* at(unsigned char* halo, int hp, int ch) {
    return halo + hp * 128 + ((ch ^ ((hp % HW_) & 7)) << 4);
  }
};

// registers -> LDS, masked; LZ && lazy: relu(x * lsc + lsh) on the way (chunk_bn_relu, the rounding of bn_act)
template <typename T, int TW, int TH, int CPP, int NT, int ITEMS, typename Layout, bool LZ>
__device__ __forceinline__ void halo_put(unsigned char* halo, int t, const u32x4 (&hreg)[ITEMS], unsigned hbits, bool lazy,
                                         const float* lsc, const float* lsh) {
  constexpr int HPIX = (TH + 2) * (TW + 2);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int it = t + NT * k;
    if (it < HPIX * CPP) {
      const int hp = it / CPP, ch = it - hp * CPP;
      const u32x4 hv = (LZ && lazy) ? chunk_bn_relu<T>(hreg[k], lsc, lsh) : hreg[k];
      *reinterpret_cast<u32x4*>(Layout::at(halo, hp, ch)) = hv & (0u - ((hbits >> k) & 1u));
    }
  }
}

}  // namespace flair
