// Test-time augmentation over the D4 group the network is trained under (DESIGN §10 "Test-time augmentation"): the mean of the class
// probabilities over a list of transform codes (csrc/d4.h), as one permutation kernel in front of each forward and one accumulate
// kernel behind it.
//   d4_nchw       out = T(in) for fp32 NCHW, out of place: a pure permutation.
//   tta_accum     one pass of the ensemble: softmax of the transformed-frame logits at (i, j), added into the fp32 (B, C, H, W) sum at
//                 the original-frame pixel T sends there.  `first` stores instead of adding (no memset); the last pass (preds given)
//                 finishes the sum in registers and writes the uint8 class (lowest index of the largest sum) and, optionally, largest
//                 sum / n -- the sum itself is not written then, so no probability tensor ever is.
// Both kernels give each 256-thread block a 32 x 32 pixel tile of the ORIGINAL frame (of the output, for d4_nchw), two rows of 32 lanes per wave: under an odd
// rot90 count one side of the permutation walks columns, and over such a tile both sides still touch whole 128-byte row segments
// (32 rows x 128 B read or written by the block, each byte of them used).  The inverse mapping is a permutation of pixels: no atomics,
// the sum at a pixel is the same sequence of fp32 additions on every run.
#include "d4.h"
#include "logit_source.h"
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

constexpr int TILE = 32;

__global__ __launch_bounds__(256) void d4_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, long planes, int H, int W,
                                                      int code) {
  const int tj_n = (W + TILE - 1) / TILE, ti_n = (H + TILE - 1) / TILE;
  const long per_plane = (long)ti_n * tj_n, total = per_plane * planes, HW = (long)H * W;
  const int lj = threadIdx.x & (TILE - 1), li = threadIdx.x >> 5;
  for (long t = blockIdx.x; t < total; t += gridDim.x) {
    const long pl = t / per_plane;
    const int r = (int)(t - pl * per_plane);
    const int i0 = (r / tj_n) * TILE, j = (r % tj_n) * TILE + lj;
    if (j >= W) continue;
    const float* src = in + pl * HW;
    float* dst = out + pl * HW;
#pragma unroll
    for (int e = 0; e < TILE / 8; ++e) {
      const int i = i0 + li + 8 * e;
      if (i >= H) break;
      int si, sj;
      d4_source(code, i, j, H, W, si, sj);
      dst[(long)i * W + j] = src[(long)si * W + sj];
    }
  }
}

// SRC (logit_source.h): FullLogits reads (B, C, H, W); QuarterLogits interpolates (B, C, H/4, W/4) x4 in registers (H == W)
template <class SRC, int CM>
__global__ __launch_bounds__(256) void tta_accum_kernel(const float* __restrict__ logits, int B, int C, int H, int W, int code, int first,
                                                        float* __restrict__ acc, unsigned char* __restrict__ preds,
                                                        float* __restrict__ prob, float n) {
  const int tj_n = (W + TILE - 1) / TILE, ti_n = (H + TILE - 1) / TILE;
  const long per_img = (long)ti_n * tj_n, total = per_img * B, HW = (long)H * W;
  const int lj = threadIdx.x & (TILE - 1), li = threadIdx.x >> 5;
  for (long t = blockIdx.x; t < total; t += gridDim.x) {
    const int b = (int)(t / per_img);
    const int r = (int)(t - (long)b * per_img);
    const int si0 = (r / tj_n) * TILE, sj = (r % tj_n) * TILE + lj;
    if (sj >= W) continue;
    for (int e = 0; e < TILE / 8; ++e) {
      const int si = si0 + li + 8 * e;
      if (si >= H) break;
      int i, j;
      d4_dest(code, si, sj, H, W, i, j);   // the pixel of the transformed frame that shows original pixel (si, sj)
      const SRC src(logits, b, C, W, HW, i, j);
      float v[CM];
      float m = -INFINITY;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) { v[c] = src(c); m = fmaxf(m, v[c]); }
      float ssum = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) { v[c] = expf(v[c] - m); ssum += v[c]; }
      const long o = (long)si * W + sj;
      float* a = acc ? acc + (long)b * C * HW + o : nullptr;
      int best = 0;
      float pbest = -1.f;
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) {
          float q = v[c] / ssum;
          if (!first) q = a[(long)c * HW] + q;
          if (preds) {
            if (q > pbest) { pbest = q; best = c; }
          } else {
            a[(long)c * HW] = q;
          }
        }
      if (preds) {
        preds[(long)b * HW + o] = (unsigned char)best;
        if (prob) prob[(long)b * HW + o] = pbest / n;
      }
    }
  }
}

inline int tile_blocks(long tiles) {
  const long cap = 256L * 64;
  return (int)(tiles < 1 ? 1 : (tiles > cap ? cap : tiles));
}

inline long tiles_of(int H, int W) { return (long)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE); }

inline bool d4_code_ok(int code, int H, int W) { return code >= 0 && code <= 15 && (!(code & 4) || H == W); }

template <class SRC>
void launch_accum(const float* logits, int B, int C, int H, int W, int code, int first, float* acc, unsigned char* preds, float* prob, int n,
                  hipStream_t s) {
  auto kern = C <= 16 ? tta_accum_kernel<SRC, 16> : tta_accum_kernel<SRC, 32>;
  hipLaunchKernelGGL(kern, dim3(tile_blocks(tiles_of(H, W) * B)), dim3(256), 0, s, logits, B, C, H, W, code, first, acc, preds, prob,
                     (float)n);
}

}  // namespace

int d4_nchw_f32(const float* in, float* out, int B, int C, int H, int W, int code, hipStream_t s) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || code < 0 || code > 15) return -2;
  if (!d4_code_ok(code, H, W)) return -19;
  const long planes = (long)B * C;
  ProfScope ps("d4_nchw", 0.0, (double)planes * H * W * 8.0, s);
  hipLaunchKernelGGL(d4_nchw_kernel, dim3(tile_blocks(tiles_of(H, W) * planes)), dim3(256), 0, s, in, out, planes, H, W, code);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int tta_accum(const float* logits, int up, int B, int C, int H, int W, int code, int first, float* acc, unsigned char* preds, float* prob,
              int n, hipStream_t s) {
  if (B < 1 || C < 1 || C > 32 || H < 1 || W < 1 || n < 1 || n > 16 || code < 0 || code > 15) return -2;
  if (!d4_code_ok(code, H, W)) return -19;
  if ((up != 1 && up != 4) || (up == 4 && (H != W || H % 4))) return -2;
  if (prob && !preds) return -1;
  if (!acc && !(first && preds)) return -1;   // only a pass that is both first and last leaves the sum alone
  const double px = (double)B * H * W;
  const double bytes = px * (4.0 * C / (up * up) + (first ? 0.0 : 4.0 * C) + (preds ? 1.0 + (prob ? 4.0 : 0.0) : 4.0 * C));
  if (up == 4) {
    ProfScope ps("tta_accum_q4", 0.0, bytes, s);
    launch_accum<QuarterLogits>(logits, B, C, H, W, code, first, acc, preds, prob, n, s);
    FLAIR_CHECK_LAUNCH();
    return 0;
  }
  ProfScope ps("tta_accum", 0.0, bytes, s);
  launch_accum<FullLogits>(logits, B, C, H, W, code, first, acc, preds, prob, n, s);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
