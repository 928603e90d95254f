// zone_detect's overlap stitching ('average', 'average_weights', 'max'; src/zone_detect/compare.py:84-136 as DESIGN §8
// states its intent): windows slid with a stride shorter than their margin-cropped core, overlaps blended on the device.
//
// Every kernel here is in GATHER form: one thread per output pixel of a rectangle, walking the launch's windows in job order in
// registers, reading its accumulator / output pixel once and writing it once.  No float atomics: the sum at a pixel is the
// same sequence of fp32 operations however the job is cut into batches and launches.
//   blend_accum   softmax of each covering window's logits, w * p per class and w added into a (C+1, H, K) fp32 ring of
//                 K = S - 2m raster columns indexed x mod K (w = 1 for 'average', the Chebyshev-distance table of
//                 patch_weights(S, 0.5, 'exp') for 'average_weights')
//   blend_flush   finished ring columns -> convert('argmax') of sum(w p) / sum(w) into the (2, H, W) raster; zeroes them
//   stitch_max    running (class, probability) per pixel in the (2, H, W) raster; a later window wins unless the past
//                 probability is strictly greater (compare.py:135-136, on the confidence band)
#include "logit_source.h"
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

constexpr int MAXC = 32;

__device__ __forceinline__ bool covers(int v, int o, int S, int margin) { return v >= o + margin && v < o + S - margin; }

// SRC (logit_source.h): FullLogits reads (B, C, S, S); QuarterLogits interpolates (B, C, S/4, S/4) x4 in registers
template <class SRC>
__global__ __launch_bounds__(256) void blend_accum_kernel(const float* __restrict__ logits, int B, int C, int S, int margin,
                                                          const int* __restrict__ tiles, const float* __restrict__ wtab,
                                                          int x_lo, int y_lo, int rw, int rh, float* __restrict__ ring, int Hr) {
  const int K = S - 2 * margin, c0 = S / 2;
  const long total = (long)rw * rh, SS = (long)S * S, plane = (long)Hr * K;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int y = y_lo + (int)(t / rw), x = x_lo + (int)(t % rw);
    float* r = ring + (long)y * K + x % K;
    float acc[MAXC], wsum = 0.f;
    bool any = false;
    for (int b = 0; b < B; ++b) {
      const int x0 = tiles[b * 6 + 0], y0 = tiles[b * 6 + 1];
      if (!covers(x, x0, S, margin) || !covers(y, y0, S, margin)) continue;
      if (!any) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) acc[c] = r[(long)c * plane];
        wsum = r[(long)C * plane];
        any = true;
      }
      const int i = y - y0, j = x - x0;
      const SRC src(logits, b, C, S, SS, i, j);
      float v[MAXC];
      float m = -INFINITY;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) { v[c] = src(c); m = fmaxf(m, v[c]); }
      float ssum = 0.f;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) { v[c] = expf(v[c] - m); ssum += v[c]; }
      const float w = wtab ? wtab[max(abs(i - c0), abs(j - c0))] : 1.f;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) acc[c] += w * (v[c] / ssum);
      wsum += w;
    }
    if (any) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) r[(long)c * plane] = acc[c];
      r[(long)C * plane] = wsum;
    }
  }
}

__global__ __launch_bounds__(256) void blend_flush_kernel(float* __restrict__ ring, int C, int K, int x_lo, int rw, float* __restrict__ out,
                                                          int Hr, int Wr) {
  const long total = (long)rw * Hr, plane = (long)Hr * K;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int y = (int)(t / rw), x = x_lo + (int)(t % rw);
    float* r = ring + (long)y * K + x % K;
    const float wsum = r[(long)C * plane];
    if (!(wsum > 0.f)) continue;  // no window's core reached this pixel: the output keeps its zero fill
    int best = 0;
    float pbest = -1.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C) {
        const float q = r[(long)c * plane] / wsum;
        r[(long)c * plane] = 0.f;
        if (q > pbest) { pbest = q; best = c; }
      }
    r[(long)C * plane] = 0.f;
    const long dst = (long)y * Wr + x;
    out[dst] = (float)best;
    out[(long)Hr * Wr + dst] = pbest;
  }
}

// preds != null: the (class, probability) maps of flair_unet_fwd_opts_t::preds_u8; otherwise softmax + first argmax of the logits
template <class SRC>
__global__ __launch_bounds__(256) void stitch_max_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ preds,
                                                         const float* __restrict__ maxprob, int B, int C, int S, int margin,
                                                         const int* __restrict__ tiles, int x_lo, int y_lo, int rw, int rh,
                                                         float* __restrict__ out, int Hr, int Wr) {
  const long total = (long)rw * rh, SS = (long)S * S, HW = (long)Hr * Wr;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int y = y_lo + (int)(t / rw), x = x_lo + (int)(t % rw);
    const long dst = (long)y * Wr + x;
    float cls = 0.f, prob = 0.f;
    bool any = false;
    for (int b = 0; b < B; ++b) {
      const int x0 = tiles[b * 6 + 0], y0 = tiles[b * 6 + 1];
      if (!covers(x, x0, S, margin) || !covers(y, y0, S, margin)) continue;
      if (!any) { cls = out[dst]; prob = out[HW + dst]; any = true; }
      const long src = (long)(y - y0) * S + (x - x0);
      int best = 0;
      float pbest;
      if (preds) {
        best = preds[(long)b * SS + src];
        pbest = maxprob[(long)b * SS + src];
      } else {
        const SRC lsrc(logits, b, C, S, SS, y - y0, x - x0, src);
        float v[MAXC];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) { v[c] = lsrc(c); m = fmaxf(m, v[c]); }
        float ssum = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) { v[c] = expf(v[c] - m); ssum += v[c]; }
        pbest = -1.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            const float q = v[c] / ssum;
            if (q > pbest) { pbest = q; best = c; }
          }
      }
      if (!(prob > pbest)) { cls = (float)best; prob = pbest; }
    }
    if (any) { out[dst] = cls; out[HW + dst] = prob; }
  }
}

inline int stream_blocks(long items) {
  long b = (items + 255) / 256;
  if (b > 256 * 8) b = 256 * 8;
  return (int)(b < 1 ? 1 : b);
}

inline bool rect_ok(int x_lo, int x_hi, int y_lo, int y_hi, int Hr, int Wr) {
  return Hr >= 1 && Wr >= 1 && 0 <= x_lo && x_lo <= x_hi && x_hi <= Wr && 0 <= y_lo && y_lo <= y_hi && y_hi <= Hr;
}

}  // namespace

int detect_blend_accum(const float* logits, int up, int B, int C, int S, int margin, const int* tiles, const float* wtab, int x_lo, int x_hi,
                       int y_lo, int y_hi, float* ring, int Hr, int Wr, hipStream_t s) {
  if (C < 1 || C > MAXC || B < 1 || margin < 0 || S - 2 * margin < 1 || !rect_ok(x_lo, x_hi, y_lo, y_hi, Hr, Wr)) return -2;
  if (x_hi - x_lo > S - 2 * margin) return -2;  // two columns of the rectangle would share a ring column
  if ((up != 1 && up != 4) || S % up) return -2;
  const long px = (long)(x_hi - x_lo) * (y_hi - y_lo);
  if (px == 0) return 0;
  const long K = S - 2 * margin;
  const double bytes = (double)B * K * K * 4.0 * C / (up * up) + (double)px * 8.0 * (C + 1);
  if (up == 4) {
    ProfScope ps("detect_blend_accum_q4", 0.0, bytes, s);
    hipLaunchKernelGGL(blend_accum_kernel<QuarterLogits>, dim3(stream_blocks(px)), dim3(256), 0, s, logits, B, C, S, margin, tiles, wtab,
                       x_lo, y_lo, x_hi - x_lo, y_hi - y_lo, ring, Hr);
    FLAIR_CHECK_LAUNCH();
    return 0;
  }
  ProfScope ps("detect_blend_accum", 0.0, bytes, s);
  hipLaunchKernelGGL(blend_accum_kernel<FullLogits>, dim3(stream_blocks(px)), dim3(256), 0, s, logits, B, C, S, margin, tiles, wtab, x_lo,
                     y_lo, x_hi - x_lo, y_hi - y_lo, ring, Hr);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int detect_blend_flush(float* ring, int C, int K, int x_lo, int x_hi, float* out, int Hr, int Wr, hipStream_t s) {
  if (C < 1 || C > MAXC || K < 1 || !rect_ok(x_lo, x_hi, 0, Hr, Hr, Wr) || x_hi - x_lo > K) return -2;
  const long px = (long)(x_hi - x_lo) * Hr;
  if (px == 0) return 0;
  ProfScope ps("detect_blend_flush", 0.0, (double)px * (8.0 * (C + 1) + 8.0), s);
  hipLaunchKernelGGL(blend_flush_kernel, dim3(stream_blocks(px)), dim3(256), 0, s, ring, C, K, x_lo, x_hi - x_lo, out, Hr, Wr);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int detect_stitch_max(const float* logits, int up, const unsigned char* preds, const float* maxprob, int B, int C, int S, int margin,
                      const int* tiles, int x_lo, int x_hi, int y_lo, int y_hi, float* out, int Hr, int Wr, hipStream_t s) {
  if ((!preds && (C < 1 || C > MAXC)) || B < 1 || margin < 0 || S - 2 * margin < 1 || !rect_ok(x_lo, x_hi, y_lo, y_hi, Hr, Wr)) return -2;
  if ((up != 1 && up != 4) || S % up || (preds && up != 1)) return -2;
  const long px = (long)(x_hi - x_lo) * (y_hi - y_lo);
  if (px == 0) return 0;
  const long K = S - 2 * margin;
  const double bytes = (double)B * K * K * (preds ? 5.0 : 4.0 * C / (up * up)) + (double)px * 16.0;
  if (up == 4) {
    ProfScope ps("detect_stitch_max_q4", 0.0, bytes, s);
    hipLaunchKernelGGL(stitch_max_kernel<QuarterLogits>, dim3(stream_blocks(px)), dim3(256), 0, s, logits, preds, maxprob, B, C, S, margin,
                       tiles, x_lo, y_lo, x_hi - x_lo, y_hi - y_lo, out, Hr, Wr);
    FLAIR_CHECK_LAUNCH();
    return 0;
  }
  ProfScope ps("detect_stitch_max", 0.0, bytes, s);
  hipLaunchKernelGGL(stitch_max_kernel<FullLogits>, dim3(stream_blocks(px)), dim3(256), 0, s, logits, preds, maxprob, B, C, S, margin, tiles,
                     x_lo, y_lo, x_hi - x_lo, y_hi - y_lo, out, Hr, Wr);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
