// zone_detect's comparison metrics against a ground-truth raster (src/zone_detect/test/metrics.py, main.py:350-366): the
// counts stay on the device next to the stitched raster and the windows' predictions; only (n, C, C) int64 matrices and a
// K x K fp64 map come back to the host, the scores are host arithmetic on those.
//   window_confmat   one C x C matrix per window: confusion_matrix(truth - 1, pred, labels=range(C)) over the window's
//                    margin-cropped core [x0+m, x0+S-m) x [y0+m, y0+S-m); pred from the window's u8 class tile, from its fp32
//                    logits (first argmax of the softmax, as detect_convert writes it) or from the finished fp32 raster
//   raster_confmat   the same over the whole class band of a finished (2, H, W) fp32 raster
//   error_map        error_rate_patch (metrics.py:350-442): mismatch mask, two integer comb sums over the slice_pixels origins,
//                    / P, then scipy.ndimage.gaussian_filter (mode 'reflect') in fp64
// Every count is an integer: LDS-privatised u32 histograms flushed with integer atomics, so the matrices do not depend on the
// launch shape or the batch split.  No float atomics.
#include "logit_source.h"
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

constexpr int MAXC = 32;
constexpr int CHUNKS_PER_BLOCK = 2048;   // 4-pixel chunks of one window per block (8 per thread)

enum { SRC_PREDS = 0, SRC_LOGITS = 1, SRC_RASTER = 2, SRC_LOGITS_Q4 = 3 };

// numpy: uint8 raster - 1 wraps 0 -> 255; sklearn drops a pair whose truth or prediction lies outside range(C)
__device__ __forceinline__ unsigned truth_class(unsigned raw) { return (raw + 255u) & 0xffu; }

__device__ __forceinline__ unsigned float_class(float v) { return (v >= 0.f && v < 256.f) ? (unsigned)(int)v : 0xffu; }

// the class detect_convert_kernel writes for 'argmax': softmax in fp32, first index of the largest probability
template <class LSRC>
__device__ __forceinline__ unsigned logits_class(const LSRC& src, int C) {
  float x[MAXC];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) { x[c] = src(c); m = fmaxf(m, x[c]); }
  float ssum = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) { x[c] = expf(x[c] - m); ssum += x[c]; }
  int best = 0;
  float pbest = -1.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) {
      const float q = x[c] / ssum;
      if (q > pbest) { pbest = q; best = c; }
    }
  return (unsigned)best;
}

__device__ __forceinline__ void count(unsigned* hist, unsigned t, unsigned p, int C) {
  if (t < (unsigned)C && p < (unsigned)C) atomicAdd(&hist[t * C + p], 1u);
}

__device__ __forceinline__ void flush_hist(const unsigned* hist, int C, long long* __restrict__ out) {
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
    const unsigned v = hist[i];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(out + i), (unsigned long long)v);
  }
}

// grid (blocks per window, B); a block walks 4-pixel chunks (row i, columns 4q .. 4q+3) of window b's K x K core.
// A chunk reads its truth (and u8 / fp32 class) bytes with one vector load when the addresses allow it, else byte by byte.
// SRC_LOGITS_Q4: pred is the quarter-resolution (B, C, S/4, S/4) logits, interpolated per pixel (logit_source.h).
template <int SRC>
__global__ __launch_bounds__(256) void window_confmat_kernel(const void* __restrict__ pred, int C, int S, int margin,
                                                             const int* __restrict__ tiles, const unsigned char* __restrict__ truth,
                                                             int Hr, int Wr, long long* __restrict__ confmats) {
  __shared__ unsigned hist[MAXC * MAXC];
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  const int b = blockIdx.y, K = S - 2 * margin, QK = (K + 3) / 4;
  const long SS = (long)S * S, nchunk = (long)K * QK;
  const int cx = tiles[b * 6 + 0] + margin, cy = tiles[b * 6 + 1] + margin;   // the core's top-left raster pixel
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nchunk; t += (long)gridDim.x * blockDim.x) {
    const int i = (int)(t / QK), j = 4 * (int)(t - (long)i * QK);
    const int gy = cy + i, gx = cx + j;
    if ((unsigned)gy >= (unsigned)Hr) continue;
    const int n = min(min(4, K - j), Wr - gx);   // pixels of this chunk inside the core and the raster
    if (gx < 0 || n <= 0) {
      // a core reaching left of the raster (tiles not from tile_grid): count pixel by pixel
      for (int e = 0; e < min(4, K - j); ++e) {
        const int x = gx + e;
        if ((unsigned)x >= (unsigned)Wr) continue;
        const unsigned tc = truth_class(truth[(long)gy * Wr + x]);
        unsigned pc;
        if (SRC == SRC_PREDS) pc = reinterpret_cast<const unsigned char*>(pred)[b * SS + (long)(i + margin) * S + j + e + margin];
        else if (SRC == SRC_LOGITS) pc = logits_class(FullLogits(reinterpret_cast<const float*>(pred) + b * C * SS + (long)(i + margin) * S + j + e + margin, SS), C);
        else if (SRC == SRC_LOGITS_Q4) pc = logits_class(QuarterLogits(reinterpret_cast<const float*>(pred), b, C, S, SS, i + margin, j + e + margin), C);
        else pc = float_class(reinterpret_cast<const float*>(pred)[(long)gy * Wr + x]);
        count(hist, tc, pc, C);
      }
      continue;
    }
    const unsigned char* tp = truth + (long)gy * Wr + gx;
    unsigned tc[4], pc[4];
    if (n == 4 && !((uintptr_t)tp & 3)) {
      const unsigned w = *reinterpret_cast<const unsigned*>(tp);
#pragma unroll
      for (int e = 0; e < 4; ++e) tc[e] = truth_class((w >> (8 * e)) & 0xffu);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) tc[e] = e < n ? truth_class(tp[e]) : 0xffu;
    }
    if (SRC == SRC_PREDS) {
      const unsigned char* pp = reinterpret_cast<const unsigned char*>(pred) + b * SS + (long)(i + margin) * S + j + margin;
      if (n == 4 && !((uintptr_t)pp & 3)) {
        const unsigned w = *reinterpret_cast<const unsigned*>(pp);
#pragma unroll
        for (int e = 0; e < 4; ++e) pc[e] = (w >> (8 * e)) & 0xffu;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pc[e] = e < n ? pp[e] : 0xffu;
      }
    } else if (SRC == SRC_LOGITS) {
      const float* pp = reinterpret_cast<const float*>(pred) + b * C * SS + (long)(i + margin) * S + j + margin;
#pragma unroll
      for (int e = 0; e < 4; ++e) pc[e] = e < n ? logits_class(FullLogits(pp + e, SS), C) : 0xffu;
    } else if (SRC == SRC_LOGITS_Q4) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pc[e] = e < n ? logits_class(QuarterLogits(reinterpret_cast<const float*>(pred), b, C, S, SS, i + margin, j + e + margin), C) : 0xffu;
    } else {
      const float* pp = reinterpret_cast<const float*>(pred) + (long)gy * Wr + gx;   // band 0 of (2, H, W)
      if (n == 4 && !((uintptr_t)pp & 15)) {
        const float4 v = *reinterpret_cast<const float4*>(pp);
        pc[0] = float_class(v.x); pc[1] = float_class(v.y); pc[2] = float_class(v.z); pc[3] = float_class(v.w);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pc[e] = e < n ? float_class(pp[e]) : 0xffu;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) count(hist, tc[e], pc[e], C);
  }
  __syncthreads();
  flush_hist(hist, C, confmats + (long)b * C * C);
}

// the class band of a finished raster against the truth, 4 pixels per step (float4 + u32 loads: both arrays start aligned)
__global__ __launch_bounds__(256) void raster_confmat_kernel(const float* __restrict__ band, const unsigned char* __restrict__ truth,
                                                             long n, int C, long long* __restrict__ confmat) {
  __shared__ unsigned hist[MAXC * MAXC];
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(band)[i];
    const unsigned w = reinterpret_cast<const unsigned*>(truth)[i];
    count(hist, truth_class(w & 0xffu), float_class(v.x), C);
    count(hist, truth_class((w >> 8) & 0xffu), float_class(v.y), C);
    count(hist, truth_class((w >> 16) & 0xffu), float_class(v.z), C);
    count(hist, truth_class(w >> 24), float_class(v.w), C);
  }
  if (blockIdx.x == 0)
    for (long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) count(hist, truth_class(truth[i]), float_class(band[i]), C);
  __syncthreads();
  flush_hist(hist, C, confmat);
}

// error_rate_patch step 1: target != pred with the 255 of a no-data truth pixel counted as an error (metrics.py:410)
__global__ __launch_bounds__(256) void mismatch_kernel(const float* __restrict__ band, const unsigned char* __restrict__ truth, long n,
                                                       unsigned char* __restrict__ mask) {
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(band)[i];
    const unsigned w = reinterpret_cast<const unsigned*>(truth)[i];
    const unsigned r = (unsigned)((float)truth_class(w & 0xffu) != v.x) | ((unsigned)((float)truth_class((w >> 8) & 0xffu) != v.y) << 8) |
                       ((unsigned)((float)truth_class((w >> 16) & 0xffu) != v.z) << 16) |
                       ((unsigned)((float)truth_class(w >> 24) != v.w) << 24);
    reinterpret_cast<unsigned*>(mask)[i] = r;
  }
  if (blockIdx.x == 0)
    for (long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) mask[i] = (float)truth_class(truth[i]) != band[i];
}

// step 2a: colsum[r, j] = sum over column origins x of mask[r, x + j]   (H x K, one thread per entry, coalesced along j)
__global__ __launch_bounds__(256) void comb_cols_kernel(const unsigned char* __restrict__ mask, int Hr, int Wr, int K,
                                                        const int* __restrict__ xs, int nx, int* __restrict__ colsum) {
  const long total = (long)Hr * K;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int r = (int)(t / K), j = (int)(t - (long)r * K);
    const unsigned char* row = mask + (long)r * Wr + j;
    int s = 0;
    for (int k = 0; k < nx; ++k) {
      const int x = xs[k];
      if (x >= 0 && x + K <= Wr) s += row[x];
    }
    colsum[t] = s;
  }
}

// step 2b: counts[i, j] = sum over row origins y of colsum[y + i, j]   (K x K)
__global__ __launch_bounds__(256) void comb_rows_kernel(const int* __restrict__ colsum, int Hr, int K, const int* __restrict__ ys, int ny,
                                                        int* __restrict__ counts) {
  const long total = (long)K * K;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int i = (int)(t / K), j = (int)(t - (long)i * K);
    int s = 0;
    for (int k = 0; k < ny; ++k) {
      const int y = ys[k];
      if (y >= 0 && y + K <= Hr) s += colsum[(long)(y + i) * K + j];
    }
    counts[t] = s;
  }
}

// scipy.ndimage mode 'reflect' (d c b a | a b c d | d c b a), repeated for a line shorter than the filter
__device__ __forceinline__ int reflect(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

constexpr int MAXR = 32;

// step 3: one axis of gaussian_filter (correlate1d with the normalised exp(-x^2 / (2 sigma^2)), |x| <= radius) in fp64.
// axis 0 reads the integer counts and divides by P first (out_array / len(patches)); axis 1 reads the axis-0 result.
__global__ __launch_bounds__(256) void gauss_axis_kernel(const int* __restrict__ counts, const double* __restrict__ src, int K,
                                                         double n_patches, double sigma, int radius, int axis, double* __restrict__ dst) {
  __shared__ double w[2 * MAXR + 1];
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int k = -radius; k <= radius; ++k) { w[k + radius] = exp(-0.5 / (sigma * sigma) * (double)(k * k)); sum += w[k + radius]; }
    for (int k = 0; k <= 2 * radius; ++k) w[k] /= sum;
  }
  __syncthreads();
  const long total = (long)K * K;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int i = (int)(t / K), j = (int)(t - (long)i * K);
    double acc = 0.0;
    for (int k = -radius; k <= radius; ++k) {
      double v;
      if (axis == 0) v = (double)counts[(long)reflect(i + k, K) * K + j] / n_patches;
      else v = src[(long)i * K + reflect(j + k, K)];
      acc += w[k + radius] * v;
    }
    dst[t] = acc;
  }
}

inline int blocks_for(long items) {
  long b = (items + 255) / 256;
  if (b > 256 * 8) b = 256 * 8;
  return (int)(b < 1 ? 1 : b);
}

}  // namespace

int zone_window_confmat(int source, const void* pred, int B, int C, int S, int margin, const int* tiles, const unsigned char* truth,
                        int Hr, int Wr, long long* confmats, hipStream_t s) {
  if (source < SRC_PREDS || source > SRC_LOGITS_Q4 || C < 1 || C > MAXC || B < 0 || margin < 0 || S - 2 * margin < 1 || Hr < 1 || Wr < 1)
    return -2;
  if (source == SRC_LOGITS_Q4 && S % 4) return -2;
  if (B == 0) return 0;
  const long K = S - 2 * margin, nchunk = K * ((K + 3) / 4);
  const long nblk = (nchunk + CHUNKS_PER_BLOCK - 1) / CHUNKS_PER_BLOCK;
  const int per_window = (int)(nblk < 256 ? nblk : 256);
  const double bytes = (double)B * K * K * (1.0 + (source == SRC_PREDS ? 1.0 : source == SRC_LOGITS ? 4.0 * C : source == SRC_LOGITS_Q4 ? 0.25 * C : 4.0));
  ProfScope ps(source == SRC_LOGITS_Q4 ? "zone_window_confmat_q4" : "zone_window_confmat", 0.0, bytes, s);
  const dim3 grid(per_window, B);
  if (source == SRC_PREDS)
    hipLaunchKernelGGL(window_confmat_kernel<SRC_PREDS>, grid, dim3(256), 0, s, pred, C, S, margin, tiles, truth, Hr, Wr, confmats);
  else if (source == SRC_LOGITS)
    hipLaunchKernelGGL(window_confmat_kernel<SRC_LOGITS>, grid, dim3(256), 0, s, pred, C, S, margin, tiles, truth, Hr, Wr, confmats);
  else if (source == SRC_LOGITS_Q4)
    hipLaunchKernelGGL(window_confmat_kernel<SRC_LOGITS_Q4>, grid, dim3(256), 0, s, pred, C, S, margin, tiles, truth, Hr, Wr, confmats);
  else
    hipLaunchKernelGGL(window_confmat_kernel<SRC_RASTER>, grid, dim3(256), 0, s, pred, C, S, margin, tiles, truth, Hr, Wr, confmats);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int zone_raster_confmat(const float* band, const unsigned char* truth, int Hr, int Wr, int C, long long* confmat, hipStream_t s) {
  if (C < 1 || C > MAXC || Hr < 1 || Wr < 1) return -2;
  if (((uintptr_t)band & 15) || ((uintptr_t)truth & 3)) return -2;
  const long n = (long)Hr * Wr;
  ProfScope ps("zone_raster_confmat", 0.0, 5.0 * (double)n, s);
  hipLaunchKernelGGL(raster_confmat_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, s, band, truth, n, C, confmat);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int zone_error_map(const float* band, const unsigned char* truth, int Hr, int Wr, int K, const int* ys, int ny, const int* xs, int nx,
                   double sigma, int radius, unsigned char* mask, int* colsum, int* counts, double* tmp, double* out, hipStream_t s) {
  if (Hr < 1 || Wr < 1 || K < 1 || K > Hr || K > Wr || ny < 1 || nx < 1 || radius < 0 || radius > MAXR || !(sigma > 0.0)) return -2;
  if (((uintptr_t)band & 15) || ((uintptr_t)truth & 3) || ((uintptr_t)mask & 3)) return -2;
  const long n = (long)Hr * Wr, KK = (long)K * K;
  {
    ProfScope ps("zone_error_mask", 0.0, 6.0 * (double)n, s);
    hipLaunchKernelGGL(mismatch_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, s, band, truth, n, mask);
    FLAIR_CHECK_LAUNCH();
  }
  {
    ProfScope ps("zone_error_comb", (double)Hr * K * nx + (double)KK * ny, (double)Hr * K * (nx + 4.0) + (double)KK * 4.0 * (ny + 1), s);
    hipLaunchKernelGGL(comb_cols_kernel, dim3(blocks_for((long)Hr * K)), dim3(256), 0, s, mask, Hr, Wr, K, xs, nx, colsum);
    FLAIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(comb_rows_kernel, dim3(blocks_for(KK)), dim3(256), 0, s, colsum, Hr, K, ys, ny, counts);
    FLAIR_CHECK_LAUNCH();
  }
  ProfScope ps("zone_error_gauss", 4.0 * (2 * radius + 1) * (double)KK, 8.0 * (2 * radius + 2) * (double)KK, s);
  const double n_patches = (double)ny * (double)nx;
  hipLaunchKernelGGL(gauss_axis_kernel, dim3(blocks_for(KK)), dim3(256), 0, s, counts, nullptr, K, n_patches, sigma, radius, 0, tmp);
  FLAIR_CHECK_LAUNCH();
  hipLaunchKernelGGL(gauss_axis_kernel, dim3(blocks_for(KK)), dim3(256), 0, s, nullptr, tmp, K, n_patches, sigma, radius, 1, out);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
