// The per-pixel head of ce_head.hip with a configurable objective: label-smoothed or focal cross entropy and a soft multiclass
// Dice term, loss = ce * CE + dice * Dice (definitions: include/flair_hip.h, flair_amd/losses.py).  Same shape as
// ce_head(): ce_labels() -> lab8 and D, one pass over the logits that yields the CE contribution, the gradient, the argmax and the
// confusion matrix, a one-block fp64 sum.  Dice needs its per-class sums before any gradient can be written, so a spec with
// dice > 0 runs one more read of the logits first (seg_dice_sums_kernel + seg_dice_finalize_kernel); a spec without it does not.
// The softmax, the argmax and the histogram are ce_main_kernel's to the operation (e * (1 / sum e), strict >), so predictions and
// confusion matrix are bit-identical to flair_ce_head(_nhwc)'s.  No floating-point atomics: every sum has a fixed order.
#include <cmath>

#include "ops.h"
#include "prof.h"

namespace flair {
namespace {

constexpr int MAXC = 32;
enum { CE_NONE = 0, CE_PLAIN = 1, CE_SMOOTH = 2, CE_FOCAL = 3 };
enum { SRC_NCHW = 0, SRC_NHWC = 1 };
constexpr int DICE_OUT_FLOATS = 4 + 2 * MAXC;   // [0] the Dice value, [4 + 2c] dice * g_c for y != c, [4 + 2c + 1] for y == c

static inline int seg_blocks(long npix) {   // ce_blocks()
  long b = (npix + 255) / 256;
  if (b > CE_MAX_BLOCKS) b = CE_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

struct SegWorkspace { float* dice_out; float* dice_pf; int* dice_pt; };
static inline size_t seg_ce_floats(int B, int H, int W) { return (ce_workspace_floats(B, H, W) + 3) & ~(size_t)3; }
static SegWorkspace seg_workspace_layout(float* ws, int B, int H, int W) {
  SegWorkspace w;
  w.dice_out = ws + seg_ce_floats(B, H, W);
  w.dice_pf = w.dice_out + DICE_OUT_FLOATS;                       // [CE_MAX_BLOCKS][2 * MAXC]: I_c, then P_c
  w.dice_pt = reinterpret_cast<int*>(w.dice_pf + (size_t)CE_MAX_BLOCKS * 2 * MAXC);   // [CE_MAX_BLOCKS][MAXC]: T_c
  return w;
}

__device__ __forceinline__ float seg_block_sum(float v, float* sh) {   // the reduction tree of ce_head.hip's block_sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) {
    for (int w = 0; w < 4; ++w) r += sh[w];
  }
  __syncthreads();
  return r;  // valid in thread 0
}

template <typename TO>
__device__ __forceinline__ void seg_store_row(TO* dst, const float* g, int C, int ld) {
  constexpr int CH = Elem<TO>::CH;
#pragma unroll
  for (int c0 = 0; c0 < MAXC; c0 += CH)
    if (c0 < ld) {
      float f[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) f[e] = (c0 + e) < C ? g[c0 + e] : 0.f;
      *reinterpret_cast<uint4*>(dst + c0) = f_to_chunk<TO>(f);
    }
}

// one pixel's C logits -> x[0 .. C)
template <int SRC, typename T, int LD>
__device__ __forceinline__ void seg_load_row(const void* logits, long i, long HW, int C, float* x) {
  if constexpr (SRC == SRC_NCHW) {
    const long n = i / HW, pix = i - n * HW;
    const float* p = (const float*)logits + n * C * HW + pix;
#pragma unroll
    for (int c = 0; c < LD; ++c)
      if (c < C) x[c] = p[(long)c * HW];
  } else {
    constexpr int CH = Elem<T>::CH;
#pragma unroll
    for (int c0 = 0; c0 < LD; c0 += CH) chunk_to_f<T>(*reinterpret_cast<const uint4*>((const T*)logits + i * LD + c0), x + c0);
  }
}

// x -> softmax(x) in place, by ce_main_kernel's operations; returns the argmax (first index among equals)
template <int LD>
__device__ __forceinline__ int seg_softmax(float* x, int C, int y, float& m, float& xy, float& ssum) {
  m = -INFINITY;
#pragma unroll
  for (int c = 0; c < LD; ++c)
    if (c < C) m = fmaxf(m, x[c]);
  xy = 0.f;
  ssum = 0.f;
#pragma unroll
  for (int c = 0; c < LD; ++c)
    if (c < C) {
      if (c == y) xy = x[c];
      x[c] = __expf(x[c] - m);
      ssum += x[c];
    }
  const float rs = 1.f / ssum;
  int pred = 0;
  float pbest = -1.f;
#pragma unroll
  for (int c = 0; c < LD; ++c)
    if (c < C) {
      x[c] = x[c] * rs;
      if (x[c] > pbest) { pbest = x[c]; pred = c; }
    }
  return pred;
}

// ---- Dice sums: I_c = sum k p_c [y = c], P_c = sum k p_c, T_c = sum k [y = c] over the counted pixels, per block
template <int SRC, typename T, int LD>
__global__ __launch_bounds__(256) void seg_dice_sums_kernel(const void* __restrict__ logits, const unsigned char* __restrict__ lab8,
                                                            const float* __restrict__ weight, int C, long HW, long npix,
                                                            float* __restrict__ pf, int* __restrict__ pt) {
  __shared__ float shr[4][2 * MAXC];
  __shared__ unsigned int tcount[MAXC];
  if (threadIdx.x < MAXC) tcount[threadIdx.x] = 0;
  __syncthreads();
  float I[LD], P[LD];
#pragma unroll
  for (int c = 0; c < LD; ++c) { I[c] = 0.f; P[c] = 0.f; }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
    const int y = lab8[i];
    if (!(y < C && (!weight || weight[y] > 0.f))) continue;   // not counted: its logits are not read
    float x[LD];
    seg_load_row<SRC, T, LD>(logits, i, HW, C, x);
    float m, xy, ssum;
    seg_softmax<LD>(x, C, y, m, xy, ssum);
#pragma unroll
    for (int c = 0; c < LD; ++c)
      if (c < C) {
        P[c] += x[c];
        I[c] += c == y ? x[c] : 0.f;
      }
    atomicAdd(&tcount[y], 1u);   // (integer, LDS)
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < LD; ++c) {
    float a = I[c], b = P[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if (lane == 0) { shr[wave][c] = a; shr[wave][MAXC + c] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * MAXC) {
    const int c = threadIdx.x & (MAXC - 1);
    float r = 0.f;
    if (c < LD) r = ((shr[0][threadIdx.x] + shr[1][threadIdx.x]) + shr[2][threadIdx.x]) + shr[3][threadIdx.x];
    pf[(long)blockIdx.x * 2 * MAXC + threadIdx.x] = r;
  }
  if (threadIdx.x < MAXC) pt[(long)blockIdx.x * MAXC + threadIdx.x] = (int)tcount[threadIdx.x];
}

// one block: the partial rows in fp64, eight interleaved runs per class and then those eight in order; the Dice value and the
// per-class gradient pair, scaled by the term's coefficient, for the main pass
__global__ __launch_bounds__(256) void seg_dice_finalize_kernel(const float* __restrict__ pf, const int* __restrict__ pt, int nb, int C,
                                                                float dice_w, float smooth, float eps, float* __restrict__ out) {
  __shared__ double sI[8][MAXC], sP[8][MAXC], sD[MAXC];
  __shared__ long long sT[8][MAXC];
  const int g = threadIdx.x >> 5, c = threadIdx.x & (MAXC - 1);
  double aI = 0.0, aP = 0.0;
  long long aT = 0;
  for (int b = g; b < nb; b += 8) {
    aI += (double)pf[(long)b * 2 * MAXC + c];
    aP += (double)pf[(long)b * 2 * MAXC + MAXC + c];
    aT += pt[(long)b * MAXC + c];
  }
  sI[g][c] = aI; sP[g][c] = aP; sT[g][c] = aT;
  __syncthreads();
  if (threadIdx.x < MAXC) {
    double I = 0.0, P = 0.0;
    long long T = 0;
    for (int k = 0; k < 8; ++k) { I += sI[k][c]; P += sP[k][c]; T += sT[k][c]; }
    double d = 0.0, gno = 0.0, gyes = 0.0;
    if (c < C && T > 0) {
      const double u = 2.0 * I + (double)smooth, den = P + (double)T + (double)smooth;
      if (den >= (double)eps) {
        d = 1.0 - u / den;
        gno = u / (den * den) / C;
        gyes = gno - 2.0 / (den * C);
      } else {   // the clamp holds the denominator: only the intersection moves the term
        d = 1.0 - u / (double)eps;
        gyes = -2.0 / ((double)eps * C);
      }
    }
    sD[c] = d;
    out[4 + 2 * c] = (float)((double)dice_w * gno);
    out[4 + 2 * c + 1] = (float)((double)dice_w * gyes);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < C; ++k) s += sD[k];
    out[0] = (float)(s / C);
  }
}

// ---- main pass
struct SegMainArgs {
  const void* logits;
  const unsigned char* lab8;
  const float* weight;
  const float* den;
  const float* dice_g;      // dice_out + 4
  int C;
  long HW, npix;
  float ce, ls, gamma;
  float* loss_partial;
  void* dl;
  unsigned char* preds_u8;
  long long* preds_i64;
  long long* confmat;
};

template <int SRC, typename T, int LD, int CEK, bool DICE>
__global__ __launch_bounds__(256) void seg_main_kernel(const SegMainArgs a) {
  __shared__ float sh[4];
  __shared__ unsigned int hist[MAXC * MAXC];
  __shared__ float shw[MAXC];
  __shared__ float shg[2 * MAXC];
  const int C = a.C;
  if (a.confmat)
    for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0;
  if (threadIdx.x < MAXC) shw[threadIdx.x] = (int)threadIdx.x < C ? (a.weight ? a.weight[threadIdx.x] : 1.f) : 0.f;
  if (DICE && threadIdx.x < 2 * MAXC) shg[threadIdx.x] = a.dice_g[threadIdx.x];
  __syncthreads();
  float wsum = 0.f;   // sum of the class weights, in class order
  if (CEK == CE_SMOOTH)
    for (int c = 0; c < C; ++c) wsum += shw[c];
  const float cscale = CEK != CE_NONE ? a.ce * (1.f / a.den[0]) : 0.f;   // the coefficient and the mean reduction
  const float keep = 1.f - a.ls, lsc = a.ls / (float)C;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.npix; i += (long)gridDim.x * blockDim.x) {
    float x[LD];
    seg_load_row<SRC, T, LD>(a.logits, i, a.HW, C, x);
    const int y = a.lab8[i];
    const bool ok = y < C;
    float swz = 0.f;   // sum_c w[c] (z_c - m): with log(sum e) all the smoothing term needs, no logarithm per class
    if (CEK == CE_SMOOTH) {
      float m0 = -INFINITY;
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < C) m0 = fmaxf(m0, x[c]);
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < C) swz += shw[c] * (x[c] - m0);
    }
    float m, xy, ssum;
    const int pred = seg_softmax<LD>(x, C, y, m, xy, ssum);
    const float w = ok ? shw[y < MAXC ? y : 0] : 0.f;
    if (a.preds_u8) a.preds_u8[i] = (unsigned char)pred;
    if (SRC == SRC_NCHW && a.preds_i64) a.preds_i64[i] = pred;
    if (a.confmat && ok) atomicAdd(&hist[y * C + pred], 1u);
    // the CE term's contribution and its gradient: g[c] = (p_c or its focal stand-in) * ga - [c == y] * gy - w[c] * gs
    float g[LD];
    if (CEK == CE_NONE) {
#pragma unroll
      for (int c = 0; c < LD; ++c) g[c] = 0.f;
    } else if (CEK == CE_PLAIN) {
      if (ok) acc += w * (logf(ssum) - (xy - m));
      const float sc = w * cscale;
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < C) g[c] = (x[c] - ((ok && c == y) ? 1.f : 0.f)) * sc;
    } else if (CEK == CE_SMOOTH) {
      const float lse = logf(ssum);
      if (ok) acc += keep * w * (lse - (xy - m)) + lsc * (wsum * lse - swz);
      const float ga = ok ? (keep * w + lsc * wsum) * cscale : 0.f, gy = keep * w * cscale, gs = ok ? lsc * cscale : 0.f;
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < C) g[c] = x[c] * ga - ((ok && c == y) ? gy : 0.f) - shw[c] * gs;
    } else {
      // focal: q is summed from the other classes (never 1 - p_y), and the label's own column is -q, not p_y - 1
      float q = 0.f, py = 0.f;
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < C) {
          if (c == y) py = x[c];
          else q += x[c];
        }
      const float nll = logf(ssum) - (xy - m);
      const float qg1 = powf(q, a.gamma - 1.f);
      if (ok) acc += w * (qg1 * q) * nll;
      const float sc = ok ? w * (qg1 * (a.gamma * nll * py + q)) * cscale : 0.f;
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < C) g[c] = ((ok && c == y) ? -q : x[c]) * sc;
    }
    if (DICE) {
      // d Dice / d z_k = k p_k (g_k - sum_c g_c p_c), g_c picked by [y = c] from the finalize's pairs (already times the coefficient)
      if (ok && w > 0.f) {
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < LD; ++c)
          if (c < C) dot += x[c] * (c == y ? shg[2 * c + 1] : shg[2 * c]);
#pragma unroll
        for (int c = 0; c < LD; ++c)
          if (c < C) g[c] = g[c] + x[c] * ((c == y ? shg[2 * c + 1] : shg[2 * c]) - dot);
      }
    }
    if (a.dl) {
      if constexpr (SRC == SRC_NCHW) {
        const long n = i / a.HW, pix = i - n * a.HW;
        float* d = (float*)a.dl + n * C * a.HW + pix;
#pragma unroll
        for (int c = 0; c < LD; ++c)
          if (c < C) d[(long)c * a.HW] = g[c];
      } else {
        float gq[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) gq[c] = (c < LD && c < C) ? g[c < LD ? c : 0] : 0.f;
        seg_store_row<T>((T*)a.dl + i * LD, gq, C, LD);
      }
    }
  }
  const float r = seg_block_sum(acc, sh);
  if (threadIdx.x == 0) a.loss_partial[blockIdx.x] = r;
  if (a.confmat) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) {
      const unsigned int v = hist[i];
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.confmat + i), (unsigned long long)v);
    }
  }
}

// [loss, CE, Dice]: the CE partials in fp64 over D (ce_sum_kernel), the Dice value as the finalize left it
__global__ __launch_bounds__(256) void seg_finish_kernel(const float* __restrict__ partial, int n, const float* __restrict__ den,
                                                         const float* __restrict__ dice_out, float ce_w, float dice_w, int have_ce,
                                                         int have_dice, float* __restrict__ out) {
  __shared__ double sh[256];
  double a = 0.0;
  if (have_ce)
    for (int i = threadIdx.x; i < n; i += 256) a += (double)partial[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double ce = have_ce ? sh[0] / (double)den[0] : 0.0;
    const double dice = have_dice ? (double)dice_out[0] : 0.0;
    double loss = 0.0;
    if (have_ce) loss += (double)ce_w * ce;
    if (have_dice) loss += (double)dice_w * dice;
    out[0] = (float)loss;
    out[1] = (float)ce;
    out[2] = (float)dice;
  }
}

using seg_main_fn = void (*)(const SegMainArgs);
template <int SRC, typename T, int LD>
seg_main_fn seg_main_for(int cek, bool dice) {
  switch (cek * 2 + (dice ? 1 : 0)) {
    case CE_NONE * 2 + 1: return seg_main_kernel<SRC, T, LD, CE_NONE, true>;
    case CE_PLAIN * 2: return seg_main_kernel<SRC, T, LD, CE_PLAIN, false>;
    case CE_PLAIN * 2 + 1: return seg_main_kernel<SRC, T, LD, CE_PLAIN, true>;
    case CE_SMOOTH * 2: return seg_main_kernel<SRC, T, LD, CE_SMOOTH, false>;
    case CE_SMOOTH * 2 + 1: return seg_main_kernel<SRC, T, LD, CE_SMOOTH, true>;
    case CE_FOCAL * 2: return seg_main_kernel<SRC, T, LD, CE_FOCAL, false>;
    case CE_FOCAL * 2 + 1: return seg_main_kernel<SRC, T, LD, CE_FOCAL, true>;
  }
  return nullptr;
}

using seg_sums_fn = void (*)(const void*, const unsigned char*, const float*, int, long, long, float*, int*);

bool spec_ok(const SegLossSpec& s) {
  const float v[6] = {s.ce, s.label_smoothing, s.focal_gamma, s.dice, s.dice_smooth, s.dice_eps};
  for (float f : v)
    if (!std::isfinite(f)) return false;
  if (s.ce < 0.f || s.dice < 0.f || (s.ce == 0.f && s.dice == 0.f)) return false;
  if (s.label_smoothing < 0.f || s.label_smoothing >= 1.f) return false;
  if (s.focal_gamma != 0.f && s.focal_gamma < 1.f) return false;
  if (s.label_smoothing > 0.f && s.focal_gamma > 0.f) return false;
  if (s.ce == 0.f && (s.label_smoothing > 0.f || s.focal_gamma > 0.f)) return false;
  if (s.dice_smooth < 0.f || s.dice_eps <= 0.f) return false;
  return true;
}

}  // namespace

size_t seg_loss_workspace_bytes(int B, int C, int H, int W) {
  (void)C;   // the partial rows are MAXC wide whatever C
  return (seg_ce_floats(B, H, W) + DICE_OUT_FLOATS + (size_t)CE_MAX_BLOCKS * 3 * MAXC) * sizeof(float);
}

int seg_loss(const SegLossArgs& a, hipStream_t s) {
  // every refusal comes before the first launch
  if (!spec_ok(a.spec)) return -20;
  if (a.C > MAXC || a.C < 1) return -2;
  const bool nhwc = a.logits_nhwc != nullptr;
  if (nhwc) {
    if ((a.ld != 16 && a.ld != 32) || a.ld < a.C || a.preds_i64) return -3;
    if (((uintptr_t)a.logits_nhwc | (uintptr_t)a.dl) & 15) return -3;
  } else if ((uintptr_t)a.dl & 3) {
    return -3;
  }
  if ((uintptr_t)a.workspace & 3) return -3;
  const long HW = (long)a.H * a.W, npix = HW * a.B;
  const int nb = seg_blocks(npix);
  const CeWorkspace cw = ce_workspace_layout(a.workspace, npix);
  const SegWorkspace sw = seg_workspace_layout(a.workspace, a.B, a.H, a.W);
  const bool dice = a.spec.dice > 0.f;
  const int cek = a.spec.ce == 0.f ? CE_NONE : a.spec.focal_gamma > 0.f ? CE_FOCAL : a.spec.label_smoothing > 0.f ? CE_SMOOTH : CE_PLAIN;
  const double row_bytes = nhwc ? (double)a.ld * dtype_size(a.dtype) : 4.0 * a.C;
  const void* src = nhwc ? a.logits_nhwc : (const void*)a.logits;

  if (int rc = ce_labels(a.labels, a.label_kind, a.weight, a.B, a.C, a.H, a.W, a.targets_i32, a.workspace, s)) return rc;
  if (dice) {
    seg_sums_fn kern;
    if (!nhwc) kern = seg_dice_sums_kernel<SRC_NCHW, float, MAXC>;
    else if (a.dtype == DT_F32) kern = a.ld == 16 ? seg_dice_sums_kernel<SRC_NHWC, float, 16> : seg_dice_sums_kernel<SRC_NHWC, float, 32>;
    else kern = a.ld == 16 ? seg_dice_sums_kernel<SRC_NHWC, bf16_t, 16> : seg_dice_sums_kernel<SRC_NHWC, bf16_t, 32>;
    {
      ProfScope ps("seg_dice_sums", 0.0, (double)npix * (row_bytes + 1), s);
      hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, src, cw.lab8, a.weight, a.C, HW, npix, sw.dice_pf, sw.dice_pt);
      FLAIR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(seg_dice_finalize_kernel, dim3(1), dim3(256), 0, s, sw.dice_pf, sw.dice_pt, nb, a.C, a.spec.dice, a.spec.dice_smooth,
                       a.spec.dice_eps, sw.dice_out);
    FLAIR_CHECK_LAUNCH();
  }
  seg_main_fn kern;
  if (!nhwc) kern = seg_main_for<SRC_NCHW, float, MAXC>(cek, dice);
  else if (a.dtype == DT_F32) kern = a.ld == 16 ? seg_main_for<SRC_NHWC, float, 16>(cek, dice) : seg_main_for<SRC_NHWC, float, 32>(cek, dice);
  else kern = a.ld == 16 ? seg_main_for<SRC_NHWC, bf16_t, 16>(cek, dice) : seg_main_for<SRC_NHWC, bf16_t, 32>(cek, dice);
  if (!kern) return -20;
  SegMainArgs m;
  m.logits = src; m.lab8 = cw.lab8; m.weight = a.weight; m.den = cw.den; m.dice_g = sw.dice_out + 4; m.C = a.C; m.HW = HW; m.npix = npix;
  m.ce = a.spec.ce; m.ls = a.spec.label_smoothing; m.gamma = a.spec.focal_gamma; m.loss_partial = cw.loss_partial; m.dl = a.dl;
  m.preds_u8 = a.preds_u8; m.preds_i64 = a.preds_i64; m.confmat = a.confmat;
  {
    ProfScope ps("seg_loss_main", 0.0, (double)npix * (row_bytes * (a.dl ? 2 : 1) + 1 + (a.preds_u8 ? 1 : 0) + (a.preds_i64 ? 8 : 0)), s);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, m);
    FLAIR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(256), 0, s, cw.loss_partial, nb, cw.den, sw.dice_out, a.spec.ce, a.spec.dice,
                     cek != CE_NONE ? 1 : 0, dice ? 1 : 0, a.loss3);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
