// Update rules of the fused trainer over one flat fp32 buffer (DESIGN §10 "Optimizers"): torch.optim.SGD's and torch.optim.AdamW's
// single-tensor rules, the squared gradient norm and clip_grad_norm_'s coefficient.  One bandwidth-bound pass each: float4 per lane,
// 256-thread blocks, a grid-stride loop capped like misc.hip's elementwise launches, the n % 4 tail by the first lanes of block 0.
// Plain C++ with vector loads and stores, no atomics; nothing here waits for the host -- the clip coefficient travels in memory.
//   g' = g * grad_scale * coef        (coef read from a device float when given, else 1; both left out of the plain instances)
//   optim_sgd     g' += wd p;  buf = first ? g' : mu buf + (1 - damp) g';  g' = nesterov ? g' + mu buf : buf;  p -= lr g'
//   optim_adamw   m += (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2;  p = p (1 - lr wd) - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
//   grad_sqnorm   sum g^2 in fp64: a grid that depends on n alone writes one partial per block, one block adds them in a fixed order
//   clip_coef     norm = sqrt(sum) * grad_scale;  coef = min(1, max_norm / (norm + 1e-6))
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  if (b > 256 * 16) b = 256 * 16;
  if (b < 1) b = 1;
  return (int)b;
}

// momentum buffer: none, written from g' (first step: its content is not read), or updated
enum { MOM_NONE = 0, MOM_FIRST = 1, MOM_NEXT = 2 };

struct SgdArgs {
  float lr, momentum, one_minus_damp, weight_decay, grad_scale;
  const float* coef;
};

template <bool SCALE, bool WD, int MOM, bool NEST>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, const SgdArgs& a, float coef) {
  if (SCALE) g = g * a.grad_scale * coef;
  if (WD) g += a.weight_decay * p;
  if (MOM == MOM_FIRST) b = g;
  if (MOM == MOM_NEXT) b = a.momentum * b + a.one_minus_damp * g;
  if (MOM != MOM_NONE) g = NEST ? g + a.momentum * b : b;
  p -= a.lr * g;   // <false, false, MOM_NONE, false>: misc.hip's sgd_kernel, to the bit
}

template <bool SCALE, bool WD, int MOM, bool NEST>
__global__ __launch_bounds__(256) void optim_sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                        SgdArgs a) {
  const float coef = SCALE && a.coef ? *a.coef : 1.f;
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 x = reinterpret_cast<float4*>(p)[i];
    const float4 y = reinterpret_cast<const float4*>(g)[i];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MOM == MOM_NEXT) b = reinterpret_cast<float4*>(buf)[i];
    sgd_elem<SCALE, WD, MOM, NEST>(x.x, y.x, b.x, a, coef);
    sgd_elem<SCALE, WD, MOM, NEST>(x.y, y.y, b.y, a, coef);
    sgd_elem<SCALE, WD, MOM, NEST>(x.z, y.z, b.z, a, coef);
    sgd_elem<SCALE, WD, MOM, NEST>(x.w, y.w, b.w, a, coef);
    reinterpret_cast<float4*>(p)[i] = x;
    if (MOM != MOM_NONE) reinterpret_cast<float4*>(buf)[i] = b;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = n4 * 4 + threadIdx.x;
    float x = p[i], b = 0.f;
    if (MOM == MOM_NEXT) b = buf[i];
    sgd_elem<SCALE, WD, MOM, NEST>(x, g[i], b, a, coef);
    p[i] = x;
    if (MOM != MOM_NONE) buf[i] = b;
  }
}

struct AdamArgs {
  float decay /* 1 - lr wd */, step_size /* lr / bc1 */, one_minus_b1, beta2, one_minus_b2, sqrt_bc2, eps, grad_scale;
  const float* coef;
};

template <bool SCALE>
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamArgs& a, float coef) {
  if (SCALE) g = g * a.grad_scale * coef;
  m = m + (g - m) * a.one_minus_b1;
  v = a.beta2 * v + a.one_minus_b2 * (g * g);
  const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
  p = fmaf(p, a.decay, -(a.step_size * (m / denom)));   // decay and step in one rounding
}

template <bool SCALE, bool FIRST>
__global__ __launch_bounds__(256) void optim_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long n, AdamArgs a) {
  const float coef = SCALE && a.coef ? *a.coef : 1.f;
  const long n4 = n / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 x = reinterpret_cast<float4*>(p)[i];
    const float4 y = reinterpret_cast<const float4*>(g)[i];
    float4 mm = make_float4(0.f, 0.f, 0.f, 0.f), vv = mm;   // a first step reads neither state buffer
    if (!FIRST) {
      mm = reinterpret_cast<float4*>(m)[i];
      vv = reinterpret_cast<float4*>(v)[i];
    }
    adamw_elem<SCALE>(x.x, y.x, mm.x, vv.x, a, coef);
    adamw_elem<SCALE>(x.y, y.y, mm.y, vv.y, a, coef);
    adamw_elem<SCALE>(x.z, y.z, mm.z, vv.z, a, coef);
    adamw_elem<SCALE>(x.w, y.w, mm.w, vv.w, a, coef);
    reinterpret_cast<float4*>(p)[i] = x;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = n4 * 4 + threadIdx.x;
    float x = p[i], mm = 0.f, vv = 0.f;
    if (!FIRST) {
      mm = m[i];
      vv = v[i];
    }
    adamw_elem<SCALE>(x, g[i], mm, vv, a, coef);
    p[i] = x;
    m[i] = mm;
    v[i] = vv;
  }
}

// ---------------------------------------------------------------- squared norm
constexpr int SQN_MAX_BLOCKS = 1024;

inline int sqnorm_blocks(long n) {
  long b = (n / 4 + 255) / 256;
  if (b > SQN_MAX_BLOCKS) b = SQN_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

// sum over the block's 256 lanes in a fixed order (lane tree inside each wave, then the four waves in index order); valid in thread 0
__device__ __forceinline__ double block_sum_256(double acc, double* wave_sums) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partials) {
  __shared__ double wave_sums[4];
  const long n4 = n / 4;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 y = reinterpret_cast<const float4*>(g)[i];
    acc += (double)y.x * y.x;
    acc += (double)y.y * y.y;
    acc += (double)y.z * y.z;
    acc += (double)y.w * y.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float y = g[n4 * 4 + threadIdx.x];
    acc += (double)y * y;
  }
  const double total = block_sum_256(acc, wave_sums);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void sqnorm_final_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ sum,
                                                           int accumulate) {
  __shared__ double wave_sums[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) acc += partials[i];
  const double total = block_sum_256(acc, wave_sums);
  if (threadIdx.x == 0) *sum = accumulate ? *sum + total : total;
}

__global__ void clip_coef_kernel(const double* __restrict__ sum, float grad_scale, float max_norm, float* __restrict__ norm,
                                 float* __restrict__ coef) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float nrm = (float)(sqrt(*sum) * (double)grad_scale);
    const float c = max_norm / (nrm + 1e-6f);
    *norm = nrm;
    *coef = c > 1.f ? 1.f : c;   // a NaN norm stays visible in coef, as torch.clamp keeps it
  }
}

template <bool SCALE, bool WD>
void launch_sgd(float* p, const float* g, float* buf, long n, const SgdArgs& a, int mom, bool nest, hipStream_t s) {
  const dim3 grid(ew_blocks(n / 4 + 1)), block(256);
  if (mom == MOM_NONE) hipLaunchKernelGGL((optim_sgd_kernel<SCALE, WD, MOM_NONE, false>), grid, block, 0, s, p, g, buf, n, a);
  else if (mom == MOM_FIRST && !nest) hipLaunchKernelGGL((optim_sgd_kernel<SCALE, WD, MOM_FIRST, false>), grid, block, 0, s, p, g, buf, n, a);
  else if (mom == MOM_FIRST) hipLaunchKernelGGL((optim_sgd_kernel<SCALE, WD, MOM_FIRST, true>), grid, block, 0, s, p, g, buf, n, a);
  else if (!nest) hipLaunchKernelGGL((optim_sgd_kernel<SCALE, WD, MOM_NEXT, false>), grid, block, 0, s, p, g, buf, n, a);
  else hipLaunchKernelGGL((optim_sgd_kernel<SCALE, WD, MOM_NEXT, true>), grid, block, 0, s, p, g, buf, n, a);
}

inline bool misaligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) != 0;
}

}  // namespace

int optim_sgd(float* params, const float* grads, float* buf, long n, float lr, float momentum, float dampening, float weight_decay,
              int nesterov, int first, float grad_scale, const float* coef, hipStream_t s) {
  if (!params || !grads || n < 0 || (momentum != 0.f && !buf)) return -1;
  if (!(momentum >= 0.f) || !(weight_decay >= 0.f) || !(lr >= 0.f)) return -2;
  if (nesterov && (momentum == 0.f || dampening != 0.f)) return -2;
  if (misaligned16(params, grads, momentum != 0.f ? buf : nullptr) || ((uintptr_t)coef & 3)) return -2;
  const int mom = momentum == 0.f ? MOM_NONE : (first ? MOM_FIRST : MOM_NEXT);
  const bool scale = grad_scale != 1.f || coef, wd = weight_decay != 0.f;
  const SgdArgs a = {lr, momentum, 1.f - dampening, weight_decay, grad_scale, coef};
  ProfScope ps(mom == MOM_NONE ? "optim_sgd" : "optim_sgd_momentum", 0.0, (double)n * (mom == MOM_NONE ? 12.0 : mom == MOM_FIRST ? 16.0 : 20.0), s);
  if (scale && wd) launch_sgd<true, true>(params, grads, buf, n, a, mom, nesterov != 0, s);
  else if (scale) launch_sgd<true, false>(params, grads, buf, n, a, mom, nesterov != 0, s);
  else if (wd) launch_sgd<false, true>(params, grads, buf, n, a, mom, nesterov != 0, s);
  else launch_sgd<false, false>(params, grads, buf, n, a, mom, nesterov != 0, s);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int optim_adamw(float* params, const float* grads, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                float weight_decay, float bc1, float bc2, int first, float grad_scale, const float* coef, hipStream_t s) {
  if (!params || !grads || !m || !v || n < 0) return -1;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return -2;
  if (!(lr >= 0.f) || !(eps >= 0.f) || !(weight_decay >= 0.f) || !(bc1 > 0.f) || !(bc2 > 0.f)) return -2;
  if (misaligned16(params, grads, m, v) || ((uintptr_t)coef & 3)) return -2;
  const bool scale = grad_scale != 1.f || coef;
  const AdamArgs a = {1.f - lr * weight_decay, lr / bc1, 1.f - beta1, beta2, 1.f - beta2, sqrtf(bc2), eps, grad_scale, coef};
  ProfScope ps("optim_adamw", 0.0, (double)n * (first ? 20.0 : 28.0), s);
  const dim3 grid(ew_blocks(n / 4 + 1)), block(256);
  if (scale && first) hipLaunchKernelGGL((optim_adamw_kernel<true, true>), grid, block, 0, s, params, grads, m, v, n, a);
  else if (scale) hipLaunchKernelGGL((optim_adamw_kernel<true, false>), grid, block, 0, s, params, grads, m, v, n, a);
  else if (first) hipLaunchKernelGGL((optim_adamw_kernel<false, true>), grid, block, 0, s, params, grads, m, v, n, a);
  else hipLaunchKernelGGL((optim_adamw_kernel<false, false>), grid, block, 0, s, params, grads, m, v, n, a);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int grad_sqnorm_partials() { return SQN_MAX_BLOCKS; }

int grad_sqnorm(const float* grads, long n, double* partials, double* sum, int accumulate, hipStream_t s) {
  if (!grads || !partials || !sum || n < 0) return -1;
  if (((uintptr_t)grads & 15) || (((uintptr_t)partials | (uintptr_t)sum) & 7)) return -2;
  const int nblk = sqnorm_blocks(n);
  ProfScope ps("grad_sqnorm", 0.0, (double)n * 4.0, s);
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nblk), dim3(256), 0, s, grads, n, partials);
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, nblk, sum, accumulate);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int clip_coef(const double* sum, float grad_scale, float max_norm, float* norm, float* coef, hipStream_t s) {
  if (!sum || !norm || !coef) return -1;
  if (!(max_norm > 0.f) || !(grad_scale > 0.f)) return -2;
  if (((uintptr_t)sum & 7) || (((uintptr_t)norm | (uintptr_t)coef) & 3)) return -2;
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, s, sum, grad_scale, max_norm, norm, coef);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
