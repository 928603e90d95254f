// Kernels of the UperNet-Swin inference path (transformers' UperNetForSemanticSegmentation with a SwinBackbone) that the
// SegFormer path does not have: shifted-window attention, LayerNorm over wide rows (with the patch-merging gather), adaptive
// average pooling of the pyramid-pooling module and the FPN's upsample-add.  The matrix products run on conv_igemm.hip /
// conv_hg.hip.  Activations are token-major [B * H * W][C] = NHWC, T = float (parity mode, exact-fp32 MFMA) or bf16.
#include "swin_ops.h"

#include "bilinear_src.h"
#include "prof.h"

namespace flair {
namespace {

// ------------------------------------------------------------------------------------------------ shifted-window attention
// One wave per (window, head, image).  A window is 49 tokens, padded to 64 slots (four 16-row tiles); slots 49 .. 63 only fill
// the tiles: as keys they get -inf, as queries they are never stored.  Slot j < 49 is position (j / 7, j % 7) of the window on
// the shifted, padded grid; torch.roll(x, -shift) puts padded-grid position ((sy + shift) % Hp, (sx + shift) % Wp) there, and a
// position past the real grid is a pad token (zeros after the LayerNorm: q, k, v = the projection biases).  The merge back
// and the reverse roll send the output of slot j to that same position; pad positions are cropped (not stored).
// K rows and V^T go to LDS; the scores are computed TRANSPOSED, S^T = K Q^T (as in segformer_ops.hip's attention), so that a
// lane holds one query's scores for 4 keys per 16-key tile: bias, mask and softmax are applied in registers and the
// exponentiated scores are the B operand of O^T = V^T P^T.
template <typename T> struct SwAtt;
template <> struct SwAtt<bf16_t> {
  static constexpr int KROW = 64 + 16;    // bytes per key row of K (32 bf16 + pad)
  static constexpr int VROW = 128 + 16;   // bytes per channel row of V^T (64 slots + pad)
};
template <> struct SwAtt<float> {
  static constexpr int KROW = 128 + 16;
  static constexpr int VROW = 256 + 16;
};

template <typename T>
__global__ __launch_bounds__(64) void swin_attention_kernel(const T* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                            const float* __restrict__ table, T* __restrict__ out, int H, int W, int C,
                                                            int heads, int shift, int Hp, int Wp, int nwx) {
  constexpr int CH = Elem<T>::CH;
  constexpr int KROW = SwAtt<T>::KROW, VROW = SwAtt<T>::VROW;
  __shared__ __attribute__((aligned(16))) unsigned char ks[64 * KROW];
  __shared__ __attribute__((aligned(16))) unsigned char vt[32 * VROW];
  __shared__ float rb[169];
  __shared__ int tok[64];   // token (y * W + x) of slot j, -1: pad token or filler
  __shared__ int lab[64];   // region label of slot j on the padded grid (shifted blocks)
  const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
  const int win = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int wy = win / nwx, wx = win - wy * nwx;
  const long C3 = 3L * C;
  const T* __restrict__ base = qkv + (long)b * H * W * C3;
  int tk = -1, lb = 0;
  if (lane < 49) {
    const int py = lane / 7, px = lane - py * 7;
    const int sy = wy * 7 + py, sx = wx * 7 + px;
    int oy = sy + shift, ox = sx + shift;
    if (oy >= Hp) oy -= Hp;
    if (ox >= Wp) ox -= Wp;
    tk = (oy < H && ox < W) ? oy * W + ox : -1;
    // SwinLayer.get_attn_mask: regions [0, Hp - 7), [Hp - 7, Hp - shift), [Hp - shift, Hp) per axis, label 3 * hr + wr
    if (shift) lb = 3 * ((sy >= Hp - 7 ? 1 : 0) + (sy >= Hp - shift ? 1 : 0)) + (sx >= Wp - 7 ? 1 : 0) + (sx >= Wp - shift ? 1 : 0);
  }
  tok[lane] = tk;
  lab[lane] = lb;
  for (int i = lane; i < 169; i += 64) rb[i] = table[i * heads + head];
  {
    // slot `lane`: K row and V^T column (projection output, biases for a pad token, zeros for filler)
    float kf[32], vf[32];
    if (tk >= 0) {
      const T* kp = base + (long)tk * C3 + C + head * 32;
#pragma unroll
      for (int c = 0; c < 32 / CH; ++c) {
        chunk_to_f<T>(*reinterpret_cast<const uint4*>(kp + c * CH), kf + c * CH);
        chunk_to_f<T>(*reinterpret_cast<const uint4*>(kp + C + c * CH), vf + c * CH);
      }
    } else {
      const bool pad = lane < 49;
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        kf[e] = pad ? qkv_bias[C + head * 32 + e] : 0.f;
        vf[e] = pad ? qkv_bias[2 * C + head * 32 + e] : 0.f;
      }
    }
#pragma unroll
    for (int c = 0; c < 32 / CH; ++c) *reinterpret_cast<uint4*>(ks + lane * KROW + c * 16) = f_to_chunk<T>(kf + c * CH);
#pragma unroll
    for (int e = 0; e < 32; ++e) *reinterpret_cast<T*>(vt + e * VROW + lane * (int)sizeof(T)) = Elem<T>::from_f(vf[e]);
  }
  __syncthreads();
  const float scale = 0.17677669529663687f;   // 32 ** -0.5
  for (int qt = 0; qt < 4; ++qt) {
    const int qi = qt * 16 + lr;               // query slot of this lane's column
    const int qtk = qi < 49 ? tok[qi] : -1;    // (pad / filler queries: zeros, never stored)
    const T* qp = base + (long)(qtk >= 0 ? qtk : 0) * C3 + head * 32 + 8 * g;
    f32x4_t acc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) acc[kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(T) == 2) {
      // A = K (row key, k = dims 8 g .. 8 g + 7), B = Q^T (column query): one K step covers the head
      const u32x4 qf = qtk >= 0 ? *reinterpret_cast<const u32x4*>(qp) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(ks + (kt * 16 + lr) * KROW + 16 * g);
        acc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, qf), acc[kt], 0, 0, 0);
      }
    } else {
      // K step s, lane group g <-> dim 8 g + s on both operands
      float qf[8];
      {
        const float4 v0 = qtk >= 0 ? *reinterpret_cast<const float4*>(qp) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 v1 = qtk >= 0 ? *reinterpret_cast<const float4*>(qp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        qf[0] = v0.x; qf[1] = v0.y; qf[2] = v0.z; qf[3] = v0.w; qf[4] = v1.x; qf[5] = v1.y; qf[6] = v1.z; qf[7] = v1.w;
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const unsigned char* kr = ks + (kt * 16 + lr) * KROW + 32 * g;
        const float4 k0 = *reinterpret_cast<const float4*>(kr), k1 = *reinterpret_cast<const float4*>(kr + 16);
        const float kf[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qf[s], acc[kt], 0, 0, 0);
      }
    }
    // ---- scale, relative-position bias, shift mask (-100, not -inf), filler keys (-inf); softmax over the keys of query qi
    const int qs = qi < 49 ? qi : 0;
    const int qy = qs / 7, qx = qs - qy * 7, ql = lab[qs];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt * 16 + 4 * g + r;
        float v = -INFINITY;
        if (j < 49) {
          const int jy = j / 7, jx = j - jy * 7;
          float add = rb[(qy - jy + 6) * 13 + (qx - jx + 6)];
          if (lab[j] != ql) add += -100.f;
          v = acc[kt][r] * scale + add;
        }
        acc[kt][r] = v;
        m = fmaxf(m, v);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[kt][r] = __expf(acc[kt][r] - m);
        sum += acc[kt][r];
      }
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.f / sum;
    // ---- O^T = V^T P^T: two 16-channel tiles
    f32x4_t o[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {   // 32 keys per step: slots e < 4 <- tile 2s row 4g + e, e >= 4 <- tile 2s+1 row 4g + e - 4
        u32x4 pf;
        pf.x = (unsigned)f32_to_bf16(acc[2 * s][0]) | ((unsigned)f32_to_bf16(acc[2 * s][1]) << 16);
        pf.y = (unsigned)f32_to_bf16(acc[2 * s][2]) | ((unsigned)f32_to_bf16(acc[2 * s][3]) << 16);
        pf.z = (unsigned)f32_to_bf16(acc[2 * s + 1][0]) | ((unsigned)f32_to_bf16(acc[2 * s + 1][1]) << 16);
        pf.w = (unsigned)f32_to_bf16(acc[2 * s + 1][2]) | ((unsigned)f32_to_bf16(acc[2 * s + 1][3]) << 16);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const unsigned char* vr = vt + (dt * 16 + lr) * VROW + (s * 32 + 4 * g) * 2;
          const uint2 lo = *reinterpret_cast<const uint2*>(vr);
          const uint2 hi = *reinterpret_cast<const uint2*>(vr + 32);
          const u32x4 vf = u32x4{lo.x, lo.y, hi.x, hi.y};
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf), __builtin_bit_cast(bf16x8_t, pf), o[dt], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {   // step r of tile kt: slot g <-> key 16 kt + 4 g + r = register r of the scores
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const float4 v4 = *reinterpret_cast<const float4*>(vt + (dt * 16 + lr) * VROW + (kt * 16 + 4 * g) * 4);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4.x, acc[kt][0], o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4.y, acc[kt][1], o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4.z, acc[kt][2], o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4.w, acc[kt][3], o[dt], 0, 0, 0);
        }
      }
    }
    // ---- O^T tile dt: column = query qi, rows = channels 16 dt + 4 g + reg -> 4 consecutive channels of the token row
    if (qtk >= 0) {
      T* op = out + ((long)b * H * W + qtk) * C + head * 32 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        if constexpr (sizeof(T) == 2) {
          uint2 pk;
          pk.x = (unsigned)f32_to_bf16(o[dt][0] * inv) | ((unsigned)f32_to_bf16(o[dt][1] * inv) << 16);
          pk.y = (unsigned)f32_to_bf16(o[dt][2] * inv) | ((unsigned)f32_to_bf16(o[dt][3] * inv) << 16);
          *reinterpret_cast<uint2*>(op + dt * 16) = pk;
        } else {
          *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ LayerNorm
// G lanes per row, up to MAXC 16-byte chunks per lane in registers (rows up to 4 x 768 channels: the patch merging of the last
// stage in fp32 is 384 chunks); mean, then the biased variance of the centred values, eps inside the square root — nn.LayerNorm.
// MERGE: the row is SwinPatchMerging's concatenation of four neighbours, quadrant q = (row offset q & 1, column offset q >> 1).
constexpr int LN_MAXC = 6;

template <typename T, int G, bool MERGE>
__global__ __launch_bounds__(256) void swin_ln_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      T* __restrict__ y, long rows, int C, int ld, float eps, int Ho, int Wo) {
  constexpr int CH = Elem<T>::CH;
  const int nch = C / CH;
  const int lane = threadIdx.x % G;
  const long row = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  const bool live = row < rows;
  long pix0 = 0;   // MERGE: source pixel (2 oy, 2 ox) of image b
  int Cq = 0, ncq = 1;
  if (MERGE && live) {
    const int ox = (int)(row % Wo);
    const long t = row / Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    Cq = C / 4; ncq = nch / 4;
    pix0 = (b * 2 * Ho + 2 * oy) * (2L * Wo) + 2 * ox;
  }
  float v[LN_MAXC][CH];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXC; ++i) {
    const int c = lane + i * G;
    const bool ok = live && c < nch;
#pragma unroll
    for (int e = 0; e < CH; ++e) v[i][e] = 0.f;
    if (ok) {
      const T* src;
      if (MERGE) {
        const int q = c / ncq, cc = c - q * ncq;
        src = x + (pix0 + (long)(q & 1) * 2 * Wo + (q >> 1)) * Cq + (long)cc * CH;
      } else {
        src = x + row * C + (long)c * CH;
      }
      chunk_to_f<T>(*reinterpret_cast<const uint4*>(src), v[i]);
    }
#pragma unroll
    for (int e = 0; e < CH; ++e) s += v[i][e];
  }
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXC; ++i) {
    const bool ok = lane + i * G < nch;
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      const float d = ok ? v[i][e] - mean : 0.f;
      q = fmaf(d, d, q);
    }
  }
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.f / sqrtf(q / (float)C + eps);
#pragma unroll
  for (int i = 0; i < LN_MAXC; ++i) {
    const int c = lane + i * G;
    if (live && c < nch) {
      float o[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) o[e] = fmaf((v[i][e] - mean) * rstd, gamma[c * CH + e], beta[c * CH + e]);
      *reinterpret_cast<uint4*>(y + row * ld + (long)c * CH) = f_to_chunk<T>(o);
    }
  }
}

// ------------------------------------------------------------------------------------------------- pyramid pooling, FPN
// nn.AdaptiveAvgPool2d(S): output bin i spans [floor(i n / S), ceil((i + 1) n / S)) per axis (bins overlap; with S > n several
// bins hold the same pixel).  One 16-byte channel chunk of one output pixel per thread, fp32 sums.
template <typename T>
__global__ __launch_bounds__(256) void swin_avgpool_kernel(const T* __restrict__ x, int ld, T* __restrict__ y, int B, int h, int w, int C,
                                                           int S) {
  constexpr int CH = Elem<T>::CH;
  const int nch = C / CH;
  const long total = (long)B * S * S * nch;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % nch);
    const long p = i / nch;
    const int ox = (int)(p % S), oy = (int)((p / S) % S);
    const long b = p / ((long)S * S);
    const int y0 = oy * h / S, y1 = ((oy + 1) * h + S - 1) / S;
    const int x0 = ox * w / S, x1 = ((ox + 1) * w + S - 1) / S;
    float acc[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] = 0.f;
    for (int yy = y0; yy < y1; ++yy)
      for (int xx = x0; xx < x1; ++xx) {
        float f[CH];
        chunk_to_f<T>(*reinterpret_cast<const uint4*>(x + ((b * h + yy) * w + xx) * ld + (long)c * CH), f);
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] += f[e];
      }
    const float inv = 1.f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] *= inv;
    *reinterpret_cast<uint4*>(y + p * C + (long)c * CH) = f_to_chunk<T>(acc);
  }
}

// y += bilinear(x), both dense NHWC; the sum in fp32, rounded once
template <typename T>
__global__ __launch_bounds__(256) void swin_bilinear_add_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int h, int w, int C, int H,
                                                                int W) {
  constexpr int CH = Elem<T>::CH;
  const int nch = C / CH;
  const long total = (long)B * H * W * nch;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % nch);
    const long p = i / nch;
    const int ox = (int)(p % W), oy = (int)((p / W) % H);
    const long b = p / ((long)W * H);
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_src(oy, h, H, y0, y1, ly);
    bilinear_src(ox, w, W, x0, x1, lx);
    float a[CH], bq[CH], cq[CH], d[CH], o[CH];
    const T* src = x + b * h * w * C + (long)c * CH;
    chunk_to_f<T>(*reinterpret_cast<const uint4*>(src + ((long)y0 * w + x0) * C), a);
    chunk_to_f<T>(*reinterpret_cast<const uint4*>(src + ((long)y0 * w + x1) * C), bq);
    chunk_to_f<T>(*reinterpret_cast<const uint4*>(src + ((long)y1 * w + x0) * C), cq);
    chunk_to_f<T>(*reinterpret_cast<const uint4*>(src + ((long)y1 * w + x1) * C), d);
    T* dst = y + p * C + (long)c * CH;
    chunk_to_f<T>(*reinterpret_cast<const uint4*>(dst), o);
#pragma unroll
    for (int e = 0; e < CH; ++e) o[e] += (1.f - ly) * ((1.f - lx) * a[e] + lx * bq[e]) + ly * ((1.f - lx) * cq[e] + lx * d[e]);
    *reinterpret_cast<uint4*>(dst) = f_to_chunk<T>(o);
  }
}

static inline int ew_blocks(long total) {
  long b = (total + 255) / 256;
  if (b > 256 * 16) b = 256 * 16;
  return (int)(b < 1 ? 1 : b);
}

template <typename T, bool MERGE>
int ln_launch(const void* x, const float* gamma, const float* beta, void* y, long rows, int C, int ld, float eps, int Ho, int Wo,
              hipStream_t s) {
  constexpr int CH = Elem<T>::CH;
  const int nch = C / CH;
  const int G = nch <= 16 * LN_MAXC ? 16 : nch <= 32 * LN_MAXC ? 32 : 64;
  if (nch > 64 * LN_MAXC) return -2;
  const long blocks = (rows * G + 255) / 256;
  if (blocks >= (1L << 31)) return -2;
  if (G == 16) hipLaunchKernelGGL((swin_ln_kernel<T, 16, MERGE>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)x, gamma, beta, (T*)y, rows, C, ld, eps, Ho, Wo);
  else if (G == 32) hipLaunchKernelGGL((swin_ln_kernel<T, 32, MERGE>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)x, gamma, beta, (T*)y, rows, C, ld, eps, Ho, Wo);
  else hipLaunchKernelGGL((swin_ln_kernel<T, 64, MERGE>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)x, gamma, beta, (T*)y, rows, C, ld, eps, Ho, Wo);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int swin_window_attention(int dtype, const void* qkv, const float* qkv_bias, const float* table, void* out, int B, int H, int W, int C,
                          int heads, int shift, hipStream_t s) {
  if (C != 32 * heads || heads < 1 || shift < 0 || shift >= 7 || B < 1 || H < 1 || W < 1) return -2;
  const int Hp = (H + 6) / 7 * 7, Wp = (W + 6) / 7 * 7;
  const int nwx = Wp / 7, nwin = (Hp / 7) * nwx;
  if (B > 65535) return -2;
  dim3 grid((unsigned)nwin, (unsigned)heads, (unsigned)B);
  // 49 x 49 x 32 x 2 multiply-adds per window and head (the padded 64-slot tiles are not counted)
  ProfScope ps(dtype == DT_F32 ? "swin_attention_f32" : "swin_attention_bf16", 4.0 * 49 * 49 * 32 * (double)nwin * heads * B,
               (double)B * H * W * 4 * C * dtype_size(dtype), s);
  if (dtype == DT_F32)
    hipLaunchKernelGGL(swin_attention_kernel<float>, grid, dim3(64), 0, s, (const float*)qkv, qkv_bias, table, (float*)out, H, W, C, heads, shift, Hp, Wp, nwx);
  else
    hipLaunchKernelGGL(swin_attention_kernel<bf16_t>, grid, dim3(64), 0, s, (const bf16_t*)qkv, qkv_bias, table, (bf16_t*)out, H, W, C, heads, shift, Hp, Wp, nwx);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int swin_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, long rows, int C, int ld, float eps,
                   hipStream_t s) {
  const int ch = dtype == DT_F32 ? 4 : 8;
  if ((C % ch) || (ld % ch) || ld < C) return -2;
  ProfScope ps("swin_layernorm", 0.0, 2.0 * rows * C * dtype_size(dtype), s);
  return dtype == DT_F32 ? ln_launch<float, false>(x, gamma, beta, y, rows, C, ld, eps, 0, 0, s)
                         : ln_launch<bf16_t, false>(x, gamma, beta, y, rows, C, ld, eps, 0, 0, s);
}

int swin_patch_merge_ln(int dtype, const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps,
                        hipStream_t s) {
  const int ch = dtype == DT_F32 ? 4 : 8;
  if ((C % ch) || (H & 1) || (W & 1)) return -2;
  const long rows = (long)B * (H / 2) * (W / 2);
  ProfScope ps("swin_patch_merge_ln", 0.0, 2.0 * rows * 4 * C * dtype_size(dtype), s);
  return dtype == DT_F32 ? ln_launch<float, true>(x, gamma, beta, y, rows, 4 * C, 4 * C, eps, H / 2, W / 2, s)
                         : ln_launch<bf16_t, true>(x, gamma, beta, y, rows, 4 * C, 4 * C, eps, H / 2, W / 2, s);
}

int swin_adaptive_avgpool(int dtype, const void* x, int ld, void* y, int B, int h, int w, int C, int S, hipStream_t s) {
  const int ch = dtype == DT_F32 ? 4 : 8;
  if ((C % ch) || (ld % ch) || ld < C || S < 1) return -2;
  const long total = (long)B * S * S * (C / ch);
  ProfScope ps("swin_avgpool", 0.0, ((double)B * h * w * C + (double)B * S * S * C) * dtype_size(dtype), s);
  if (dtype == DT_F32) hipLaunchKernelGGL(swin_avgpool_kernel<float>, dim3(ew_blocks(total)), dim3(256), 0, s, (const float*)x, ld, (float*)y, B, h, w, C, S);
  else hipLaunchKernelGGL(swin_avgpool_kernel<bf16_t>, dim3(ew_blocks(total)), dim3(256), 0, s, (const bf16_t*)x, ld, (bf16_t*)y, B, h, w, C, S);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int swin_bilinear_add(int dtype, const void* x, void* y, int B, int h, int w, int C, int H, int W, hipStream_t s) {
  const int ch = dtype == DT_F32 ? 4 : 8;
  if (C % ch) return -2;
  const long total = (long)B * H * W * (C / ch);
  ProfScope ps("swin_bilinear_add", 0.0, ((double)B * H * W * C * 2 + (double)B * h * w * C) * dtype_size(dtype), s);
  if (dtype == DT_F32) hipLaunchKernelGGL(swin_bilinear_add_kernel<float>, dim3(ew_blocks(total)), dim3(256), 0, s, (const float*)x, (float*)y, B, h, w, C, H, W);
  else hipLaunchKernelGGL(swin_bilinear_add_kernel<bf16_t>, dim3(ew_blocks(total)), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, B, h, w, C, H, W);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
