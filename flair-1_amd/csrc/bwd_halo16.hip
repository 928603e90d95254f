// Fused backward of the 16 -> 16 (padded) channel 3x3 / stride-1 / pad-1 convolutions of the full-resolution decoder tail
// (decoder block 4's second convolution and the segmentation head), bf16.
//
// The separate path runs three kernels per layer over 268 MB tensors (16 ch x 512^2 x 32) that never survive in the caches from one
// kernel to the next: bn_bwd_apply (reads dz, y, writes dy), the data gradient conv3x3_halo_p_kernel<16,16,false,BNR> (reads dy with
// its halo, the upstream y for the fused BatchNorm-backward sums, writes dx) and the weight gradient wgrad3x3_halo_kernel<16,16,LZ>
// (reads dy and the lazy input again).  Here a persistent workgroup stages, per 8x32 tile, the output gradient with its halo ONCE
// (the unit flavour forms dy = k1*dz*m + k2*y + k3 on the way: dy never reaches HBM) and the layer input with its halo ONCE (the
// lazy BatchNorm + ReLU image for the weight gradient, the raw centre rows for the reduction), and feeds both products from them:
//   * data gradient: the K steps, fragment and accumulation order and the register epilogue of conv3x3_halo_p_kernel<bf16,16,16>,
//     the DirectBnr sums with y taken from LDS;
//   * weight gradient: the transposed-read MFMAs of wgrad3x3_halo_kernel<bf16,16,16>: same pixel -> K-slot map (tr_frag.h), same K
//     split over the four waves, same merge order, one fp32 slab per workgroup, summed by launch_wgrad_reduce;
//   * head flavour: the bias-gradient partials of the DB variant, in its per-thread and per-workgroup order.
// With the same tile -> workgroup deal the results are bit for bit those of the three kernels.
//
// Prefetch: two register slots.  The k-th tile of a workgroup's walk (tiles blockIdx.x + k * gridDim.x) rides in slot A for even
// k and in slot B for odd k; while tile k is multiplied, tile k + 1 waits in the other slot and tile k + 2 is requested into the
// slot tile k was staged from.  Inside a slot the sources are requested, and later put to LDS, in the order gradient, (unit
// flavour: the unit's y,) layer input.
#include "bwd_halo16.h"

#include <string.h>

#include "halo_stage.h"
#include "launch.h"
#include "mma.h"
#include "ops.h"
#include "tile_direct.h"
#include "tile_store.h"
#include "tr_frag.h"
#include "tune.h"

namespace flair {

void launch_wgrad_reduce(const float* partial, float* dw, int splits, int Cout, int Cout_pad, int Kpad, int Cin,
                         int Cin_real, int R, int S, int accumulate, hipStream_t s);  // wgrad.hip

namespace {

typedef bf16_t T;
constexpr int TH = 8, TW = 32, HW_ = TW + 2, HPIX = (TH + 2) * HW_;   // 340 halo pixels
constexpr int C = 16, CH = 8, CPP = C / CH;
constexpr int HIT = (HPIX * CPP + 255) / 256;                         // staging items per thread and source
constexpr int KF = 4 * CH, KW = (9 * C + KF - 1) / KF * KF, NK = KW / KF;   // data-gradient K: 144 -> 160, five steps
constexpr int WROW = KW * (int)sizeof(T) + 16;                        // weight row in LDS (HaloCfg::WROW)
constexpr int PSTR = C * (int)sizeof(T) + 16;                         // bytes per halo pixel of both images (WgHaloCfg::XSTRIDE): the
                                                                      // 16-byte row reads of the data gradient are conflict-free on it too
constexpr int KG = 9 * C;                                             // slab row
constexpr int WOFF = 0, GOFF = (C * WROW + 255) / 256 * 256, XOFF = GOFF + (HPIX * PSTR + 255) / 256 * 256,
              YOFF = XOFF + (HPIX * PSTR + 255) / 256 * 256,          // raw centre rows of the layer input, 32 bytes per pixel
              SOFF = YOFF + TH * TW * C * (int)sizeof(T), COFF = SOFF + 4 * C * 2 * 4, SMEM = COFF + 9 * C * 4;
static_assert(HPIX * PSTR >= 9 * 4 * 64 * 4 && HPIX * PSTR >= 256 * CH * 4, "merge and bias buffers reuse the images");

template <bool UNIT>
__global__ __launch_bounds__(256, 2) void bwd16_fused_kernel(const Bwd16Args a, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wl = smem + WOFF;
  unsigned char* gimg = smem + GOFF;
  unsigned char* ximg = smem + XOFF;
  unsigned char* yraw = smem + YOFF;
  float* st = reinterpret_cast<float*>(smem + SOFF);
  // per-channel coefficients, read from LDS where they are used (held in registers they put 120-140 bytes per lane into scratch at
  // two workgroups per CU): the unit flavour's k1 | k2 | k3 | mask scale | mask shift, then lazy scale | lazy shift of the layer
  // input and scale | shift of the reduction's mask
  float* ctab = reinterpret_cast<float*>(smem + COFF);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int H = a.H, W = a.W;
  const int tiles_x = W / TW, tiles_y = H / TH;
  const int G = gridDim.x;
  const HaloSrc<T> gsrc{(const T*)a.g, H, W, C, 0, 0};
  const HaloSrc<T> ysrc{(const T*)a.gy, H, W, C, 0, 0};
  const HaloSrc<T> xsrc{(const T*)a.x, H, W, C, 0, 0};
  T* __restrict__ dx = (T*)a.dx;

  // data-gradient weights: all nine taps of the 16 rows, once per launch; the padded K tail is zero
  {
    const T* __restrict__ wp = (const T*)a.w;
    for (int it = t; it < C * (KW - 9 * C) / CH; it += 256) {
      const int row = it / ((KW - 9 * C) / CH), pc = it - row * ((KW - 9 * C) / CH);
      *reinterpret_cast<u32x4*>(wl + row * WROW + (9 * C + pc * CH) * (int)sizeof(T)) = u32x4{0u, 0u, 0u, 0u};
    }
    for (int it = t; it < C * 9 * CPP; it += 256) {
      const int row = it / (9 * CPP), rem = it - row * (9 * CPP);
      const int tap = rem / CPP, ch = rem - tap * CPP;
      *reinterpret_cast<u32x4*>(wl + row * WROW + rem * 16) = *reinterpret_cast<const u32x4*>(wp + (long)row * a.Kpad + tap * C + ch * CH);
    }
  }
  if constexpr (UNIT) {
    if (t < 5 * C) ctab[t] = t < 3 * C ? a.gcoef[t] : (t < 4 * C ? a.gmsc[t - 3 * C] : a.gmsh[t - 4 * C]);
  }
  if (t >= 5 * C && t < 9 * C) {
    const int j = (t - 5 * C) / C, c = t % C;
    ctab[t] = j == 0 ? a.in_scale[c] : j == 1 ? a.in_shift[c] : j == 2 ? a.bnr_scale[c] : a.bnr_shift[c];
  }
  float r1[4], r2[4];   // DirectBnr sums: channel 4 * lq + e
#pragma unroll
  for (int e = 0; e < 4; ++e) { r1[e] = 0.f; r2[e] = 0.f; }
  const bool bnr_per_tile = a.bnr_cols != G;   // one partial column per tile instead of one per workgroup
  f32x4_t wacc[9];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp) wacc[tp] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) bsum[e] = 0.f;

  u32x4 gA[HIT], yA[HIT], xA[HIT], gB[HIT], yB[HIT], xB[HIT];
  unsigned bitsA = 0, bitsB = 0;
  auto tile_load = [&](int tile, u32x4 (&gr)[HIT], u32x4 (&yr)[HIT], u32x4 (&xr)[HIT], unsigned& bits) {
    const bool tok = tile < ntiles;
    int n, y0, x0;
    tile_decode<TW, TH>(tok ? tile : 0, tiles_x, tiles_y, n, y0, x0);
    halo_gather<T, TW, TH, CPP, 256>(gsrc, tok, n, y0, x0, H, W, t, gr, bits);
    if constexpr (UNIT) halo_gather<T, TW, TH, CPP, 256>(ysrc, tok, n, y0, x0, H, W, t, yr, bits);
    halo_gather<T, TW, TH, CPP, 256>(xsrc, tok, n, y0, x0, H, W, t, xr, bits);   // (the three masks are the same)
  };
  auto tile_stage = [&](const u32x4 (&gr)[HIT], const u32x4 (&yr)[HIT], const u32x4 (&xr)[HIT], unsigned bits) {
#pragma unroll
    for (int k = 0; k < HIT; ++k) {
      const int it = t + 256 * k;
      if (it < HPIX * CPP) {
        const int hp = it / CPP, ch = it - hp * CPP;
        const unsigned mask = 0u - ((bits >> k) & 1u);
        u32x4 gv = gr[k];
        if constexpr (UNIT) {   // bn_bwd_apply_kernel, mask from y
          float d[CH], yy[CH], gg[CH];
          chunk_to_f<T>(__builtin_bit_cast(uint4, gr[k]), d);
          chunk_to_f<T>(__builtin_bit_cast(uint4, yr[k]), yy);
          const float* cf = ctab + ch * CH;
#pragma unroll
          for (int e = 0; e < CH; ++e) {
            d[e] = fmaf(yy[e], cf[3 * C + e], cf[4 * C + e]) > 0.f ? d[e] : 0.f;
            gg[e] = fmaf(cf[e], d[e], fmaf(cf[C + e], yy[e], cf[2 * C + e]));
          }
          gv = __builtin_bit_cast(u32x4, f_to_chunk<T>(gg));
        }
        *reinterpret_cast<u32x4*>(gimg + hp * PSTR + ch * 16) = gv & mask;   // pixels outside the image are zero
        *reinterpret_cast<u32x4*>(ximg + hp * PSTR + ch * 16) = chunk_bn_relu<T>(xr[k], ctab + 5 * C + ch * CH, ctab + 6 * C + ch * CH) & mask;
        const int hy = hp / HW_, hx = hp - hy * HW_;
        if (hy >= 1 && hy <= TH && hx >= 1 && hx <= TW)   // the tile's own pixels, untransformed: y of the fused reduction
          *reinterpret_cast<u32x4*>(yraw + ((hy - 1) * TW + hx - 1) * (C * (int)sizeof(T)) + ch * 16) = xr[k];
      }
    }
  };

  tile_load(blockIdx.x, gA, yA, xA, bitsA);
  tile_load(blockIdx.x + G, gB, yB, xB, bitsB);
  __syncthreads();   // the coefficient table
  tile_stage(gA, yA, xA, bitsA);
  __syncthreads();
  // one tile: request tile + 2 strides into the slot that is free (`ld`), both products from LDS, stage the next tile from the
  // other slot (`st*`)
  auto do_tile = [&](int tile, u32x4 (&ldg)[HIT], u32x4 (&ldy)[HIT], u32x4 (&ldx)[HIT], unsigned& ldbits, const u32x4 (&stg)[HIT],
                     const u32x4 (&sty)[HIT], const u32x4 (&stx)[HIT], const unsigned& stbits) {
    tile_load(tile + 2 * G, ldg, ldy, ldx, ldbits);
    __builtin_amdgcn_sched_barrier(0);
    // ---- data gradient (conv3x3_halo_p_kernel<bf16, 16, 16>): weights are the MFMA's A operand, D = [channel][pixel]
    f32x4_t acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto rdk = [&](u32x4 (&af)[4], u32x4& bfr, int j) {
      const int k0 = j * KF + lq * CH;
      int tap = k0 / C;
      const int c = k0 - tap * C;
      tap = tap > 8 ? 8 : tap;  // padded K: the weights there are zero, any valid address will do
      const int r = tap / 3, s = tap - 3 * r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int py = 2 * wave + (i >> 1), px = (i & 1) * 16 + lr;
        af[i] = *reinterpret_cast<const u32x4*>(gimg + ((py + r) * HW_ + px + s) * PSTR + c * (int)sizeof(T));
      }
      bfr = *reinterpret_cast<const u32x4*>(wl + direct_row_channel<1>(0, lr) * WROW + k0 * (int)sizeof(T));
    };
    auto mmk = [&](const u32x4 (&af)[4], const u32x4& bfr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) Mma<T>::run(bfr, af[i], acc[i]);
    };
    // (plain K loop: with the read-ahead fragment sets of the stand-alone kernel this one, which also carries the weight-gradient
    // accumulators and a third staged source per slot, spills 36-40 bytes per lane at two workgroups per CU)
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      u32x4 af[4], bfr;
      rdk(af, bfr, j);
      mmk(af, bfr);
    }
    {
      int n, y0, x0;
      tile_decode<TW, TH>(tile, tiles_x, tiles_y, n, y0, x0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int py = 2 * wave + (i >> 1), px = (i & 1) * 16 + lr;
        float f[4], yv[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) f[rr] = Elem<T>::to_f(Elem<T>::from_f(acc[i][rr]));
        LaneVec<T, 4>::store(dx + ((long)(n * H + y0 + py) * W + x0 + px) * C + 4 * lq, f);
        LaneVec<T, 4>::load(reinterpret_cast<const T*>(yraw + (py * TW + px) * (C * (int)sizeof(T))) + 4 * lq, yv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // DirectBnr::item
          const float d = Elem<T>::to_f(Elem<T>::from_f(f[e]));
          const float dm = fmaf(yv[e], ctab[7 * C + 4 * lq + e], ctab[8 * C + 4 * lq + e]) > 0.f ? d : 0.f;
          r1[e] += dm;
          r2[e] = fmaf(dm, yv[e], r2[e]);
        }
      }
    }
    // ---- weight gradient (wgrad3x3_halo_kernel<bf16, 16, 16>): this wave's two tile rows, all nine taps
#pragma unroll
    for (int yy = 0; yy < 2; ++yy) {
      const int y = wave * 2 + yy;
      const u32x4 af = HFrag<T>::template load<PSTR>(gimg, (y + 1) * HW_ + 1, 0, lane);
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int r = tp / 3, s = tp - 3 * r;
        const u32x4 bf = HFrag<T>::template load<PSTR>(ximg, (y + r) * HW_ + s, 0, lane);
        Mma<T>::run(af, bf, wacc[tp]);
      }
    }
    if constexpr (!UNIT) {
      if (a.dbias_partial) {   // column sums of the gradient tile, grouped as the DB variant's staging threads group them
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int px = (t + 256 * k) / CPP, py = px / TW, pxx = px - py * TW;
          float f[CH];
          chunk_to_f<T>(*reinterpret_cast<const uint4*>(gimg + ((py + 1) * HW_ + pxx + 1) * PSTR + (t % CPP) * 16), f);
#pragma unroll
          for (int e = 0; e < CH; ++e) bsum[e] += f[e];
        }
      }
    }
    if (bnr_per_tile) {
      direct_stats_wave<1>(r1, r2, st, C, 0, wave, lane);
      __syncthreads();
      tile_stats_write<4, C>(st, a.bnr_partial, a.bnr_C, 0, a.bnr_cols, tile, t);
#pragma unroll
      for (int e = 0; e < 4; ++e) { r1[e] = 0.f; r2[e] = 0.f; }
    }
    __syncthreads();   // every wave is done with the images
    tile_stage(stg, sty, stx, stbits);
    __syncthreads();   // next images visible
  };
  for (int tile = blockIdx.x; tile < ntiles; tile += 2 * G) {
    do_tile(tile, gA, yA, xA, bitsA, gB, yB, xB, bitsB);   // slot A went to LDS before this tile; B holds the next one
    if (tile + G < ntiles) do_tile(tile + G, gB, yB, xB, bitsB, gA, yA, xA, bitsA);
  }

  if (!bnr_per_tile) {   // one partial per workgroup and channel: [2][bnr_C][gridDim.x]
    direct_stats_wave<1>(r1, r2, st, C, 0, wave, lane);
    __syncthreads();
    tile_stats_write<4, C>(st, a.bnr_partial, a.bnr_C, 0, G, blockIdx.x, t);
  }
  if constexpr (!UNIT) {
    if (a.dbias_partial) {   // workgroup sum of the gradient columns, fixed order
      float* bs = reinterpret_cast<float*>(ximg);
#pragma unroll
      for (int e = 0; e < CH; ++e) bs[t * CH + e] = bsum[e];
      __syncthreads();
      if (t < C) {
        const int chunk = t / CH, e = t - chunk * CH;
        float x = 0.f;
        for (int th = chunk; th < 256; th += CPP) x += bs[th * CH + e];
        a.dbias_partial[(long)t * G + blockIdx.x] = x;
      }
    }
  }
  // ---- merge the K parts (fixed order wave 0 <- 1, 2, 3), then one slab per workgroup
  float* red = reinterpret_cast<float*>(gimg);
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[(tp * 4 + e) * 64 + lane] = wacc[tp][e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int e = 0; e < 4; ++e) wacc[tp][e] += red[(tp * 4 + e) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* __restrict__ part = a.slabs + (long)blockIdx.x * C * KG;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int e = 0; e < 4; ++e) part[(long)(lq * 4 + e) * KG + tp * C + lr] = wacc[tp][e];
  }
}

}  // namespace

bool bwd16_fusable(int dtype, int flavour, const ConvArgs& a, const WgradArgs& w) {
  const int mode = tune("FLAIR_BWD16_FUSE", FLAIR_BWD16_FUSE_DEFAULT);
  if (!(mode == 1 || (mode == 2 && flavour == BWD16_HEAD) || (mode == 3 && flavour == BWD16_UNIT))) return false;
  if (dtype != DT_BF16) return false;
  // the data gradient: 16 -> 16 from one source, plain store, reduction of the upstream unit attached (mask from its y)
  if (a.R != 3 || a.S != 3 || a.out_mul != 1 || a.in_div != 1 || a.pad != 1) return false;
  if (a.C0 != C || a.C1 || a.up0 || a.Cout != C || a.out_ld != C || !a.out) return false;
  if (a.Hout != a.Hin || a.Wout != a.Win || (a.Hout % TH) || (a.Wout % TW)) return false;
  if (a.accumulate || a.acc_src || a.pool_c0 || a.out_skip || a.in_scale || a.stats || a.oscale || a.oshift || a.bias || a.ores ||
      a.orelu || a.out_nchw || a.out_sub || a.ncls || a.preds_u8 || a.ce_lab8 || a.ogelu)
    return false;
  if (!a.bnr_partial || !a.bnr_y || a.bnr_out || a.bnr_mask || a.bnr_C != C) return false;
  // the weight gradient: same gradient tensor, 16 wide; the lazy input IS the reduction's y
  if (w.R != 3 || w.S != 3 || w.stride != 1 || w.pad != 1 || w.C0 != C || w.C1 || w.up0 || w.dy_ld != C || w.Cout > C || w.accumulate)
    return false;
  if (w.N != a.N || w.Hin != a.Hout || w.Win != a.Wout || w.dy != a.src0 || w.fuse_y) return false;
  if (!w.in_scale || !w.in_shift || w.x0 != a.bnr_y) return false;
  return true;
}

int bwd16_grid(const WgradArgs& w) {
  const long ntiles = (long)w.N * w.Hin * w.Win / (TH * TW);
  long wgs = tune("FLAIR_BWD16_WGS", 0);
  if (wgs <= 0) wgs = (long)(wgrad_halo_workspace_bytes(DT_BF16, w) / ((size_t)C * KG * sizeof(float)));   // its slabs = its workgroups
  if (wgs < 1) wgs = 1;
  return (int)(wgs < ntiles ? wgs : ntiles);
}

size_t bwd16_workspace_bytes(int grid) { return (size_t)grid * C * KG * sizeof(float); }

int launch_bwd16(const Bwd16Args& a, hipStream_t s) {
  if ((a.H % TH) || (a.W % TW) || a.bnr_C != C || a.Cout > C) return -2;
  const long ntiles = (long)a.N * a.H * a.W / (TH * TW);
  const bool unit = a.gy != nullptr;
  const int grid = a.grid;
  if (grid < 1 || grid > ntiles) return -2;
  if (a.bnr_cols != grid && a.bnr_cols != ntiles) return -6;
  if (a.dbias && (unit || !a.dbias_partial || grid > WGRAD_DBIAS_ROWS)) return -6;
  Bwd16Args k = a;
  if (!a.dbias) k.dbias_partial = nullptr;
  // algorithmic cost: both products' MACs; every operand once (the separate kernels' helpers count the gradient twice)
  ConvArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.N = a.N; ca.Hout = a.H; ca.Wout = a.W; ca.C0 = C; ca.Cout = C; ca.Kg = KG;
  struct { int N, H, W, Cout, C0, C1, up0, dy_ld; } wa = {a.N, a.H, a.W, a.Cout, C, 0, 0, C};
  const ProfCost cd = conv_prof_cost(ca, sizeof(T), false, false), cw = wgrad3x3_prof_cost(wa, sizeof(T));
  const ProfCost cost{cd.flops + cw.flops, cd.bytes + (double)ntiles * TH * TW * C * sizeof(T) * (unit ? 2 : 1)};
  const int rc = unit ? launch_kernel<bwd16_fused_kernel<true>>("bwd16_fused_unit_bf16", cost, dim3(grid), dim3(256), SMEM, s, k, (int)ntiles)
                      : launch_kernel<bwd16_fused_kernel<false>>("bwd16_fused_head_bf16", cost, dim3(grid), dim3(256), SMEM, s, k, (int)ntiles);
  if (rc) return rc;
  launch_wgrad_reduce(a.slabs, a.dw, grid, a.Cout, C, KG, C, a.Cin_real, 3, 3, 0, s);
  if (a.dbias) {
    const int rb = partial_rows_sum(a.dbias_partial, grid, a.Cout, a.dbias, s);
    if (rb) return rb;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace flair
