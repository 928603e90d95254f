// Host-callable launchers of the elementwise / reduction kernels (bn.hip, misc.hip, ce_head.hip).
#pragma once
#include "common.h"
#include "conv_route.h"

namespace flair {

// ---- bn.hip
int bn_finalize(const float* partial, int nblk, int C, long count, const float* gamma, const float* beta,
                float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                float* mean_out, float* invstd_out, hipStream_t s);
int bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                   float* scale, float* shift, hipStream_t s);
int bn_act(int dtype, const void* y, const float* scale, const float* shift, const void* res, const float* rscale,
           const float* rshift, void* out, long rows, int C, int relu, hipStream_t s);
int bn_bwd_blocks(long rows);
int bn_backward(int dtype, const void* dout, const void* out, const void* y, const float* mean, const float* invstd,
                const float* gamma, long rows, int C, float* partial, float* coef, float* dgamma, float* dbeta,
                int accumulate_param, void* dy, void* dres, int dres_accumulate, const float* mscale, const float* mshift,
                int pre_nblk /* > 0: partial already holds that many producer-side tile sums */,
                int premasked /* dout is dz already (ConvArgs::bnr_mask): no mask source needed; requires pre_nblk > 0 */, hipStream_t s);

int partial_rows_sum(const float* partial, int nblk, int ncols, float* out, hipStream_t s);
int bn_stats_partial(int dtype, const void* y, long rows, int C, float* partial, float* zeros_ones, hipStream_t s);
int colsum(int dtype, const void* x, long rows, int ld, int C, float* partial, float* out, hipStream_t s);

// ---- misc.hip
int maxpool3x3s2_fwd(int dtype, const void* in, void* out, unsigned char* idx, int N, int H, int W, int C, hipStream_t s);
// act = relu(y * scale + shift) and its 3x3 / stride-2 max pool (+ tap indices) in one pass (the stem in training mode)
int bn_act_maxpool3x3s2(int dtype, const void* y, const float* scale, const float* shift, void* act, void* out, unsigned char* idx, int N, int H,
                        int W, int C, hipStream_t s);
int maxpool3x3s2_bwd(int dtype, const void* dout, const unsigned char* idx, void* din, int accumulate, int N, int H,
                     int W, int C, hipStream_t s, const void* bnr_y = nullptr, const float* bnr_msc = nullptr,
                     const float* bnr_msh = nullptr, float* bnr_partial = nullptr);   // bnr_*: fused BN-backward reduction, [2][C][N*H] partials
int upcat_bwd(int dtype, const void* dcat, void* dx0, int dx0_accumulate, void* dskip, int dskip_accumulate, int N,
              int H, int W, int C0, int C1, hipStream_t s);
int nchw_f32_to_nhwc(int dtype, const float* in, void* out, int N, int C, int H, int W, int Cp, hipStream_t s);
int nhwc_to_nchw_f32(int dtype, const void* in, float* out, int N, int C, int H, int W, int Cp, float* accumulate_into,
                     hipStream_t s);
int pack_weight(int dtype, const float* w_oihw, void* dst, int Cout, int Cin, int R, int S, int Cin_p, int rows_pad,
                int Kpad, int transpose_flip, hipStream_t s);
struct PackDesc {
  long w_off;      // float offset of the OIHW master in the flat parameter buffer
  size_t dst_off;  // byte offset of the packed copy from the arena base
  int Cout, Cin, R, S, Cin_p, rows_pad, Kpad, tf;
  // tap subset of the packed copy: packed tap (ri, si), ri < Rc, si < Sc, is tap (r0 + ri*rstep, s0 + si*sstep) of the
  // full R x S pack (Rc = 0: all taps).  Used by the parity classes of a stride-2 data gradient.
  unsigned char r0, rstep, Rc, s0, sstep, Sc, pad_[2];
};
// full R x R pack of one layer: tf = 0 the forward [Cout][(r,s),Cin_p] copy, tf = 1 the flipped / transposed data-gradient copy
inline PackDesc pack_desc(long w_off, size_t dst_off, int Cout, int Cin, int R, int Cin_p, int rows_pad, int Kpad, int tf) {
  PackDesc d = {};
  d.w_off = w_off; d.dst_off = dst_off; d.Cout = Cout; d.Cin = Cin; d.R = R; d.S = R;
  d.Cin_p = Cin_p; d.rows_pad = rows_pad; d.Kpad = Kpad; d.tf = tf;
  return d;
}
struct PackTable {
  static constexpr int MAX = 64;
  int n;
  PackDesc d[MAX];
};
int pack_weights_all(int dtype, const float* params, void* base, const PackTable& tb, hipStream_t s);
int sgd_step(float* params, const float* grads, long n, float lr, hipStream_t s);
int add_rowvec_nchw(float* x, const float* v, int N, int C, int H, int W, hipStream_t s);
// x[n][h][w][c] += v[n*H + h] on an NHWC tensor of the compute dtype, in place (C a multiple of 8, x 16-byte aligned)
int add_rowvec_nhwc(int dtype, void* x, const float* v, int N, int H, int W, int C, hipStream_t s);
// y[n][h][w][c] = T(float(x[n][h][w][c]) + v[n*H + h]): the same add out of place (x == y allowed), for a training forward, where x
// is still needed as it is
int add_rowvec_nhwc_to(int dtype, const void* x, const float* v, void* y, int N, int H, int W, int C, hipStream_t s);
// dv[n*H + h] = sum over w, c of dx[n][h][w][c]: the gradient of either add with respect to v; fp32, fixed order, no atomics
int rowvec_grad_nhwc(int dtype, const void* dx, float* dv, int N, int H, int W, int C, hipStream_t s);
int ew_add(int dtype, void* dst, const void* src, long n, hipStream_t s);
int fill_zero(void* p, size_t bytes, hipStream_t s);
int fill_f32(float* p, long n, float v, hipStream_t s);

// ---- optim.hip: update rules over a flat fp32 buffer.  g' = g * grad_scale * coef (coef: optional device float)
int optim_sgd(float* params, const float* grads, float* buf, long n, float lr, float momentum, float dampening, float weight_decay,
              int nesterov, int first, float grad_scale, const float* coef, hipStream_t s);
int optim_adamw(float* params, const float* grads, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                float weight_decay, float bc1, float bc2, int first, float grad_scale, const float* coef, hipStream_t s);
int grad_sqnorm_partials();   // fp64 elements of grad_sqnorm's workspace
int grad_sqnorm(const float* grads, long n, double* partials, double* sum, int accumulate, hipStream_t s);
int clip_coef(const double* sum, float grad_scale, float max_norm, float* norm, float* coef, hipStream_t s);

// ---- ce_head.hip
struct CeArgs {
  const float* logits;        // NCHW fp32 [B][C][H][W]   (or null with logits_nhwc set)
  const void* logits_nhwc = nullptr;   // NHWC T [B*H*W][logits_ld]: the head convolution's own output layout
  int logits_dtype = 0, logits_ld = 0;
  const void* labels;         // label map, dtype per label_kind
  int label_kind;             // 0: uint8 [B][H][W]; 1: int32; 2: int64; 3: fp32 one-hot NCHW [B][C][H][W]
  const float* weight;        // optional class weights [C]
  int B, C, H, W;
  float* loss;                // out: scalar mean loss
  float* dlogits_nchw;        // optional out: fp32 NCHW gradient of the mean loss
  void* dlogits_nhwc;         // optional out: NHWC T gradient, row stride ld (>= C), padded columns zeroed; like logits_nhwc 16-byte aligned (-3)
  int dlogits_dtype, dlogits_ld;
  unsigned char* preds_u8;    // optional out [B][H][W]
  long long* preds_i64;       // optional out [B][H][W]
  int* targets_i32;           // optional out [B][H][W]
  long long* confmat;         // optional in/out [C][C] += bincount(target*C + pred)
  float* workspace;           // >= ce_workspace_floats() floats
};
size_t ce_workspace_floats(int B, int H, int W);
int ce_head(const CeArgs& a, hipStream_t s);
// The two ends of ce_head() for a caller whose per-pixel pass runs elsewhere (the CE flavour of the head convolution, ConvArgs::ce_lab8):
// ce_labels, the caller's pass with at most CE_MAX_BLOCKS loss partials, ce_finish.
constexpr int CE_MAX_BLOCKS = 2048;
struct CeWorkspace { unsigned char* lab8; float* den_partial; float* loss_partial; float* den; };
CeWorkspace ce_workspace_layout(float* workspace, long npix);
int ce_labels(const void* labels, int label_kind, const float* weight, int B, int C, int H, int W, int* targets_i32, float* workspace, hipStream_t s);
int ce_finish(float* workspace, long npix, int nblk, float* loss, hipStream_t s);
int softmax_argmax(const float* logits, int B, int C, int H, int W, unsigned char* preds_u8, long long* preds_i64,
                   float* maxprob, hipStream_t s);
int softmax_argmax_nhwc(const void* logits, int dtype, int ld, long npix, int C, unsigned char* preds_u8, long long* preds_i64,
                        float* maxprob, hipStream_t s);
int confmat_update(const void* target, int target_kind, const void* pred, int pred_kind, long n, int C,
                   long long* confmat, hipStream_t s);
int jaccard_from_confmat(const long long* confmat, int C, float* per_class, float* weighted, float* macro, hipStream_t s);

// ---- seg_loss.hip: the head with a configurable objective (label-smoothed / focal CE, soft Dice); the field order of
// flair_seg_loss_t (include/flair_hip.h)
struct SegLossSpec { float ce, label_smoothing, focal_gamma, dice, dice_smooth, dice_eps; };
struct SegLossArgs {
  const float* logits = nullptr;       // NCHW fp32 [B][C][H][W]   (or null with logits_nhwc set)
  const void* logits_nhwc = nullptr;   // NHWC T [B*H*W][ld], ld 16 or 32
  int dtype = 0, ld = 0;               // of logits_nhwc and of dl when the source is NHWC
  const void* labels = nullptr;
  int label_kind = 0;                  // as CeArgs::label_kind
  const float* weight = nullptr;       // optional class weights [C]
  int B = 0, C = 0, H = 0, W = 0;
  SegLossSpec spec = {};
  float* loss3 = nullptr;              // out: [loss, CE term, Dice term]
  void* dl = nullptr;                  // optional out: fp32 NCHW for the NCHW source, else NHWC T rows of stride ld, padding zeroed
  unsigned char* preds_u8 = nullptr;   // optional out [B][H][W]
  long long* preds_i64 = nullptr;      // optional out [B][H][W] (NCHW source only)
  int* targets_i32 = nullptr;          // optional out [B][H][W]
  long long* confmat = nullptr;        // optional in/out [C][C]
  float* workspace = nullptr;          // >= seg_loss_workspace_bytes() bytes
};
size_t seg_loss_workspace_bytes(int B, int C, int H, int W);
int seg_loss(const SegLossArgs& a, hipStream_t s);

// ---- feed.hip (rows either side of the hot path)
struct FeedArgs {
  static constexpr int MAXCH = 16;
  const unsigned char* img;     // [B][Cb][H][W] raster bands as stored
  const unsigned char* msk;     // optional [B][H][W] raw label raster (values 1..C as stored)
  const unsigned char* d4;      // optional [B] per-sample draw: bit0 V-flip, bit1 H-flip, bits 2-3 rot90 count
  float* out;                   // optional [B][Cout][H][W] fp32 NCHW (batch["img"])
  unsigned char* labels;        // optional [B][H][W] class index = argmax(batch["msk"], 1)
  int B, Cb, Cout, H, W;
  int mode;                     // 0 'without', 1 'scaling', 2 'custom'
  int num_classes;
  int band[MAXCH];              // 0-based band of output channel c (config "channels" minus one)
  double mean[MAXCH], stdv[MAXCH];
};
int feed_tiles(const FeedArgs& a, hipStream_t s);
// a.img / a.msk unused: sample b's (Cb, H, W) planes lie at img_ptrs[b] (0: the sample is skipped), its (H, W) mask at msk_ptrs[b]
int feed_tiles_ptrs(const FeedArgs& a, const unsigned long long* img_ptrs, const unsigned long long* msk_ptrs, hipStream_t s);
int gather_tiles(const FeedArgs& a, const int* tiles, int Hr, int Wr, hipStream_t s);  // a.img: one (Cb, Hr, Wr) raster
int detect_stitch_preds(const unsigned char* preds, const float* maxprob, int B, int S, int margin, const int* tiles, float* out,
                        int Hr, int Wr, hipStream_t s);
// `up` of the logits consumers: 1 = logits (B, C, S, S); 4 = (B, C, S/4, S/4), interpolated x4 per pixel (csrc/logit_source.h)
int detect_convert(const float* logits, int up, int B, int C, int S, int margin, int mode, void* out, const int* tiles, int Hr, int Wr,
                   hipStream_t s);
// zone_detect overlap stitching (csrc/zone_stitch.hip); rectangles are [x_lo, x_hi) x [y_lo, y_hi) of the raster
int detect_blend_accum(const float* logits, int up, int B, int C, int S, int margin, const int* tiles, const float* wtab, int x_lo, int x_hi,
                       int y_lo, int y_hi, float* ring, int Hr, int Wr, hipStream_t s);
int detect_blend_flush(float* ring, int C, int K, int x_lo, int x_hi, float* out, int Hr, int Wr, hipStream_t s);
int detect_stitch_max(const float* logits, int up, const unsigned char* preds, const float* maxprob, int B, int C, int S, int margin,
                      const int* tiles, int x_lo, int x_hi, int y_lo, int y_hi, float* out, int Hr, int Wr, hipStream_t s);
int confmat_masks(const unsigned char* truth, const unsigned char* pred, long n, int C, int truth_offset, long long* confmat,
                  hipStream_t s);
// test-time augmentation (csrc/tta.hip); code: the D4 packing of csrc/d4.h, -19 for an odd rot90 count with H != W
int d4_nchw_f32(const float* in, float* out, int B, int C, int H, int W, int code, hipStream_t s);
// one pass: acc (B, C, H, W) (+)= softmax of the transformed-frame logits, moved back to the original frame; `up` as above
int tta_accum(const float* logits, int up, int B, int C, int H, int W, int code, int first, float* acc, unsigned char* preds, float* prob,
              int n, hipStream_t s);
// zone_detect metrics (csrc/zone_metrics.hip); source 0: u8 class tiles (B, S, S), 1: fp32 logits (B, C, S, S), 2: fp32 raster,
// 3: fp32 quarter-resolution logits (B, C, S/4, S/4)
int zone_window_confmat(int source, const void* pred, int B, int C, int S, int margin, const int* tiles, const unsigned char* truth,
                        int Hr, int Wr, long long* confmats, hipStream_t s);
int zone_raster_confmat(const float* band, const unsigned char* truth, int Hr, int Wr, int C, long long* confmat, hipStream_t s);
int zone_error_map(const float* band, const unsigned char* truth, int Hr, int Wr, int K, const int* ys, int ny, const int* xs, int nx,
                   double sigma, int radius, unsigned char* mask, int* colsum, int* counts, double* tmp, double* out, hipStream_t s);
// TIFF 6.0 LZW streams, one per strip of R rows of a (B, H, W) u8 tensor (csrc/tiff_lzw.hip)
long tiff_lzw_slot_bytes(int R, int W);
int tiff_lzw_encode(const unsigned char* img, int B, int H, int W, int R, unsigned char* out, long slot_bytes, int* counts, hipStream_t s);
// the inverse, strip by strip from device tables: per-strip status (include/flair_hip.h), two launches (strips up to 16 KB, up to the cap)
// one stream per TIFF tile of a (bands, H, W) raster, u8 or fp32 with a per-band scale; packing streams out of their slots
long tiff_lzw_tile_slot_bytes(int T, int samples);
int tiff_lzw_encode_tiles(const void* raster, int src_f32, const float* scale, int bands, int H, int W, int T, int interleave,
                          long first_stream, long n_streams, unsigned char* out, long slot_bytes, int* counts, hipStream_t s);
int tiff_pack_streams(const unsigned char* slots, long slot_bytes, const int* counts, const long long* dst_off, long n_streams,
                      unsigned char* dst, long dst_bytes, hipStream_t s);
int tiff_lzw_decode_max_strip();
int tiff_lzw_decode(const unsigned char* src, long src_bytes, const long long* strip_src_off, const int* strip_src_len,
                    const long long* strip_dst_off, const int* strip_dst_len, const int* strip_mode, long nstrips, unsigned char* dst,
                    long dst_bytes, int* status, hipStream_t s);
// the chunks (tiles or strips) of a raster file into slots of a scratch buffer, any size up to the cap, and the slots into the band
// planes with the horizontal predictor undone (csrc/tiff_read.hip)
int tiff_lzw_decode_chunks_cap();
int tiff_lzw_decode_chunks_window();
int tiff_lzw_decode_chunks(const unsigned char* src, long src_bytes, const long long* src_off, const int* src_len, const int* dst_len,
                           const int* mode, long nchunks, unsigned char* scratch, long slot_bytes, int* status, hipStream_t s);
int tiff_chunks_to_planes(const unsigned char* scratch, long slot_bytes, const int* chunks, const int* status, long nchunks, int max_rows,
                          int samples, int predictor, unsigned char* planes, int bands, int H, int W, hipStream_t s);
// the same scatter for the chunks of a batch of files, samples and predictor per chunk (the tile loader)
int tiff_chunks_to_batch(const unsigned char* scratch, long slot_bytes, const int* chunks, const int* status, long nchunks, int max_rows,
                         unsigned char* planes, int n_planes, int H, int W, hipStream_t s);

}  // namespace flair
