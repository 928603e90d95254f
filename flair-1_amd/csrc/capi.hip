// extern "C" surface of libflair_hip.so — declarations and reference citations in include/flair_hip.h.
#include <new>
#include <string.h>

#include "../../include/flair_hip.h"
#include "unet.h"
#include "conv_args.h"
#include "parity_pack.h"
#include "segformer.h"
#include "upernet.h"
#include "segformer_ops.h"
#include "swin_ops.h"

using namespace flair;

struct flair_unet { UNet net; flair_unet(int a, int b, int c) : net(a, b, c) {} };
struct flair_segformer {
  SegFormer net;
  flair_segformer(int a, int b, const int* d, const int* h, const int* hd, const int* sr, int dh, int dt) : net(a, b, d, h, hd, sr, dh, dt) {}
};

struct flair_upernet {
  UperNet net;
  flair_upernet(int a, int b, int e, const int* d, const int* h, int hid, const int* ps, int ai, int ac, int dt)
      : net(a, b, e, d, h, hid, ps, ai, ac, dt) {}
};

// one entry of a transformer executor's tensor table (flair_segformer_tensor_info, flair_upernet_tensor_info)
static int tf_tensor_info(const std::vector<SfTensor>& tensors, int i, char* name, int name_cap, int64_t shape[4], int* ndim,
                          int64_t* offset, int* kind) {
  if (i < 0 || i >= (int)tensors.size() || !name || name_cap < 2) return -1;
  const SfTensor& t = tensors[i];
  strncpy(name, t.name.c_str(), name_cap - 1);
  name[name_cap - 1] = 0;
  for (int d = 0; d < 4; ++d) shape[d] = t.shape[d];
  *ndim = t.ndim; *offset = t.offset; *kind = t.kind;
  return 0;
}

// the arguments flair_feed_tiles and flair_feed_tiles_ptrs share, checked and packed; have_img: the call names image sources
static int feed_args(FeedArgs& a, bool have_img, const uint8_t* d4_flags, int B, int bands, int H, int W, const int* channels, int n_channels,
                     int norm_type, const double* means, const double* stds, int num_classes, float* img_out, uint8_t* labels_out) {
  if (!img_out && !labels_out) return -1;
  if (n_channels < 0 || n_channels > FeedArgs::MAXCH) return -2;
  if (img_out && (!have_img || !channels || n_channels < 1)) return -1;
  if (norm_type == 2 && (!means || !stds)) return -1;
  a.d4 = d4_flags; a.out = img_out; a.labels = labels_out;
  a.B = B; a.Cb = bands; a.Cout = img_out ? n_channels : 0; a.H = H; a.W = W; a.mode = norm_type; a.num_classes = num_classes;
  for (int c = 0; c < a.Cout; ++c) {
    a.band[c] = channels[c] - 1;  // config "channels" start at 1 (rasterio band numbering)
    a.mean[c] = norm_type == 2 ? means[c] : 0.0;
    a.stdv[c] = norm_type == 2 ? stds[c] : 1.0;
  }
  return 0;
}

extern "C" {

const char* flair_strerror(int code) {
  if (code == 0) return "ok";
  if (code > 0) return hipGetErrorString((hipError_t)code);
  switch (code) {
    case -1: return "null or invalid handle or argument (flair_unet_fwd_opts_t: maxprob_f32 needs preds_u8; ce_labels needs ce_loss, "
                    "ce_workspace and a ce_label_kind in 0..3; drows_f32 needs rows_f32)";
    case -2: return "channel count / pointer alignment not supported by the kernel";
    case -3: return "output rows too short for whole 16-byte chunks (channel count / row stride), or flair_ce_head(_nhwc): NHWC logits / "
                    "gradient rows not 16-byte aligned, workspace not 4-byte aligned";
    case -4: return "fused upsample needs even extents";
    case -5: return "unsupported stride";
    case -6: return "requested fused epilogue / input transform is not available in the kernel this shape dispatches to";
    case -7: return "diagnostic feature: rebuild with FLAIR_STAMPS=1";
    case -10: return "Wrong input shape: height and width must be divisible by 32";
    case -11: return "call order: backward / stage call without the matching forward on this workspace";
    case -12: return "gradient buffer already initialised";
    case -13: return "internal side stream: event record / wait failed";
    case -14: return "UperNet-Swin tile size: height and width must be multiples of 32 from 64 to 2048";
    case -15: return "flair_unet_fwd_opts_t: ce_labels needs an eval-mode forward without fp32 logits and without preds_u8";
    case -16: return "flair_unet_fwd_opts_t: rows_f32 in a training forward needs drows_f32 (the in-place add is for eval-mode forwards)";
    case -17: return "flair_unet_fwd_opts_t: drows_f32 is for a training forward (an eval-mode forward takes rows_f32 alone)";
    case -18: return "flair_unet_fwd_opts_t: the gradient that reaches the bottleneck tensor was stored masked, its sums into drows_f32 would be wrong";
    case -19: return "D4 transform code with an odd rot90 count needs a square tile (H == W)";
    case -20: return "flair_seg_loss_t: invalid specification (ce / dice negative or both 0, label_smoothing outside [0, 1), focal_gamma neither "
                     "0 nor >= 1, label_smoothing with focal_gamma, either without ce, dice_smooth < 0, dice_eps <= 0)";
    case -100: return "workspace too small";
    default: return "invalid argument";
  }
}

int flair_version(void) { return 1; }

int flair_unet_create(flair_unet_t** out, int in_channels, int classes, int dtype) {
  if (!out || in_channels < 1 || in_channels > 8 || classes < 1 || classes > 32 || (dtype != 0 && dtype != 1)) return -1;
  *out = new (std::nothrow) flair_unet(in_channels, classes, dtype);
  return *out ? 0 : -1;
}
void flair_unet_destroy(flair_unet_t* h) { delete h; }
int64_t flair_unet_param_count(const flair_unet_t* h) { return h ? h->net.n_params : -1; }
int64_t flair_unet_buffer_count(const flair_unet_t* h) { return h ? h->net.n_buffers : -1; }
int flair_unet_num_tensors(const flair_unet_t* h) { return h ? (int)h->net.tensors.size() : -1; }
int flair_unet_tensor_info(const flair_unet_t* h, int i, char* name, int name_cap, int64_t shape[4], int* ndim,
                           int64_t* offset, int* kind, int* stage) {
  if (!h || i < 0 || i >= (int)h->net.tensors.size()) return -1;
  const TensorInfo& t = h->net.tensors[i];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  for (int d = 0; d < 4; ++d) shape[d] = t.shape[d];
  *ndim = t.ndim; *offset = t.offset; *kind = t.kind; *stage = t.stage;
  return 0;
}
int flair_unet_stage_range(const flair_unet_t* h, int stage, int64_t* begin, int64_t* end) {
  if (!h || stage < 0 || stage > 6) return -1;
  *begin = h->net.stage_begin[stage]; *end = h->net.stage_begin[stage + 1];
  return 0;
}
int64_t flair_unet_workspace_bytes(flair_unet_t* h, int B, int H, int W, int training) {
  if (!h || B < 1 || (H % 32) || (W % 32)) return -1;
  return (int64_t)h->net.workspace_bytes(B, H, W, training);
}
int flair_unet_head_ld(const flair_unet_t* h) { return h ? h->net.convs.back().Cout_p : -1; }
int flair_unet_forward(flair_unet_t* h, const float* params, float* buffers, const float* x, float* logits, int B, int H,
                       int W, int training, void* ws, size_t wsb, void* stream, const flair_unet_fwd_opts_t* opts) {
  if (!h) return -1;
  FwdOpts o;
  if (opts) {
    o.reuse_constants = opts->reuse_constants != 0;
    o.preds = opts->preds_u8; o.maxprob = opts->maxprob_f32;
    o.ce.labels = opts->ce_labels; o.ce.kind = opts->ce_label_kind; o.ce.weight = opts->ce_class_weight; o.ce.loss = opts->ce_loss;
    o.ce.preds = opts->ce_preds_u8; o.ce.confmat = (long long*)opts->ce_confmat; o.ce.ws = (float*)opts->ce_workspace;
    o.rows = opts->rows_f32; o.drows = opts->drows_f32;
  }
  return h->net.forward(params, buffers, x, logits, B, H, W, training, ws, wsb, (hipStream_t)stream, o);
}
int flair_unet_backward(flair_unet_t* h, const float* params, const float* dl_nchw, const void* dl_nhwc, float* grads,
                        void* ws, size_t wsb, void* stream, void* const* stage_events) {
  if (!h || (!dl_nchw == !dl_nhwc)) return -1;
  return h->net.backward(params, dl_nchw, dl_nhwc, grads, ws, wsb, (hipStream_t)stream, stage_events);
}
int flair_unet_encoder_forward(flair_unet_t* h, const float* params, float* buffers, const float* x,
                               float* const feats[5], int B, int H, int W, int training, void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.encoder_forward(params, buffers, x, feats, B, H, W, training, ws, wsb, (hipStream_t)stream);
}
int flair_unet_decoder_forward(flair_unet_t* h, const float* params, float* buffers, const float* const feats[5],
                               float* out, int B, int H, int W, int training, void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.decoder_forward(params, buffers, feats, out, B, H, W, training, ws, wsb, (hipStream_t)stream);
}
int flair_unet_head_forward(flair_unet_t* h, const float* params, const float* x, float* logits, int B, int H, int W,
                            int training, void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.head_forward(params, x, logits, B, H, W, training, ws, wsb, (hipStream_t)stream);
}
int flair_unet_head_backward(flair_unet_t* h, const float* params, const float* dl, float* dx, float* grads, void* ws,
                             size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.head_backward(params, dl, dx, grads, ws, wsb, (hipStream_t)stream);
}
int flair_unet_decoder_backward(flair_unet_t* h, const float* params, const float* dout, float* const dfeats[5],
                                float* grads, void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.decoder_backward(params, dout, dfeats, grads, ws, wsb, (hipStream_t)stream);
}
int flair_unet_encoder_backward(flair_unet_t* h, const float* params, const float* const dfeats[5], float* grads,
                                void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.encoder_backward(params, dfeats, grads, ws, wsb, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ head
size_t flair_ce_workspace_bytes(int B, int H, int W) { return ce_workspace_floats(B, H, W) * sizeof(float); }

int flair_ce_head(const float* logits, const void* labels, int label_kind, const float* weight, int B, int C, int H,
                  int W, float* loss, float* dl_nchw, void* dl_nhwc, int dl_dtype, int dl_ld, uint8_t* preds_u8,
                  int64_t* preds_i64, int32_t* targets_i32, int64_t* confmat, void* workspace, void* stream) {
  if (!logits || !labels || !loss || !workspace || label_kind < 0 || label_kind > 3) return -1;
  CeArgs a;
  a.logits = logits; a.labels = labels; a.label_kind = label_kind; a.weight = weight;
  a.B = B; a.C = C; a.H = H; a.W = W; a.loss = loss; a.dlogits_nchw = dl_nchw; a.dlogits_nhwc = dl_nhwc;
  a.dlogits_dtype = dl_dtype; a.dlogits_ld = dl_ld; a.preds_u8 = preds_u8; a.preds_i64 = (long long*)preds_i64;
  a.targets_i32 = targets_i32; a.confmat = (long long*)confmat; a.workspace = (float*)workspace;
  return ce_head(a, (hipStream_t)stream);
}
const void* flair_unet_logits_nhwc(const flair_unet_t* h) { return h ? h->net.logits_nhwc() : nullptr; }

int flair_ce_head_nhwc(const void* logits_nhwc, int dtype, int ld, const void* labels, int label_kind, const float* weight,
                       int B, int C, int H, int W, float* loss, void* dl_nhwc, uint8_t* preds_u8, int32_t* targets_i32,
                       int64_t* confmat, void* workspace, void* stream) {
  if (!logits_nhwc || !labels || !loss || !workspace || label_kind < 0 || label_kind > 3) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  CeArgs a;
  a.logits = nullptr; a.logits_nhwc = logits_nhwc; a.logits_dtype = dtype; a.logits_ld = ld;
  a.labels = labels; a.label_kind = label_kind; a.weight = weight;
  a.B = B; a.C = C; a.H = H; a.W = W; a.loss = loss; a.dlogits_nchw = nullptr; a.dlogits_nhwc = dl_nhwc;
  a.dlogits_dtype = dtype; a.dlogits_ld = ld; a.preds_u8 = preds_u8; a.preds_i64 = nullptr;
  a.targets_i32 = targets_i32; a.confmat = (long long*)confmat; a.workspace = (float*)workspace;
  return ce_head(a, (hipStream_t)stream);
}
size_t flair_seg_loss_workspace_bytes(int B, int C, int H, int W) { return seg_loss_workspace_bytes(B, C, H, W); }

static void seg_loss_common(SegLossArgs& a, const void* labels, int label_kind, const float* weight, int B, int C, int H, int W,
                            const flair_seg_loss_t* spec, float* loss3, void* dl, uint8_t* preds_u8, int32_t* targets_i32, int64_t* confmat,
                            void* workspace) {
  a.labels = labels; a.label_kind = label_kind; a.weight = weight; a.B = B; a.C = C; a.H = H; a.W = W;
  a.spec = SegLossSpec{spec->ce, spec->label_smoothing, spec->focal_gamma, spec->dice, spec->dice_smooth, spec->dice_eps};
  a.loss3 = loss3; a.dl = dl; a.preds_u8 = preds_u8; a.targets_i32 = targets_i32; a.confmat = (long long*)confmat;
  a.workspace = (float*)workspace;
}
int flair_seg_loss(const float* logits, const void* labels, int label_kind, const float* weight, int B, int C, int H, int W,
                   const flair_seg_loss_t* spec, float* loss3, float* dl_nchw, uint8_t* preds_u8, int64_t* preds_i64,
                   int32_t* targets_i32, int64_t* confmat, void* workspace, void* stream) {
  if (!logits || !labels || !spec || !loss3 || !workspace || label_kind < 0 || label_kind > 3) return -1;
  SegLossArgs a;
  seg_loss_common(a, labels, label_kind, weight, B, C, H, W, spec, loss3, dl_nchw, preds_u8, targets_i32, confmat, workspace);
  a.logits = logits; a.preds_i64 = (long long*)preds_i64;
  return seg_loss(a, (hipStream_t)stream);
}
int flair_seg_loss_nhwc(const void* logits_nhwc, int dtype, int ld, const void* labels, int label_kind, const float* weight, int B,
                        int C, int H, int W, const flair_seg_loss_t* spec, float* loss3, void* dl_nhwc, uint8_t* preds_u8,
                        int32_t* targets_i32, int64_t* confmat, void* workspace, void* stream) {
  if (!logits_nhwc || !labels || !spec || !loss3 || !workspace || label_kind < 0 || label_kind > 3) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  SegLossArgs a;
  seg_loss_common(a, labels, label_kind, weight, B, C, H, W, spec, loss3, dl_nhwc, preds_u8, targets_i32, confmat, workspace);
  a.logits_nhwc = logits_nhwc; a.dtype = dtype; a.ld = ld;
  return seg_loss(a, (hipStream_t)stream);
}
int flair_softmax_argmax_nhwc(const void* logits_nhwc, int dtype, int ld, int B, int C, int H, int W, uint8_t* preds_u8,
                              int64_t* preds_i64, float* maxprob, void* stream) {
  if (!logits_nhwc) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return softmax_argmax_nhwc(logits_nhwc, dtype, ld, (long)B * H * W, C, preds_u8, (long long*)preds_i64, maxprob, (hipStream_t)stream);
}
int flair_softmax_argmax(const float* logits, int B, int C, int H, int W, uint8_t* preds_u8, int64_t* preds_i64,
                         float* maxprob, void* stream) {
  if (!logits) return -1;
  return softmax_argmax(logits, B, C, H, W, preds_u8, (long long*)preds_i64, maxprob, (hipStream_t)stream);
}
int flair_confmat_update(const void* target, int tk, const void* pred, int pk, int64_t n, int C, int64_t* confmat, void* stream) {
  if (!target || !pred || !confmat) return -1;
  return confmat_update(target, tk, pred, pk, n, C, (long long*)confmat, (hipStream_t)stream);
}
int flair_jaccard(const int64_t* confmat, int C, float* per_class, float* weighted, float* macro, void* stream) {
  if (!confmat) return -1;
  return jaccard_from_confmat((const long long*)confmat, C, per_class, weighted, macro, (hipStream_t)stream);
}
int flair_feed_tiles(const uint8_t* img_u8, const uint8_t* msk_raw, const uint8_t* d4_flags, int B, int bands, int H, int W,
                     const int* channels, int n_channels, int norm_type, const double* means, const double* stds,
                     int num_classes, float* img_out, uint8_t* labels_out, void* stream) {
  FeedArgs a{};
  const int rc = feed_args(a, img_u8 != nullptr, d4_flags, B, bands, H, W, channels, n_channels, norm_type, means, stds, num_classes,
                           img_out, labels_out);
  if (rc) return rc;
  a.img = img_u8; a.msk = msk_raw;
  return feed_tiles(a, (hipStream_t)stream);
}
int flair_feed_tiles_ptrs(const uint64_t* img_ptrs, const uint64_t* msk_ptrs, const uint8_t* d4_flags, int B, int bands, int H, int W,
                          const int* channels, int n_channels, int norm_type, const double* means, const double* stds,
                          int num_classes, float* img_out, uint8_t* labels_out, void* stream) {
  FeedArgs a{};
  const int rc = feed_args(a, img_ptrs != nullptr, d4_flags, B, bands, H, W, channels, n_channels, norm_type, means, stds, num_classes,
                           img_out, labels_out);
  if (rc) return rc;
  return feed_tiles_ptrs(a, (const unsigned long long*)img_ptrs, (const unsigned long long*)msk_ptrs, (hipStream_t)stream);
}
int flair_detect_convert(const float* logits_nchw, int B, int C, int S, int margin, int output_type, void* out, void* stream) {
  if (!logits_nchw || !out) return -1;
  return detect_convert(logits_nchw, 1, B, C, S, margin, output_type, out, nullptr, 0, 0, (hipStream_t)stream);
}
int flair_detect_convert_q4(const float* logits_nchw, int B, int C, int S, int margin, int output_type, void* out, void* stream) {
  if (!logits_nchw || !out) return -1;
  return detect_convert(logits_nchw, 4, B, C, S, margin, output_type, out, nullptr, 0, 0, (hipStream_t)stream);
}
int flair_detect_stitch(const float* logits_nchw, int B, int C, int S, int margin, int output_type, const int32_t* tiles,
                        void* raster_out, int raster_h, int raster_w, void* stream) {
  if (!logits_nchw || !raster_out || !tiles) return -1;
  return detect_convert(logits_nchw, 1, B, C, S, margin, output_type, raster_out, tiles, raster_h, raster_w, (hipStream_t)stream);
}
int flair_detect_stitch_q4(const float* logits_nchw, int B, int C, int S, int margin, int output_type, const int32_t* tiles,
                           void* raster_out, int raster_h, int raster_w, void* stream) {
  if (!logits_nchw || !raster_out || !tiles) return -1;
  return detect_convert(logits_nchw, 4, B, C, S, margin, output_type, raster_out, tiles, raster_h, raster_w, (hipStream_t)stream);
}
int flair_detect_stitch_preds(const uint8_t* preds_u8, const float* maxprob_f32, int B, int S, int margin, const int32_t* tiles,
                              float* raster_out, int raster_h, int raster_w, void* stream) {
  if (!preds_u8 || !maxprob_f32 || !raster_out || !tiles) return -1;
  return detect_stitch_preds(preds_u8, maxprob_f32, B, S, margin, tiles, raster_out, raster_h, raster_w, (hipStream_t)stream);
}
int flair_detect_blend_accum(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, const float* cheb_weights,
                             int x_lo, int x_hi, int y_lo, int y_hi, float* ring, int raster_h, int raster_w, void* stream) {
  if (!logits_nchw || !tiles || !ring) return -1;
  return detect_blend_accum(logits_nchw, 1, B, C, S, margin, tiles, cheb_weights, x_lo, x_hi, y_lo, y_hi, ring, raster_h, raster_w,
                            (hipStream_t)stream);
}
int flair_detect_blend_accum_q4(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, const float* cheb_weights,
                                int x_lo, int x_hi, int y_lo, int y_hi, float* ring, int raster_h, int raster_w, void* stream) {
  if (!logits_nchw || !tiles || !ring) return -1;
  return detect_blend_accum(logits_nchw, 4, B, C, S, margin, tiles, cheb_weights, x_lo, x_hi, y_lo, y_hi, ring, raster_h, raster_w,
                            (hipStream_t)stream);
}
int flair_detect_blend_flush(float* ring, int C, int ring_cols, int x_lo, int x_hi, float* raster_out, int raster_h, int raster_w,
                             void* stream) {
  if (!ring || !raster_out) return -1;
  return detect_blend_flush(ring, C, ring_cols, x_lo, x_hi, raster_out, raster_h, raster_w, (hipStream_t)stream);
}
int flair_detect_stitch_max(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, int x_lo, int x_hi,
                            int y_lo, int y_hi, float* raster_out, int raster_h, int raster_w, void* stream) {
  if (!logits_nchw || !tiles || !raster_out) return -1;
  return detect_stitch_max(logits_nchw, 1, nullptr, nullptr, B, C, S, margin, tiles, x_lo, x_hi, y_lo, y_hi, raster_out, raster_h,
                           raster_w, (hipStream_t)stream);
}
int flair_detect_stitch_max_q4(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, int x_lo, int x_hi,
                               int y_lo, int y_hi, float* raster_out, int raster_h, int raster_w, void* stream) {
  if (!logits_nchw || !tiles || !raster_out) return -1;
  return detect_stitch_max(logits_nchw, 4, nullptr, nullptr, B, C, S, margin, tiles, x_lo, x_hi, y_lo, y_hi, raster_out, raster_h,
                           raster_w, (hipStream_t)stream);
}
int flair_detect_stitch_max_preds(const uint8_t* preds_u8, const float* maxprob_f32, int B, int S, int margin, const int32_t* tiles,
                                  int x_lo, int x_hi, int y_lo, int y_hi, float* raster_out, int raster_h, int raster_w, void* stream) {
  if (!preds_u8 || !maxprob_f32 || !tiles || !raster_out) return -1;
  return detect_stitch_max(nullptr, 1, preds_u8, maxprob_f32, B, 0, S, margin, tiles, x_lo, x_hi, y_lo, y_hi, raster_out, raster_h,
                           raster_w, (hipStream_t)stream);
}
int flair_zone_window_confmat_preds(const uint8_t* preds_u8, int B, int C, int S, int margin, const int32_t* tiles,
                                    const uint8_t* truth_u8, int raster_h, int raster_w, int64_t* confmats, void* stream) {
  if (!preds_u8 || !tiles || !truth_u8 || !confmats) return -1;
  return zone_window_confmat(0, preds_u8, B, C, S, margin, tiles, truth_u8, raster_h, raster_w, (long long*)confmats, (hipStream_t)stream);
}
int flair_zone_window_confmat_logits(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles,
                                     const uint8_t* truth_u8, int raster_h, int raster_w, int64_t* confmats, void* stream) {
  if (!logits_nchw || !tiles || !truth_u8 || !confmats) return -1;
  return zone_window_confmat(1, logits_nchw, B, C, S, margin, tiles, truth_u8, raster_h, raster_w, (long long*)confmats,
                             (hipStream_t)stream);
}
int flair_zone_window_confmat_logits_q4(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles,
                                        const uint8_t* truth_u8, int raster_h, int raster_w, int64_t* confmats, void* stream) {
  if (!logits_nchw || !tiles || !truth_u8 || !confmats) return -1;
  return zone_window_confmat(3, logits_nchw, B, C, S, margin, tiles, truth_u8, raster_h, raster_w, (long long*)confmats,
                             (hipStream_t)stream);
}
int flair_zone_window_confmat_raster(const float* raster, int B, int C, int S, int margin, const int32_t* tiles, const uint8_t* truth_u8,
                                     int raster_h, int raster_w, int64_t* confmats, void* stream) {
  if (!raster || !tiles || !truth_u8 || !confmats) return -1;
  return zone_window_confmat(2, raster, B, C, S, margin, tiles, truth_u8, raster_h, raster_w, (long long*)confmats, (hipStream_t)stream);
}
int flair_zone_raster_confmat(const float* raster, const uint8_t* truth_u8, int raster_h, int raster_w, int C, int64_t* confmat,
                              void* stream) {
  if (!raster || !truth_u8 || !confmat) return -1;
  return zone_raster_confmat(raster, truth_u8, raster_h, raster_w, C, (long long*)confmat, (hipStream_t)stream);
}
int flair_zone_error_map(const float* raster, const uint8_t* truth_u8, int raster_h, int raster_w, int K, const int32_t* row_origins,
                         int n_rows, const int32_t* col_origins, int n_cols, double sigma, int radius, uint8_t* mask_ws,
                         int32_t* colsum_ws, int32_t* counts_ws, double* tmp_ws, double* error_map, void* stream) {
  if (!raster || !truth_u8 || !row_origins || !col_origins || !mask_ws || !colsum_ws || !counts_ws || !tmp_ws || !error_map) return -1;
  return zone_error_map(raster, truth_u8, raster_h, raster_w, K, row_origins, n_rows, col_origins, n_cols, sigma, radius, mask_ws,
                        colsum_ws, counts_ws, tmp_ws, error_map, (hipStream_t)stream);
}
int flair_gather_tiles(const uint8_t* raster_u8, int bands, int raster_h, int raster_w, const int32_t* tiles, int B, int S,
                       const int* channels, int n_channels, int norm_type, const double* means, const double* stds,
                       float* img_out, void* stream) {
  if (!raster_u8 || !tiles || !channels || !img_out) return -1;
  if (n_channels < 1 || n_channels > FeedArgs::MAXCH) return -2;
  if (norm_type == 2 && (!means || !stds)) return -1;
  FeedArgs a{};
  a.img = raster_u8; a.out = img_out; a.B = B; a.Cb = bands; a.Cout = n_channels; a.H = S; a.W = S; a.mode = norm_type;
  for (int c = 0; c < n_channels; ++c) {
    a.band[c] = channels[c] - 1;
    a.mean[c] = norm_type == 2 ? means[c] : 0.0;
    a.stdv[c] = norm_type == 2 ? stds[c] : 1.0;
  }
  return gather_tiles(a, tiles, raster_h, raster_w, (hipStream_t)stream);
}
int flair_d4_nchw_f32(const float* in_nchw, float* out_nchw, int B, int C, int H, int W, int code, void* stream) {
  if (!in_nchw || !out_nchw || in_nchw == out_nchw) return -1;
  return d4_nchw_f32(in_nchw, out_nchw, B, C, H, W, code, (hipStream_t)stream);
}
int flair_tta_accum(const float* logits_nchw, int B, int C, int H, int W, int code, int first, float* acc_nchw, uint8_t* preds_u8,
                    float* prob_f32, int n, void* stream) {
  if (!logits_nchw) return -1;
  return tta_accum(logits_nchw, 1, B, C, H, W, code, first, acc_nchw, preds_u8, prob_f32, n, (hipStream_t)stream);
}
int flair_tta_accum_q4(const float* logits_nchw, int B, int C, int H, int W, int code, int first, float* acc_nchw, uint8_t* preds_u8,
                       float* prob_f32, int n, void* stream) {
  if (!logits_nchw) return -1;
  return tta_accum(logits_nchw, 4, B, C, H, W, code, first, acc_nchw, preds_u8, prob_f32, n, (hipStream_t)stream);
}
int flair_confmat_masks(const uint8_t* truth_raw, const uint8_t* pred, int64_t n, int C, int truth_offset, int64_t* confmat,
                        void* stream) {
  if (!truth_raw || !pred || !confmat) return -1;
  return confmat_masks(truth_raw, pred, n, C, truth_offset, (long long*)confmat, (hipStream_t)stream);
}
int flair_sgd_step(float* params, const float* grads, int64_t n, float lr, void* stream) {
  if (!params || !grads) return -1;
  return sgd_step(params, grads, n, lr, (hipStream_t)stream);
}
int flair_optim_sgd(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                    float weight_decay, int nesterov, int first, float grad_scale, const float* coef, void* stream) {
  return optim_sgd(params, grads, momentum_buf, n, lr, momentum, dampening, weight_decay, nesterov, first, grad_scale, coef,
                   (hipStream_t)stream);
}
int flair_optim_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float bc1, float bc2, int first, float grad_scale, const float* coef, void* stream) {
  return optim_adamw(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, first, grad_scale, coef,
                     (hipStream_t)stream);
}
int flair_grad_sqnorm_partials(void) { return grad_sqnorm_partials(); }
int flair_grad_sqnorm(const float* grads, int64_t n, double* partials, double* sum, int accumulate, void* stream) {
  return grad_sqnorm(grads, n, partials, sum, accumulate, (hipStream_t)stream);
}
int flair_clip_coef(const double* sum, float grad_scale, float max_norm, float* norm, float* coef, void* stream) {
  return clip_coef(sum, grad_scale, max_norm, norm, coef, (hipStream_t)stream);
}
int flair_add_rowvec_nchw(float* x, const float* v, int N, int C, int H, int W, void* stream) {
  if (!x || !v) return -1;
  return add_rowvec_nchw(x, v, N, C, H, W, (hipStream_t)stream);
}
int flair_add_rowvec_nhwc(int dtype, void* x, const float* v, int N, int H, int W, int C, void* stream) {
  if (!x || !v) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return add_rowvec_nhwc(dtype, x, v, N, H, W, C, (hipStream_t)stream);
}
int flair_add_rowvec_nhwc_to(int dtype, const void* x, const float* v, void* y, int N, int H, int W, int C, void* stream) {
  if (!x || !v || !y) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return add_rowvec_nhwc_to(dtype, x, v, y, N, H, W, C, (hipStream_t)stream);
}
int flair_rowvec_grad_nhwc(int dtype, const void* dx, float* dv, int N, int H, int W, int C, void* stream) {
  if (!dx || !dv) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return rowvec_grad_nhwc(dtype, dx, dv, N, H, W, C, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ operators

size_t flair_conv2d_workspace_bytes(int dtype, int N, int H, int W, int C0, int C1, int up0, int Cout, int R, int stride,
                                    int pad) {
  const size_t es = dtype_size(dtype);
  const ConvInput in{nullptr, nullptr, C0, C1, up0, N, H, W};
  ConvArgs a;
  conv_fwd_args(a, dtype, in, R, stride, pad, Cout);
  size_t b = (size_t)conv_weight_rows_pad(Cout) * a.Kpad * es + 4096;
  b += ((size_t)N * a.Hout * a.Wout / 128 + 2) * 2 * Cout * 4 + 4096;            // stats partial
  const int CoutP = (int)round_up(Cout, 8);
  b += (size_t)conv_weight_rows_pad(C0 + C1) * conv_kpad(dtype, R * R * CoutP) * es + 4096;  // dgrad pack
  WgradArgs w;
  wgrad_args(w, in, R, stride, pad, nullptr, CoutP, Cout, nullptr, 0);
  b += wgrad_workspace_bytes(dtype, w) + 4096;
  return b;
}

// the plain forward is the fused form with every option off: one code path, the same arena layout and launches
int flair_conv2d_forward(int dtype, const void* x0, const void* x1, int N, int H, int W, int C0, int C1, int up0,
                         const float* w_oihw, const float* bias, int Cout, int R, int stride, int pad, void* y_nhwc,
                         float* y_nchw, float* stats, void* workspace, size_t wsb, void* stream) {
  flair_conv_ex_t p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype; p.x0 = x0; p.x1 = x1; p.N = N; p.H = H; p.W = W; p.C0 = C0; p.C1 = C1; p.up0 = up0;
  p.w_oihw = w_oihw; p.bias = bias; p.Cout = Cout; p.R = R; p.stride = stride; p.pad = pad;
  p.y_nhwc = y_nhwc; p.y_nchw = y_nchw; p.stats = stats;
  return flair_conv2d_ex(&p, workspace, wsb, stream);
}

int flair_conv2d_backward(int dtype, const void* x0, int N, int H, int W, int Cin, const float* w_oihw, int Cout, int R,
                          int stride, int pad, const void* dy, void* dx, float* dw, void* workspace, size_t wsb, void* stream) {
  if (!x0 || !w_oihw || !dy || !workspace) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int Ho = conv_out_extent(H, R, stride, pad), Wo = conv_out_extent(W, R, stride, pad);
  Arena ar(workspace, wsb);
  int rc = 0;
  if (dx) {
    ConvArgs a;
    conv_dgrad_args(a, dtype, ConvInput{dy, nullptr, Cout, 0, 0, N, Ho, Wo}, R, stride, pad, H, W, Cin);
    const int rows_d = conv_weight_rows_pad(Cin);
    void* wd = ar.get((size_t)rows_d * a.Kpad * dtype_size(dtype));
    if (ar.err) return ar.err;
    rc = pack_weight(dtype, w_oihw, wd, Cout, Cin, R, R, Cout, rows_d, a.Kpad, 1, s);
    if (rc) return rc;
    a.w = wd; a.out = dx; a.out_ld = Cin;
    rc = launch_conv(dtype, a, s);
    if (rc) return rc;
  }
  if (dw) {
    WgradArgs w;
    wgrad_args(w, ConvInput{x0, nullptr, Cin, 0, 0, N, H, W}, R, stride, pad, dy, Cout, Cout, dw, Cin);
    w.partial = (float*)ar.get(wgrad_workspace_bytes(dtype, w));
    if (ar.err) return ar.err;
    rc = launch_wgrad(dtype, w, s);
  }
  return rc;
}

// ---- the fused forms of the same launchers (plain structs in, ConvArgs / WgradArgs out; no kernel differs)
static int conv_ex_fill(const flair_conv_ex_t* p, ConvArgs& a) {
  if (p->dtype != DT_F32 && p->dtype != DT_BF16) return -2;
  if (p->mode != 0 && p->mode != 1 && p->mode != 2) return -2;
  if (p->mode == 1 && p->stride != 1) return -6;   // (mode 2 is the stride-2 data gradient)
  const ConvInput in{p->x0, p->x1, p->C0, p->x1 ? p->C1 : 0, p->up0, p->N, p->H, p->W};
  const int out_ld = p->out_ld > 0 ? p->out_ld : p->Cout;
  if (p->mode == 2) {
    // the network's stride-2 data gradient (UNet::unit_backward, DG_PARITY): x0 is dY, the output twice its extent
    const bool r3 = p->R == 3 && p->pad == 1, r1 = p->R == 1 && p->pad == 0;
    if (p->stride != 2 || (!r3 && !r1) || p->x1 || p->up0) return -6;
    // every other option of the struct belongs to kernels this form never reaches
    if (p->bias || p->y_nchw || p->stats || p->in_scale || p->in_shift || p->oscale || p->oshift || p->ores || p->orelu || p->acc_src ||
        p->pool_c0 || p->out_skip || p->preds_u8 || p->maxprob_f32 || p->ogelu || p->bnr_y || p->bnr_out || p->bnr_partial || p->bnr_mask)
      return -6;
    conv_dgrad_args(a, p->dtype, in, p->R, p->stride, p->pad, 2 * p->H, 2 * p->W, p->Cout);
    conv_parity_args(a, p->dtype, p->R);
    a.out = p->y_nhwc; a.out_ld = out_ld; a.accumulate = p->accumulate;
    return 0;
  }
  // mode 1: the data gradient of a stride-1 layer, to the extent of that layer's input
  if (p->mode == 1) {
    const int fp = p->R - 1 - p->pad, up = in.up0 ? 2 : 1;   // (the flipped padding gives that layer's input extent)
    conv_dgrad_args(a, p->dtype, in, p->R, 1, p->pad, conv_out_extent(up * in.H, p->R, 1, fp), conv_out_extent(up * in.W, p->R, 1, fp), p->Cout);
  } else {
    conv_fwd_args(a, p->dtype, in, p->R, p->stride, p->pad, p->Cout);
  }
  a.bias = p->bias; a.out = p->y_nhwc; a.out_ld = out_ld; a.out_nchw = p->y_nchw;
  a.in_scale = p->in_scale; a.in_shift = p->in_shift;
  a.oscale = p->oscale; a.oshift = p->oshift; a.ores = p->ores; a.orelu = p->orelu;
  a.accumulate = p->accumulate; a.acc_src = p->acc_src;
  a.pool_c0 = p->pool_c0; a.out_skip = p->out_skip; a.out_skip_ld = p->out_skip_ld; a.skip_accumulate = p->skip_accumulate;
  a.preds_u8 = p->preds_u8; a.maxprob_f32 = p->maxprob_f32; a.ogelu = p->ogelu;
  a.bnr_mask = p->bnr_mask;
  if (p->bnr_partial || p->bnr_y) {
    a.bnr_y = p->bnr_y; a.bnr_out = p->bnr_out; a.bnr_scale = p->bnr_scale; a.bnr_shift = p->bnr_shift; a.bnr_C = a.out_ld;
    a.bnr_partial = p->bnr_partial;
  }
  return 0;
}

// The sizing queries launch nothing, and the dispatch predicates they ask only look at which pointers are set: the weights stand
// in as the struct itself, and a request for the fused reduction whose partial is still to be sized (bnr_y without bnr_partial)
// as `standin`, host storage of the query.  Arguments prepared here never reach launch_conv.
static void conv_ex_sizing(const flair_conv_ex_t* p, ConvArgs& a, float* standin) {
  a.w = p;
  if (p->mode != 2 && p->bnr_y && !a.bnr_partial) a.bnr_partial = standin;
}

// the four class packs of mode 2 (R = 3), or its one transposed pack (R = 1): descriptors relative to the workspace base
static size_t conv_ex_parity_packs(const flair_conv_ex_t* p, ConvArgs& a, unsigned char* base, PackTable& tb) {
  const size_t es = dtype_size(p->dtype);
  const int rows_d = conv_weight_rows_pad(p->Cout);
  const PackDesc d = pack_desc(0, 0, p->C0, p->Cout, p->R, p->C0, rows_d, a.Kpad, 1);
  tb.n = 0;
  size_t top = 0;
  if (!a.ncls) {
    tb.d[tb.n++] = d;
    a.w = base;
    return Arena::rounded((size_t)rows_d * a.Kpad * es);
  }
  for (int cls = 0; cls < 4; ++cls) {
    tb.d[tb.n++] = parity_class_pack(d, cls, top, a.cls_kpad[cls]);
    a.cls_w[cls] = base + top;
    top += Arena::rounded((size_t)rows_d * a.cls_kpad[cls] * es);
  }
  a.w = a.cls_w[3];
  return top;
}

size_t flair_conv2d_ex_workspace_bytes(const flair_conv_ex_t* p) {
  ConvArgs a;
  float standin;
  if (!p || conv_ex_fill(p, a)) return 0;
  conv_ex_sizing(p, a, &standin);
  if (p->mode == 2) {
    PackTable tb;
    return conv_ex_parity_packs(p, a, nullptr, tb) + 256;
  }
  a.stats = p->stats;
  size_t b = Arena::rounded((size_t)conv_weight_rows_pad(p->Cout) * a.Kpad * dtype_size(p->dtype));
  if (p->stats) b += Arena::rounded((size_t)conv_grid_rows(p->dtype, a) * 2 * p->Cout * 4);
  return b + 256;
}

int flair_conv2d_ex_grid_rows(const flair_conv_ex_t* p) {
  ConvArgs a;
  float standin;
  if (!p) return -1;
  const int rc = conv_ex_fill(p, a);
  if (rc) return rc;
  conv_ex_sizing(p, a, &standin);
  a.stats = p->stats;
  return conv_grid_rows(p->dtype, a);
}

int flair_conv2d_ex(const flair_conv_ex_t* p, void* workspace, size_t wsb, void* stream) {
  if (!p || !p->x0 || !p->w_oihw || !workspace) return -1;
  hipStream_t s = (hipStream_t)stream;
  ConvArgs a;
  int rc = conv_ex_fill(p, a);
  if (rc) return rc;
  if (p->mode == 2) {
    if (!p->y_nhwc) return -1;
    PackTable tb;
    if (conv_ex_parity_packs(p, a, (unsigned char*)workspace, tb) > wsb) return -100;
    rc = pack_weights_all(p->dtype, p->w_oihw, workspace, tb, s);
    return rc ? rc : launch_conv(p->dtype, a, s);
  }
  // the epilogue reads bnr_y, bnr_scale and bnr_shift unconditionally, and a reduction without a partial has nowhere to go
  if (p->bnr_partial ? (!p->bnr_y || !p->bnr_scale || !p->bnr_shift) : (p->bnr_y != nullptr)) return -1;
  Arena ar(workspace, wsb);
  const int Cin = a.C0 + a.C1, rows_f = conv_weight_rows_pad(p->Cout);
  void* wp = ar.get((size_t)rows_f * a.Kpad * dtype_size(p->dtype));
  a.w = wp;
  // the partial is the caller's, one row per row block of the launch
  if (p->bnr_partial && p->bnr_rows < conv_grid_rows(p->dtype, a)) return -100;
  float* partial = nullptr;
  int nblk = 0;
  if (p->stats) {
    a.stats = p->stats;   // (so that the row count is that of the kernel launch_conv picks with statistics on)
    nblk = conv_grid_rows(p->dtype, a);
    partial = (float*)ar.get((size_t)nblk * 2 * p->Cout * 4);
    a.stats = partial;
  }
  if (ar.err) return ar.err;
  // mode 1: w_oihw is the forward layer's [C0][Cout][R][R]; the data gradient multiplies by its transposed, flipped pack
  rc = p->mode == 1 ? pack_weight(p->dtype, p->w_oihw, wp, Cin, p->Cout, p->R, p->R, Cin, rows_f, a.Kpad, 1, s)
                    : pack_weight(p->dtype, p->w_oihw, wp, p->Cout, Cin, p->R, p->R, Cin, rows_f, a.Kpad, 0, s);
  if (rc) return rc;
  rc = launch_conv(p->dtype, a, s);
  if (rc) return rc;
  if (p->stats) rc = partial_rows_sum(partial, nblk, 2 * p->Cout, p->stats, s);
  return rc;
}

static int wgrad_ex_fill(const flair_wgrad_ex_t* p, WgradArgs& w) {
  if (p->dtype != DT_F32 && p->dtype != DT_BF16) return -2;
  const ConvInput in{p->x0, p->x1, p->C0, p->x1 ? p->C1 : 0, p->up0, p->N, p->H, p->W};
  wgrad_args(w, in, p->R, p->stride, p->pad, p->dy, p->dy_ld > 0 ? p->dy_ld : p->Cout, p->Cout, p->dw,
             p->Cin_real > 0 ? p->Cin_real : in.C0 + in.C1);
  w.accumulate = p->accumulate; w.in_scale = p->in_scale; w.in_shift = p->in_shift; w.cus = p->cus; w.dbias = p->dbias;
  w.fuse_y = p->fuse_y; w.fuse_coef = p->fuse_coef; w.fuse_msc = p->fuse_msc; w.fuse_msh = p->fuse_msh;
  return 0;
}

size_t flair_conv2d_wgrad_ex_workspace_bytes(const flair_wgrad_ex_t* p) {
  WgradArgs w;
  if (!p || wgrad_ex_fill(p, w)) return 0;
  size_t b = Arena::rounded(wgrad_workspace_bytes(p->dtype, w));
  if (p->dbias && wgrad_dbias_fusable(p->dtype, w)) b += Arena::rounded((size_t)WGRAD_DBIAS_ROWS * w.dy_ld * 4);
  return b + 256;
}

int flair_conv2d_wgrad_ex(const flair_wgrad_ex_t* p, void* workspace, size_t wsb, void* stream) {
  if (!p || !p->x0 || !p->dy || !p->dw || !workspace) return -1;
  WgradArgs w;
  int rc = wgrad_ex_fill(p, w);
  if (rc) return rc;
  Arena ar(workspace, wsb);
  w.partial = (float*)ar.get(wgrad_workspace_bytes(p->dtype, w));
  if (p->dbias && wgrad_dbias_fusable(p->dtype, w)) w.dbias_partial = (float*)ar.get((size_t)WGRAD_DBIAS_ROWS * w.dy_ld * 4);
  if (ar.err) return ar.err;
  return launch_wgrad(p->dtype, w, (hipStream_t)stream);
}

// partial block sums + the per-channel coefficient rows of either direction (what the two calls below carve out of `workspace`)
size_t flair_bn_workspace_bytes(int64_t rows, int C) {
  if (rows < 1 || C < 1) return 0;
  const size_t partial = Arena::rounded((size_t)bn_bwd_blocks(rows) * 2 * C * 4);
  const size_t fwd = 2 * Arena::rounded((size_t)C * 4) + partial + Arena::rounded((size_t)2 * C * 4);
  const size_t bwd = partial + Arena::rounded((size_t)3 * C * 4);
  return (fwd > bwd ? fwd : bwd) + 256;
}

int flair_bn_relu_forward(int dtype, const void* y, int64_t rows, int C, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int training, const void* residual, int relu,
                          void* out, float* save_mean, float* save_invstd, void* workspace, size_t wsb, void* stream) {
  if (!y || !out || !workspace) return -1;
  hipStream_t s = (hipStream_t)stream;
  Arena ar(workspace, wsb);
  float* scale = (float*)ar.get(C * 4);
  float* shift = (float*)ar.get(C * 4);
  int rc;
  if (training) {
    const int nblk = bn_bwd_blocks(rows);
    float* partial = (float*)ar.get((size_t)nblk * 2 * C * 4);
    float* zo = (float*)ar.get(2 * C * 4);
    if (ar.err) return ar.err;
    rc = bn_stats_partial(dtype, y, rows, C, partial, zo, s);
    if (rc) return rc;
    rc = bn_finalize(partial, nblk, C, rows, gamma, beta, running_mean, running_var, 0.1f, 1e-5f, scale, shift,
                     save_mean, save_invstd, s);
  } else {
    if (ar.err) return ar.err;
    rc = bn_eval_coeffs(C, gamma, beta, running_mean, running_var, 1e-5f, scale, shift, s);
  }
  if (rc) return rc;
  return bn_act(dtype, y, scale, shift, residual, nullptr, nullptr, out, rows, C, relu, s);
}

int flair_bn_relu_backward(int dtype, const void* dout, const void* out, const void* y, int64_t rows, int C,
                           const float* gamma, const float* save_mean, const float* save_invstd, int relu, void* dy,
                           void* dres, float* dgamma, float* dbeta, void* workspace, size_t wsb, void* stream) {
  if (!dout || !y || !dy || !workspace) return -1;
  Arena ar(workspace, wsb);
  float* partial = (float*)ar.get((size_t)bn_bwd_blocks(rows) * 2 * C * 4);
  float* coef = (float*)ar.get(3 * C * 4);
  if (ar.err) return ar.err;
  return bn_backward(dtype, dout, relu ? out : nullptr, y, save_mean, save_invstd, gamma, rows, C, partial, coef, dgamma,
                     dbeta, 0, dy, dres, 0, nullptr, nullptr, 0, 0, (hipStream_t)stream);
}

int flair_bn_backward_ex(const flair_bn_bwd_ex_t* p, void* workspace, size_t wsb, void* stream) {
  if (!p || !p->dout || !p->y || !p->mean || !p->invstd || !workspace || p->rows < 1 || p->C < 1) return -1;
  if (p->dtype != DT_F32 && p->dtype != DT_BF16) return -2;
  if (p->dres && !p->dy) return -1;              // the apply pass always writes dy
  if (!p->dgamma != !p->dbeta) return -1;
  if (p->pre_nblk > 0 && !p->partial) return -1;
  Arena ar(workspace, wsb);
  float* partial = p->pre_nblk > 0 ? p->partial : (float*)ar.get((size_t)bn_bwd_blocks(p->rows) * 2 * p->C * 4);
  float* coef = p->coef ? p->coef : (float*)ar.get(3 * (size_t)p->C * 4);
  if (ar.err) return ar.err;
  return bn_backward(p->dtype, p->dout, p->out, p->y, p->mean, p->invstd, p->gamma, (long)p->rows, p->C, partial, coef, p->dgamma,
                     p->dbeta, p->accumulate_param, p->dy, p->dres, p->dres_accumulate, p->mscale, p->mshift, p->pre_nblk,
                     p->premasked, (hipStream_t)stream);
}

static size_t bwd16_ex_pack_bytes() { return Arena::rounded((size_t)16 * conv_kpad(DT_BF16, 9 * 16) * 2); }

// the separate weight gradient of the same layer: its grid is the fused kernel's default
static void bwd16_ex_wgrad(const flair_bwd16_ex_t* p, WgradArgs& w) {
  wgrad_args(w, ConvInput{p->x, nullptr, 16, 0, 0, p->N, p->H, p->W}, 3, 1, 1, p->g, 16, p->Cout, p->dw, 16);
  w.in_scale = p->in_scale; w.in_shift = p->in_shift;
}

size_t flair_bwd16_ex_workspace_bytes(const flair_bwd16_ex_t* p) {
  if (!p || p->N < 1 || p->H < 1 || p->W < 1 || (p->H % 8) || (p->W % 32)) return 0;
  WgradArgs w;
  bwd16_ex_wgrad(p, w);
  return bwd16_ex_pack_bytes() + Arena::rounded(bwd16_workspace_bytes(bwd16_grid(w))) +
         Arena::rounded((size_t)WGRAD_DBIAS_ROWS * 16 * 4) + 256;
}

int flair_bwd16_ex_grid_rows(const flair_bwd16_ex_t* p) {
  if (!p || p->N < 1 || p->H < 1 || p->W < 1) return -1;
  if ((p->H % 8) || (p->W % 32)) return -2;
  WgradArgs w;
  bwd16_ex_wgrad(p, w);
  return bwd16_grid(w);
}

int flair_bwd16_ex(const flair_bwd16_ex_t* p, void* workspace, size_t wsb, void* stream) {
  if (!p || !p->g || !p->x || !p->in_scale || !p->in_shift || !p->w_oihw || !p->dx || !p->bnr_scale || !p->bnr_shift || !p->bnr_partial ||
      !p->dw || !workspace || p->N < 1 || p->H < 1 || p->W < 1)
    return -1;
  if (p->gy && (!p->gcoef || !p->gmsc || !p->gmsh || p->dbias)) return -1;
  if (p->Cout < 1 || p->Cout > 16 || (p->H % 8) || (p->W % 32)) return -2;
  hipStream_t s = (hipStream_t)stream;
  WgradArgs w;
  bwd16_ex_wgrad(p, w);
  const int grid = bwd16_grid(w);
  if (p->bnr_rows < grid) return -100;
  Arena ar(workspace, wsb);
  const int Kpad = conv_kpad(DT_BF16, 9 * 16);
  void* wp = ar.get((size_t)16 * Kpad * 2);
  Bwd16Args f;
  memset(&f, 0, sizeof(f));
  f.slabs = (float*)ar.get(bwd16_workspace_bytes(grid));
  f.grid = grid;
  if (p->dbias) f.dbias_partial = (float*)ar.get((size_t)WGRAD_DBIAS_ROWS * 16 * 4);
  if (ar.err) return ar.err;
  // the forward layer's [Cout][16][3][3] as the flipped / transposed data-gradient pack, 16 rows of 9 x 16 (padded) gradient channels
  const int rc = pack_weight(DT_BF16, p->w_oihw, wp, p->Cout, 16, 3, 3, 16, 16, Kpad, 1, s);
  if (rc) return rc;
  f.g = p->g; f.gy = p->gy; f.gcoef = p->gcoef; f.gmsc = p->gmsc; f.gmsh = p->gmsh;
  f.x = p->x; f.in_scale = p->in_scale; f.in_shift = p->in_shift;
  f.w = wp; f.Kpad = Kpad; f.dx = p->dx;
  f.bnr_scale = p->bnr_scale; f.bnr_shift = p->bnr_shift; f.bnr_partial = p->bnr_partial; f.bnr_C = 16; f.bnr_cols = grid;
  f.dw = p->dw; f.Cout = p->Cout; f.Cin_real = 16; f.dbias = p->dbias;
  f.N = p->N; f.H = p->H; f.W = p->W;
  return launch_bwd16(f, s);
}

int flair_maxpool_backward_ex(int dtype, const void* dy, const uint8_t* idx, void* dx, int accumulate, int N, int H, int W, int C,
                              const void* bnr_y, const float* bnr_msc, const float* bnr_msh, float* bnr_partial, void* stream) {
  if (!dy || !idx || !dx || N < 1 || H < 1 || W < 1 || C < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return maxpool3x3s2_bwd(dtype, dy, idx, dx, accumulate, N, H, W, C, (hipStream_t)stream, bnr_y, bnr_msc, bnr_msh, bnr_partial);
}
int flair_bn_act(int dtype, const void* y, const float* scale, const float* shift, void* out, int64_t rows, int C, int relu, void* stream) {
  if (!y || !scale || !shift || !out || rows < 1 || C < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return bn_act(dtype, y, scale, shift, nullptr, nullptr, nullptr, out, (long)rows, C, relu, (hipStream_t)stream);
}
int flair_bn_act_maxpool(int dtype, const void* y, const float* scale, const float* shift, void* act, void* out, uint8_t* idx, int N,
                         int H, int W, int C, void* stream) {
  if (!y || !scale || !shift || !act || !out || N < 1 || H < 1 || W < 1 || C < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return bn_act_maxpool3x3s2(dtype, y, scale, shift, act, out, idx, N, H, W, C, (hipStream_t)stream);
}
int flair_upcat_bwd(int dtype, const void* dcat, void* dx0, int dx0_accumulate, void* dskip, int dskip_accumulate, int N, int H, int W,
                    int C0, int C1, void* stream) {
  if (!dcat || !dx0 || (C1 > 0 && !dskip) || N < 1 || H < 1 || W < 1 || C0 < 1 || C1 < 0) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return upcat_bwd(dtype, dcat, dx0, dx0_accumulate, dskip, dskip_accumulate, N, H, W, C0, C1, (hipStream_t)stream);
}
int flair_ew_add(int dtype, void* dst, const void* src, int64_t n, void* stream) {
  if (!dst || !src || n < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  return ew_add(dtype, dst, src, (long)n, (hipStream_t)stream);
}
int flair_colsum(int dtype, const void* x, int64_t rows, int ld, int C, float* out, void* workspace, size_t wsb, void* stream) {
  if (!x || !out || !workspace || rows < 1 || ld < 1 || C < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  Arena ar(workspace, wsb);
  float* partial = (float*)ar.get((size_t)bn_bwd_blocks((long)rows) * ld * 4);
  if (ar.err) return ar.err;
  return colsum(dtype, x, (long)rows, ld, C, partial, out, (hipStream_t)stream);
}
int flair_pack_weights(int dtype, const float* params, const flair_pack_desc_t* descs, int n, void* base, void* stream) {
  if (!params || !descs || !base) return -1;
  if ((dtype != DT_F32 && dtype != DT_BF16) || n < 1 || n > PackTable::MAX) return -2;
  PackTable tb;
  tb.n = n;
  for (int i = 0; i < n; ++i) {
    const flair_pack_desc_t& q = descs[i];
    // the kernel trusts its table: a pack must hold its own real region
    const int taps = q.Rc > 0 ? q.Rc * q.Sc : q.R * q.S;
    if (q.Cout < 1 || q.Cin < 1 || q.R < 1 || q.S < 1 || taps < 1 || (long)taps * q.Cin_p > q.Kpad || q.Cin_p < (q.tf ? q.Cout : q.Cin) ||
        q.rows_pad < (q.tf ? q.Cin : q.Cout) || q.w_off < 0)
      return -2;
    // the bf16 forward 3x3 branch and the transposed 32 x 32 branch of the kernel load the master 16 bytes at a time
    const bool vec = dtype == DT_BF16 && q.R * q.S == 9 &&
                     (q.tf ? ((q.Cin & 31) == 0 && (q.Cout & 31) == 0) : (q.Rc == 0 && (q.Cin & 3) == 0));
    if (vec && (((uintptr_t)params & 15) || (q.w_off & 3))) return -2;
    if (q.Rc > 0 && (q.r0 + (q.Rc - 1) * q.rstep >= q.R || q.s0 + (q.Sc - 1) * q.sstep >= q.S || q.r0 < 0 || q.s0 < 0 || q.rstep < 1 || q.sstep < 1))
      return -2;
    PackDesc& d = tb.d[i];
    memset(&d, 0, sizeof(d));
    d.w_off = (long)q.w_off; d.dst_off = (size_t)q.dst_off; d.Cout = q.Cout; d.Cin = q.Cin; d.R = q.R; d.S = q.S;
    d.Cin_p = q.Cin_p; d.rows_pad = q.rows_pad; d.Kpad = q.Kpad; d.tf = q.tf;
    d.r0 = (unsigned char)q.r0; d.rstep = (unsigned char)q.rstep; d.Rc = (unsigned char)q.Rc;
    d.s0 = (unsigned char)q.s0; d.sstep = (unsigned char)q.sstep; d.Sc = (unsigned char)q.Sc;
  }
  return pack_weights_all(dtype, params, base, tb, (hipStream_t)stream);
}
int flair_pack_weight(int dtype, const float* w_oihw, void* dst, int Cout, int Cin, int R, int S, int Cin_p, int rows_pad, int Kpad,
                      int tf, void* stream) {
  if (!w_oihw || !dst) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  // as in flair_pack_weights: the pack holds its own real region (the kernel writes rows_pad x Kpad elements and reads w inside it)
  if (Cout < 1 || Cin < 1 || R < 1 || S < 1 || (long)R * S * Cin_p > Kpad || Cin_p < (tf ? Cout : Cin) || rows_pad < (tf ? Cin : Cout))
    return -2;
  return pack_weight(dtype, w_oihw, dst, Cout, Cin, R, S, Cin_p, rows_pad, Kpad, tf ? 1 : 0, (hipStream_t)stream);
}

int flair_maxpool_forward(int dtype, const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, void* stream) {
  return maxpool3x3s2_fwd(dtype, x, y, idx, N, H, W, C, (hipStream_t)stream);
}
int flair_maxpool_backward(int dtype, const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C, void* stream) {
  return maxpool3x3s2_bwd(dtype, dy, idx, dx, 0, N, H, W, C, (hipStream_t)stream);
}
int flair_nchw_to_nhwc(int dtype, const float* x, void* y, int N, int C, int H, int W, int Cpad, void* stream) {
  return nchw_f32_to_nhwc(dtype, x, y, N, C, H, W, Cpad, (hipStream_t)stream);
}
int flair_nhwc_to_nchw(int dtype, const void* x, float* y, int N, int C, int H, int W, int Cpad, void* stream) {
  return nhwc_to_nchw_f32(dtype, x, y, N, C, H, W, Cpad, nullptr, (hipStream_t)stream);
}

// ---- the SegFormer / UperNet-Swin kernels one at a time: each forwards to the launcher the executors call
#define FLAIR_DT_OK(dt) ((dt) == DT_F32 || (dt) == DT_BF16)
int flair_sf_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int C, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || rows < 1 || C < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return sf_layernorm(dtype, x, gamma, beta, y, (long)rows, C, eps, (hipStream_t)stream);
}
int flair_sf_dwconv3x3_gelu(int dtype, const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, void* stream) {
  if (!x || !w || !bias || !y || B < 1 || H < 1 || W < 1 || C < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return sf_dwconv3x3_gelu(dtype, x, w, bias, y, B, H, W, C, (hipStream_t)stream);
}
int flair_sf_bilinear_nhwc(int dtype, const void* x, void* y, int B, int h, int w, int C, int H, int W, int ld, void* stream) {
  if (!x || !y || B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || C < 1 || ld < C) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return sf_bilinear_nhwc(dtype, x, y, B, h, w, C, H, W, ld, (hipStream_t)stream);
}
int flair_sf_bilinear_nchw_f32(const float* x, float* y, int64_t planes, int h, int w, int H, int W, void* stream) {
  if (!x || !y || planes < 1 || h < 1 || w < 1 || H < 1 || W < 1) return -1;
  return sf_bilinear_nchw_f32(x, y, (long)planes, h, w, H, W, (hipStream_t)stream);
}
int flair_sf_slice_cols(int dtype, const float* src, int ld, int col0, int ncols, int64_t rows, void* dst, void* stream) {
  if (!src || !dst || rows < 1 || col0 < 0 || ncols < 1 || col0 + ncols > ld) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return sf_slice_cols(dtype, src, ld, col0, ncols, (long)rows, dst, (hipStream_t)stream);
}
int flair_sf_fuse_bias(const float* wf, int D, const float* b3, const float* b2, const float* b1, const float* b0, const float* scale,
                       const float* shift, float* shift2, void* stream) {
  if (!wf || !b3 || !b2 || !b1 || !b0 || !scale || !shift || !shift2 || D < 1) return -1;
  return sf_fuse_bias(wf, D, b3, b2, b1, b0, scale, shift, shift2, (hipStream_t)stream);
}
int flair_sf_upsample_sum_bn_relu(int dtype, const void* g0, const void* g1, const void* g2, const void* g3, const float* scale,
                                  const float* shift2, void* z, int B, int H, int W, int D, void* stream) {
  if (!g0 || !g1 || !g2 || !g3 || !scale || !shift2 || !z || B < 1 || H < 1 || W < 1 || D < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return sf_upsample_sum_bn_relu(dtype, g0, g1, g2, g3, scale, shift2, z, B, H, W, D, (hipStream_t)stream);
}
int flair_sf_ffn_fused_ok(int dtype, int C, int H, int W) { return sf_ffn_fused_ok(dtype, C, H, W) ? 1 : 0; }
int flair_sf_ffn_dw_pack(const float* w, const float* b, float* out, int nch, void* stream) {
  if (!w || !b || !out || nch < 1) return -1;
  return sf_ffn_dw_pack(w, b, out, nch, (hipStream_t)stream);
}
int flair_sf_ffn_fused(const void* x, const float* ln_g, const float* ln_b, const void* w1, const float* b1, const float* dwp, const void* w2,
                       const float* b2, void* out, int B, int H, int W, int C, float eps, const float* ln2_g, const float* ln2_b, void* out_ln,
                       void* stream) {
  if (!x || !ln_g || !ln_b || !w1 || !b1 || !dwp || !w2 || !b2 || !out || B < 1) return -1;
  return sf_ffn_fused(x, ln_g, ln_b, w1, b1, dwp, w2, b2, out, B, H, W, C, eps, ln2_g, ln2_b, out_ln, (hipStream_t)stream);
}
int flair_sf_head_fused_ok(int dtype, int H, int W, int C0, int D, int labels) { return sf_head_fused_ok(dtype, H, W, C0, D, labels) ? 1 : 0; }
int flair_sf_head_wint(void* wint, void* stream) {
  if (!wint) return -1;
  return sf_head_wint(wint, (hipStream_t)stream);
}
int flair_sf_head_fused(const void* f0, const void* w0, const void* g1, const void* g2, const void* g3, const void* wint, const float* scale,
                        const float* shift2, const void* wc, const float* bc, float* out, int B, int H, int W, int D, int labels, void* stream) {
  if (!f0 || !w0 || !g1 || !g2 || !g3 || !wint || !scale || !shift2 || !wc || !out || B < 1 || labels < 1) return -1;
  return sf_head_fused(f0, w0, g1, g2, g3, wint, scale, shift2, wc, bc, out, B, H, W, D, labels, (hipStream_t)stream);
}
int flair_sf_attention(int dtype, const void* q, const void* k, const void* v, void* out, int B, int N, int Nk, int hidden, int kv_ld,
                       void* stream) {
  if (!q || !k || !v || !out || B < 1 || N < 1 || hidden < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return sf_attention(dtype, q, k, v, out, B, N, Nk, hidden, kv_ld, (hipStream_t)stream);
}
int flair_swin_window_attention(int dtype, const void* qkv, const float* qkv_bias, const float* table, void* out, int B, int H, int W, int C,
                                int heads, int shift, void* stream) {
  if (!qkv || !qkv_bias || !table || !out) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return swin_window_attention(dtype, qkv, qkv_bias, table, out, B, H, W, C, heads, shift, (hipStream_t)stream);
}
int flair_swin_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int C, int ld, float eps,
                         void* stream) {
  if (!x || !gamma || !beta || !y || rows < 1 || C < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return swin_layernorm(dtype, x, gamma, beta, y, (long)rows, C, ld, eps, (hipStream_t)stream);
}
int flair_swin_patch_merge_ln(int dtype, const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps,
                              void* stream) {
  if (!x || !gamma || !beta || !y || B < 1 || H < 2 || W < 2 || C < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return swin_patch_merge_ln(dtype, x, gamma, beta, y, B, H, W, C, eps, (hipStream_t)stream);
}
int flair_swin_adaptive_avgpool(int dtype, const void* x, int ld, void* y, int B, int h, int w, int C, int S, void* stream) {
  if (!x || !y || B < 1 || h < 1 || w < 1 || C < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return swin_adaptive_avgpool(dtype, x, ld, y, B, h, w, C, S, (hipStream_t)stream);
}
int flair_swin_bilinear_add(int dtype, const void* x, void* y, int B, int h, int w, int C, int H, int W, void* stream) {
  if (!x || !y || B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || C < 1) return -1;
  if (!FLAIR_DT_OK(dtype)) return -2;
  return swin_bilinear_add(dtype, x, y, B, h, w, C, H, W, (hipStream_t)stream);
}
#undef FLAIR_DT_OK

long flair_tiff_lzw_slot_bytes(int rows_per_strip, int W) { return tiff_lzw_slot_bytes(rows_per_strip, W); }
int flair_tiff_lzw_encode(const uint8_t* img, int B, int H, int W, int rows_per_strip, uint8_t* out, long slot_bytes, int32_t* counts,
                          void* stream) {
  return tiff_lzw_encode(img, B, H, W, rows_per_strip, out, slot_bytes, counts, (hipStream_t)stream);
}
long flair_tiff_lzw_tile_slot_bytes(int tile, int samples) { return tiff_lzw_tile_slot_bytes(tile, samples); }
int flair_tiff_lzw_encode_tiles(const void* raster, int src_f32, const float* scale, int bands, int H, int W, int tile, int interleave,
                                long first_stream, long n_streams, uint8_t* out, long slot_bytes, int32_t* counts, void* stream) {
  return tiff_lzw_encode_tiles(raster, src_f32, scale, bands, H, W, tile, interleave, first_stream, n_streams, out, slot_bytes, counts,
                               (hipStream_t)stream);
}
int flair_tiff_pack_streams(const uint8_t* slots, long slot_bytes, const int32_t* counts, const int64_t* dst_off, long n_streams, uint8_t* dst,
                            long dst_bytes, void* stream) {
  return tiff_pack_streams(slots, slot_bytes, counts, (const long long*)dst_off, n_streams, dst, dst_bytes, (hipStream_t)stream);
}
int flair_tiff_lzw_decode_max_strip(void) { return tiff_lzw_decode_max_strip(); }
int flair_tiff_lzw_decode(const uint8_t* src, long src_bytes, const int64_t* strip_src_off, const int32_t* strip_src_len,
                          const int64_t* strip_dst_off, const int32_t* strip_dst_len, const int32_t* strip_mode, long nstrips, uint8_t* dst,
                          long dst_bytes, int32_t* status, void* stream) {
  return tiff_lzw_decode(src, src_bytes, (const long long*)strip_src_off, strip_src_len, (const long long*)strip_dst_off, strip_dst_len,
                         strip_mode, nstrips, dst, dst_bytes, status, (hipStream_t)stream);
}
int flair_tiff_lzw_decode_chunks_cap(void) { return tiff_lzw_decode_chunks_cap(); }
int flair_tiff_lzw_decode_chunks_window(void) { return tiff_lzw_decode_chunks_window(); }
int flair_tiff_lzw_decode_chunks(const uint8_t* src, long src_bytes, const int64_t* src_off, const int32_t* src_len, const int32_t* dst_len,
                                 const int32_t* mode, long nchunks, uint8_t* scratch, long slot_bytes, int32_t* status, void* stream) {
  return tiff_lzw_decode_chunks(src, src_bytes, (const long long*)src_off, src_len, dst_len, mode, nchunks, scratch, slot_bytes, status,
                                (hipStream_t)stream);
}
int flair_tiff_chunks_to_planes(const uint8_t* scratch, long slot_bytes, const int32_t* chunks, const int32_t* status, long nchunks,
                                int max_rows, int samples, int predictor, uint8_t* planes, int bands, int H, int W, void* stream) {
  return tiff_chunks_to_planes(scratch, slot_bytes, chunks, status, nchunks, max_rows, samples, predictor, planes, bands, H, W,
                               (hipStream_t)stream);
}
int flair_tiff_chunks_to_batch(const uint8_t* scratch, long slot_bytes, const int32_t* chunks, const int32_t* status, long nchunks,
                               int max_rows, uint8_t* planes, int n_planes, int H, int W, void* stream) {
  return tiff_chunks_to_batch(scratch, slot_bytes, chunks, status, nchunks, max_rows, planes, n_planes, H, W, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ SegFormer (zone_detect, HuggingFace provider)
int flair_segformer_create(flair_segformer_t** out, int in_channels, int num_labels, const int depths[4], const int hidden_sizes[4],
                           const int num_heads[4], const int sr_ratios[4], int decoder_hidden_size, int dtype) {
  if (!out || !depths || !hidden_sizes || !num_heads || !sr_ratios || in_channels < 1 || num_labels < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  for (int i = 0; i < 4; ++i)
    if (depths[i] < 1 || hidden_sizes[i] < 64 || (hidden_sizes[i] % 64) || num_heads[i] < 1 || hidden_sizes[i] != 64 * num_heads[i] ||
        sr_ratios[i] != (8 >> i))
      return -2;   // MiT-B1 .. B5 geometry: heads of 64 channels, reduction ratios 8 / 4 / 2 / 1
  if (decoder_hidden_size < 64 || (decoder_hidden_size % 64)) return -2;
  flair_segformer* h = new (std::nothrow) flair_segformer(in_channels, num_labels, depths, hidden_sizes, num_heads, sr_ratios,
                                                          decoder_hidden_size, dtype);
  if (!h) return -100;
  *out = h;
  return 0;
}
void flair_segformer_destroy(flair_segformer_t* h) { delete h; }
int64_t flair_segformer_param_count(const flair_segformer_t* h) { return h ? h->net.n_params : -1; }
int flair_segformer_num_tensors(const flair_segformer_t* h) { return h ? (int)h->net.tensors.size() : -1; }
int flair_segformer_tensor_info(const flair_segformer_t* h, int i, char* name, int name_cap, int64_t shape[4], int* ndim, int64_t* offset,
                                int* kind) {
  return h ? tf_tensor_info(h->net.tensors, i, name, name_cap, shape, ndim, offset, kind) : -1;
}
int64_t flair_segformer_workspace_bytes(flair_segformer_t* h, int B, int H, int W) {
  if (!h || B < 1 || !h->net.shape_ok(H, W)) return -1;
  return (int64_t)h->net.workspace_bytes(B, H, W);
}
void flair_segformer_weights_changed(flair_segformer_t* h) {
  if (h) h->net.weights_changed();
}
int flair_segformer_forward(flair_segformer_t* h, const float* params, const float* x_nchw, float* logits_quarter_nchw,
                            float* logits_full_nchw, int B, int H, int W, void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  return h->net.forward(params, x_nchw, logits_quarter_nchw, logits_full_nchw, B, H, W, ws, wsb, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ UperNet-Swin (HuggingFace provider)
int flair_upernet_create(flair_upernet_t** out, int in_channels, int num_labels, int embed_dim, const int depths[4], const int num_heads[4],
                         int window_size, int hidden_size, const int pool_scales[4], int auxiliary_in_channels, int auxiliary_channels,
                         int dtype) {
  if (!out || !depths || !num_heads || !pool_scales || in_channels < 1 || num_labels < 1) return -1;
  if (dtype != DT_F32 && dtype != DT_BF16) return -2;
  if (window_size != 7) return -2;   // the attention kernel's 7 x 7 windows (swin-tiny / -small)
  if (embed_dim < 32 || (embed_dim % 32)) return -2;
  for (int i = 0; i < 4; ++i)
    if (depths[i] < 1 || num_heads[i] * 32 != (embed_dim << i) || pool_scales[i] < 1 || pool_scales[i] > 64) return -2;   // heads of 32
  if (hidden_size < 64 || (hidden_size % 64) || auxiliary_in_channels < 1 || auxiliary_channels < 1) return -2;
  flair_upernet* h = new (std::nothrow) flair_upernet(in_channels, num_labels, embed_dim, depths, num_heads, hidden_size, pool_scales,
                                                      auxiliary_in_channels, auxiliary_channels, dtype);
  if (!h) return -100;
  *out = h;
  return 0;
}
void flair_upernet_destroy(flair_upernet_t* h) { delete h; }
int64_t flair_upernet_param_count(const flair_upernet_t* h) { return h ? h->net.n_params : -1; }
int flair_upernet_num_tensors(const flair_upernet_t* h) { return h ? (int)h->net.tensors.size() : -1; }
int flair_upernet_tensor_info(const flair_upernet_t* h, int i, char* name, int name_cap, int64_t shape[4], int* ndim, int64_t* offset,
                              int* kind) {
  return h ? tf_tensor_info(h->net.tensors, i, name, name_cap, shape, ndim, offset, kind) : -1;
}
int64_t flair_upernet_workspace_bytes(flair_upernet_t* h, int B, int H, int W) {
  if (!h || B < 1) return -1;
  if (!UperNet::shape_ok(H, W)) return -14;
  return (int64_t)h->net.workspace_bytes(B, H, W);
}
void flair_upernet_weights_changed(flair_upernet_t* h) {
  if (h) h->net.weights_changed();
}
int flair_upernet_forward(flair_upernet_t* h, const float* params, const float* x_nchw, float* logits_nchw, int B, int H, int W, void* ws,
                          size_t wsb, void* stream) {
  if (!h) return -1;
  if (!UperNet::shape_ok(H, W)) return -14;
  return h->net.forward(params, x_nchw, logits_nchw, B, H, W, ws, wsb, (hipStream_t)stream, false);
}
int flair_upernet_forward_quarter(flair_upernet_t* h, const float* params, const float* x_nchw, float* logits_quarter_nchw, int B, int H,
                                  int W, void* ws, size_t wsb, void* stream) {
  if (!h) return -1;
  if (!UperNet::shape_ok(H, W)) return -14;
  if ((H % 4) || (W % 4)) return -2;
  return h->net.forward(params, x_nchw, logits_quarter_nchw, B, H, W, ws, wsb, (hipStream_t)stream, true);
}

}  // extern "C"
