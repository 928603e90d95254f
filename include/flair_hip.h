/* flair_hip.h — C ABI of the MI355X-native FLAIR-1 segmentation hot path (libflair_hip.so).
 *
 * Drop-in boundary.  The reference is Python; the calls a maintainer would bind
 * (ctypes) are listed next to the reference interface each one replaces.
 * Conventions: plain pointers and sizes only, no torch types; every pointer is DEVICE memory unless
 * marked host; every function enqueues work on `stream` (a hipStream_t passed as void*) and never
 * synchronises, allocates or frees device memory; return value 0 = ok, >0 = hipError_t,
 * <0 = argument error (flair_strerror).  Tensors at the boundary use the reference's layouts:
 * images / logits / features NCHW fp32, labels (B,H,W), parameters PyTorch OIHW fp32.
 * Internally activations are NHWC in `dtype` (0 = fp32 parity mode, 1 = bf16 throughput mode).
 */
#ifndef FLAIR_HIP_H
#define FLAIR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLAIR_DT_F32 0
#define FLAIR_DT_BF16 1

const char* flair_strerror(int code);
int flair_version(void);

/* ------------------------------------------------------------------------------------------------
 * Model object.  Replaces smp.create_model(arch='unet', encoder_name='resnet34', classes, in_channels)
 * — /root/reference/src/flair/model.py:37-41 and src/zone_detect/model.py:34-39.
 * The handle holds only host-side metadata (layer table, arena plan); parameters stay in the
 * caller's flat fp32 buffers laid out as flair_unet_tensor_info describes (names = smp-0.3.3
 * state_dict keys). */
typedef struct flair_unet flair_unet_t;
int flair_unet_create(flair_unet_t** out, int in_channels, int classes, int dtype);
void flair_unet_destroy(flair_unet_t* h);
int64_t flair_unet_param_count(const flair_unet_t* h);   /* floats in the flat parameter / gradient buffer */
int64_t flair_unet_buffer_count(const flair_unet_t* h);  /* floats in the flat BN running-stat buffer */
int flair_unet_num_tensors(const flair_unet_t* h);
/* kind: 0 = parameter (offset into params/grads), 1 = running statistic (offset into buffers);
 * stage: 0 stem, 1-4 encoder layers, 5 decoder, 6 head — contiguous gradient buckets. */
int flair_unet_tensor_info(const flair_unet_t* h, int i, char* name, int name_cap, int64_t shape[4], int* ndim,
                           int64_t* offset, int* kind, int* stage);
int flair_unet_stage_range(const flair_unet_t* h, int stage, int64_t* begin, int64_t* end);
/* training = 0 / 1: the bound that holds for every entry point (the split sequence with every activation materialised).
 * training = 2: the arena of one whole-model training step, flair_unet_forward(training = 1, no fp32 logits) + flair_unet_backward,
 * as they run under the current flair_tune_set settings: smaller (lazy BatchNorm; no dy tensor for a layer whose backward runs as
 * the fused 16-channel kernel).  Valid for that pair of calls only, and only while the settings stay what they were. */
int64_t flair_unet_workspace_bytes(flair_unet_t* h, int B, int H, int W, int training);

/* Options of ONE flair_unet_forward.  The struct is read during the call and nothing of it is kept: what a forward does depends on
 * its own arguments only, never on an earlier call.  Every pointer is a device pointer; the outputs (preds_u8, maxprob_f32, ce_loss,
 * ce_preds_u8, ce_confmat, ce_workspace) must stay valid until the enqueued work has run, drows_f32 until the flair_unet_backward of
 * this forward has run.  A zeroed struct, like opts == NULL, asks for nothing.  Malformed options (below) return -1, combinations a
 * forward cannot serve -15 / -16 / -17, all of them before anything is enqueued or the handle is touched. */
typedef struct flair_unet_fwd_opts {
  /* Inference with constant weights (zone_detect's window loop, predict): a promise that `params` and `buffers` are bit-identical
   * to those of the previous eval-mode flair_unet_forward on this handle.  Honoured only if this is an eval-mode forward with the
   * same workspace, shape and `params` / `buffers` pointers and no other call on the handle came between: it then skips re-packing
   * the weights and re-deriving the 46 BatchNorm affine pairs (both are still in the workspace); with other pointers the promise
   * cannot be about what was packed and the forward packs again.  The reference has no counterpart: PyTorch modules keep their
   * weights in the layout they compute in. */
  int reuse_constants;
  /* uint8 argmax predictions [B][H][W] — predict_step's argmax(softmax(logits)), task_module.py:206-213 — from the head
   * convolution's epilogue; the logits are then not kept (flair_unet_logits_nhwc returns NULL until the next forward).  Used only
   * by a forward with training = 0 and logits_nchw = NULL; any other forward ignores both fields.  maxprob_f32 (optional, needs
   * preds_u8): the winner's softmax probability, fp32 [B][H][W]. */
  uint8_t* preds_u8; float* maxprob_f32;
  /* ce_labels != NULL: the head of step() on this forward's logits — task_module.py:71-79, tasks_utils.py:88-93, what
   * validation_step needs: the weighted cross-entropy mean -> ce_loss, argmax(softmax) -> ce_preds_u8 (optional),
   * ce_confmat[target][pred] += 1 (int64 [C][C], optional).  Labels and ce_label_kind (0..3) as for flair_ce_head; ce_workspace:
   * flair_ce_workspace_bytes(B, H, W).  Where the head convolution's persistent kernel takes the shape — preds_u8's condition, and
   * the head's 16 input channels materialised (not handed over as a lazy BatchNorm input, FLAIR_LAZY_BN >= 2) — and the tune key
   * FLAIR_HEAD_CE is on (default off) all of it happens in that kernel's epilogue and the logits are not kept
   * (flair_unet_logits_nhwc returns NULL); otherwise the same call runs the head convolution and flair_ce_head_nhwc's kernels on
   * its NHWC logits.  Needs training = 0, logits_nchw = NULL and preds_u8 = NULL (-15 otherwise).  ce_labels == NULL: no CE
   * head, the other ce_ fields are not read. */
  const void* ce_labels; int ce_label_kind; const float* ce_class_weight; float* ce_loss;
  uint8_t* ce_preds_u8; int64_t* ce_confmat; void* ce_workspace;
  /* Bottleneck rows, fp32 (B, H/32): the metadata fusion of model.py:57-62 (x_enc of MetadataMLP; at 512 x 512 tiles H/32 = 16 =
   * its width) without leaving the fused forward, element [b][c][h][w] of the encoder's last feature + rows[b][h].  Combines with
   * everything above.  training = 0: added in place between the encoder and the decoder (flair_add_rowvec_nhwc).  training = 1:
   * the decoder reads a second tensor, dtype(float(f5) + rows[b][h]) (flair_add_rowvec_nhwc_to; f5 itself stays, it is the ReLU
   * mask source of layer4's last block), and drows_f32 is required (-16 without it); the workspace size and layout bound of
   * flair_unet_workspace_bytes hold. */
  const float* rows_f32;
  /* Training forwards only (-17 otherwise), needs rows_f32: the flair_unet_backward of this forward writes
   * drows_f32[b][h] = sum over c, w of the gradient reaching the second tensor (flair_rowvec_grad_nhwc) before it walks the
   * encoder.  The handle keeps this one pointer from the forward to its backward; any later forward that is
   * not refused drops it. */
  float* drows_f32;
} flair_unet_fwd_opts_t;

/* seg_model(x)  — model.py:64 (and zone_detect/compare.py:31).  training != 0: BatchNorm batch
 * statistics + running-stat update in `buffers`, activations kept in `workspace` for backward.
 * opts: what else this forward does (above); NULL = a plain forward. */
int flair_unet_forward(flair_unet_t* h, const float* params, float* buffers, const float* x_nchw, float* logits_nchw,
                       int B, int H, int W, int training, void* workspace, size_t workspace_bytes, void* stream,
                       const flair_unet_fwd_opts_t* opts);
/* autograd backward of the call above (Lightning's loss.backward(), task_module.py:82-86).
 * Exactly one of dlogits_nchw (fp32 (B,C,H,W)) / dlogits_nhwc (as written by flair_ce_head with
 * flair_unet_head_ld) is non-null.  Writes every parameter gradient into `grads` (flat, OIHW).
 * stage_events: optional array of 7 hipEvent_t (null = none); event k is recorded on `stream` as soon as
 * the gradients of bucket k (flair_unet_stage_range) are final — ready order 6,5,4,3,2,1,0 — so the
 * host can start the RCCL all-reduce of a bucket while the rest of backward still runs. */
int flair_unet_backward(flair_unet_t* h, const float* params, const float* dlogits_nchw, const void* dlogits_nhwc,
                        float* grads, void* workspace, size_t workspace_bytes, void* stream,
                        void* const* stage_events);
int flair_unet_head_ld(const flair_unet_t* h);

/* seg_model.encoder(x) / .decoder(*feats) / .segmentation_head(t) — the metadata path model.py:57-62.
 * feats[i] = feature i+1 of the encoder, NCHW fp32: (B,64,H/2,W/2) ... (B,512,H/32,W/32). */
int flair_unet_encoder_forward(flair_unet_t* h, const float* params, float* buffers, const float* x_nchw,
                               float* const feats_nchw[5], int B, int H, int W, int training, void* workspace,
                               size_t workspace_bytes, void* stream);
int flair_unet_decoder_forward(flair_unet_t* h, const float* params, float* buffers, const float* const feats_nchw[5],
                               float* out_nchw, int B, int H, int W, int training, void* workspace,
                               size_t workspace_bytes, void* stream);
int flair_unet_head_forward(flair_unet_t* h, const float* params, const float* x_nchw, float* logits_nchw, int B, int H,
                            int W, int training, void* workspace, size_t workspace_bytes, void* stream);
int flair_unet_head_backward(flair_unet_t* h, const float* params, const float* dlogits_nchw, float* dx_nchw,
                             float* grads, void* workspace, size_t workspace_bytes, void* stream);
int flair_unet_decoder_backward(flair_unet_t* h, const float* params, const float* dout_nchw,
                                float* const dfeats_nchw[5], float* grads, void* workspace, size_t workspace_bytes,
                                void* stream);
int flair_unet_encoder_backward(flair_unet_t* h, const float* params, const float* const dfeats_nchw[5], float* grads,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused per-pixel head.  Replaces, in one pass over the logits,
 *   targets = argmax(msk, 1); loss = criterion(logits, targets)            task_module.py:71-72
 *   nn.CrossEntropyLoss(weight) mean reduction                              tasks_utils.py:88-93
 *   preds = argmax(softmax(logits, 1), 1)                                   task_module.py:75-76
 *   MulticlassJaccardIndex.update: confmat += bincount(target*C + pred)     task_module.py:85,107-108
 * label_kind: 0 uint8 (B,H,W), 1 int32, 2 int64, 3 fp32 one-hot (B,C,H,W) (the reference's batch["msk"]).
 * A label outside [0, C) is ignored (no loss, no gradient, no count), judged in the label's own width: the int64 label 2^32 + 3 is
 * ignored, not class 3.  targets_i32 gets the label itself, or -1 for an ignored int64 label that int32 cannot hold.
 * Outputs are optional (null = skip).  workspace: flair_ce_workspace_bytes(), 4-byte aligned.
 * Returns, before anything is enqueued: -1 a required pointer is null or label_kind is outside 0..3; -2 C outside 1..32 (or, _nhwc,
 * a dtype that is neither fp32 nor bf16); -3 NHWC rows: ld not 16 / 24 / 32 (_nhwc) or < C, dlogits_ld < C, > 32 or not whole
 * 16-byte chunks (a multiple of 4 fp32 / 8 bf16), logits_nhwc or dlogits_nhwc not 16-byte aligned, workspace not 4-byte aligned. */
size_t flair_ce_workspace_bytes(int B, int H, int W);
int flair_ce_head(const float* logits_nchw, const void* labels, int label_kind, const float* class_weight, int B, int C,
                  int H, int W, float* loss, float* dlogits_nchw, void* dlogits_nhwc, int dlogits_dtype, int dlogits_ld,
                  uint8_t* preds_u8, int64_t* preds_i64, int32_t* targets_i32, int64_t* confmat, void* workspace,
                  void* stream);
/* The same head over logits left in the network's own layout: flair_unet_forward called with logits_nchw == NULL
 * (training) keeps the segmentation head's output as NHWC rows [B*H*W][flair_unet_head_ld()] of the model's compute
 * dtype inside the workspace; flair_unet_logits_nhwc returns that buffer (valid until the next forward on the arena).
 * Same arithmetic and outputs as flair_ce_head (in bf16 mode the fp32 NCHW logits are these values widened); dl_nhwc has
 * the layout flair_unet_backward takes.  Replaces task_module.py:71-79 + tasks_utils.py:88-93 for a loop that never
 * looks at the logits themselves (flair_amd.SegTrainer). */
const void* flair_unet_logits_nhwc(const flair_unet_t* h);
int flair_ce_head_nhwc(const void* logits_nhwc, int dtype, int ld, const void* labels, int label_kind,
                       const float* class_weight, int B, int C, int H, int W, float* loss, void* dlogits_nhwc,
                       uint8_t* preds_u8, int32_t* targets_i32, int64_t* confmat, void* workspace, void* stream);
/* The same head with a configurable objective in place of the weighted cross entropy (the criteria the reference's model library
 * ships as smp.losses; the reference's own criterion stays flair_ce_head):
 *   loss = ce * CE + dice * Dice
 *   CE, focal_gamma == 0:  F.cross_entropy(logits, y, weight, ignore_index, label_smoothing) with mean reduction
 *   CE, focal_gamma >= 1:  (1/D) sum_i w[y_i] q_i^gamma (-log p_{i,y_i}),  q_i = sum over c != y_i of p_ic,  D = sum_i w[y_i]
 *   Dice: soft multiclass Dice over the pixels with a valid label of non-zero weight, averaged over the C classes, the classes
 *         without such a pixel counting 0:  1 - (2 I_c + dice_smooth) / max(P_c + T_c + dice_smooth, dice_eps)
 * Labels, label kinds, ignored labels, preds, targets and confmat as for flair_ce_head; preds and confmat are bit-identical to its.
 * loss3: three floats [loss, CE, Dice].  dlogits: the gradient of loss, fp32 NCHW (flair_seg_loss) or NHWC rows of `dtype` with
 * stride ld and zeroed padding columns (flair_seg_loss_nhwc, ld 16 or 32).  workspace: flair_seg_loss_workspace_bytes(), 4-byte
 * aligned.  No floating-point atomics: two calls on the same input give the same bits.
 * A spec is invalid (-20) when: ce < 0 or dice < 0 or both 0; label_smoothing outside [0, 1); focal_gamma neither 0 nor >= 1;
 * label_smoothing > 0 with focal_gamma > 0; either of them with ce == 0; dice_smooth < 0; dice_eps <= 0; any field not finite.
 * Other codes as for flair_ce_head(_nhwc), all returned before anything is enqueued. */
typedef struct flair_seg_loss { float ce, label_smoothing, focal_gamma, dice, dice_smooth, dice_eps; } flair_seg_loss_t;
size_t flair_seg_loss_workspace_bytes(int B, int C, int H, int W);
int flair_seg_loss(const float* logits_nchw, const void* labels, int label_kind, const float* class_weight, int B, int C, int H,
                   int W, const flair_seg_loss_t* spec, float* loss3, float* dlogits_nchw, uint8_t* preds_u8, int64_t* preds_i64,
                   int32_t* targets_i32, int64_t* confmat, void* workspace, void* stream);
int flair_seg_loss_nhwc(const void* logits_nhwc, int dtype, int ld, const void* labels, int label_kind, const float* class_weight,
                        int B, int C, int H, int W, const flair_seg_loss_t* spec, float* loss3, void* dlogits_nhwc,
                        uint8_t* preds_u8, int32_t* targets_i32, int64_t* confmat, void* workspace, void* stream);
/* predict_step over NHWC logits left in the workspace (flair_unet_forward with logits_nchw == NULL, flair_unet_logits_nhwc). */
int flair_softmax_argmax_nhwc(const void* logits_nhwc, int dtype, int ld, int B, int C, int H, int W, uint8_t* preds_u8,
                              int64_t* preds_i64, float* maxprob, void* stream);
/* predict_step: argmax(softmax(logits)) — task_module.py:211-212; with maxprob also
 * zone_detect inference + convert('argmax') — src/zone_detect/compare.py:35, dataset.py:23-30. */
int flair_softmax_argmax(const float* logits_nchw, int B, int C, int H, int W, uint8_t* preds_u8, int64_t* preds_i64,
                         float* maxprob, void* stream);
/* confmat[target][pred] += 1 — torchmetrics update / sklearn confusion_matrix at src/flair/metrics.py:67-71.
 * kinds: 0 uint8, 1 int32, 2 int64. */
int flair_confmat_update(const void* target, int target_kind, const void* pred, int pred_kind, int64_t n, int C,
                         int64_t* confmat, void* stream);
/* Offline evaluation: sum over tiles of sklearn.confusion_matrix((truth - 1).flatten(), pred.flatten(),
 * labels=range(C)) — src/flair/metrics.py:60-75.  truth_offset is added to the truth byte with uint8
 * wrap-around (-1: a stored 0 becomes 255); pairs with a member outside range(C) are dropped.  Both rasters
 * 16-byte aligned. */
int flair_confmat_masks(const uint8_t* truth_raw, const uint8_t* pred, int64_t n, int C, int truth_offset, int64_t* confmat,
                        void* stream);
/* MulticlassJaccardIndex.compute (average None / 'weighted' / 'macro') — task_module.py:36-51,90,113-114. */
int flair_jaccard(const int64_t* confmat, int C, float* per_class, float* weighted, float* macro, void* stream);

/* torch.optim.SGD(lr) step, no momentum / weight decay — tasks_utils.py:95. */
/* ------------------------------------------------------------------------------------------------
 * Input contract of the step on device: what fit_dataset.__getitem__ /
 * predict_dataset.__getitem__ (src/flair/data_loader.py:74-95,130-144) and the augmentation set of
 * src/flair/tasks_utils.py:37-41 do per tile on CPU workers, for a whole batch of stored uint8 rasters.
 *   img_u8 (B, bands, H, W): bands as stored; channels[n_channels] = the config's 1-based band list
 *   norm_type 0 'without' | 1 'scaling' (x * (1/255) in fp64) | 2 'custom' ((x - mean) / std in fp64), then fp32
 *     — data_loader.py:9-30
 *   msk_raw (B, H, W): stored label raster; labels_out = argmax over the one-hot of (raw - 1) (data_loader.py:65-69,
 *     task_module.py:71): raw 1..C -> 0..C-1, anything else -> class 0
 *   d4_flags (B) or null: bit0 VerticalFlip, bit1 HorizontalFlip, bits 2-3 RandomRotate90 factor, applied in that
 *     order to image and labels alike; needs H == W.
 * img_out (B, n_channels, H, W) fp32 NCHW and/or labels_out (B, H, W) uint8; either may be null. W % 4 == 0. */
int flair_feed_tiles(const uint8_t* img_u8, const uint8_t* msk_raw, const uint8_t* d4_flags, int B, int bands, int H, int W,
                     const int* channels, int n_channels, int norm_type, const double* means, const double* stds,
                     int num_classes, float* img_out, uint8_t* labels_out, void* stream);
/* flair_feed_tiles over samples that do not lie one behind the other (flair_amd/tile_cache.py: tiles resident in cache slots next
 * to tiles a decode just wrote): the same arithmetic, the sources from two device tables of B 64-bit device addresses each.
 *   img_ptrs[b]: sample b's (bands, H, W) uint8 planes, contiguous, any byte alignment; 0: the sample is skipped, nothing of its
 *     img_out / labels_out is written
 *   msk_ptrs[b]: its (H, W) raw mask; msk_ptrs may be null without labels_out; an entry 0 leaves the sample's labels unwritten
 * The same address may stand for several samples.  The other arguments and their checks are flair_feed_tiles'.
 * Returns -1 for a null img_ptrs and for labels_out without msk_ptrs, -2 for a table that is not 8-byte aligned. */
int flair_feed_tiles_ptrs(const uint64_t* img_ptrs, const uint64_t* msk_ptrs, const uint8_t* d4_flags, int B, int bands, int H, int W,
                          const int* channels, int n_channels, int norm_type, const double* means, const double* stds,
                          int num_classes, float* img_out, uint8_t* labels_out, void* stream);
/* zone_detect: softmax over classes (src/zone_detect/compare.py:35), margin crop (compare.py:71-75) and
 * convert (src/zone_detect/dataset.py:11-34) without the probability tensor ever leaving the device.
 * output_type 0 'argmax': out fp32 (B, 2, S-2m, S-2m) = [first argmax, max probability];
 * output_type 1 'class_prob': out uint8 (B, C, S-2m, S-2m) = trunc(p * 255);
 * output_type 2 (flair_detect_convert only): no convert, out fp32 (B, C, S-2m, S-2m) = the probabilities themselves — with
 *   m = 0 the return value of the reference's inference(), compare.py:35-39. */
int flair_detect_convert(const float* logits_nchw, int B, int C, int S, int margin, int output_type, void* out, void* stream);
/* Sliding-window detection over ONE raster resident in HBM (zone_detect default pipeline, src/zone_detect/main.py:386-428).
 * tiles (device, B x 6 int32): {x0, y0, wx0, wx1, wy0, wy1} per window — top-left pixel of the S x S window in raster
 * coordinates (may lie outside: Sliced_Dataset reads boundless, src/zone_detect/dataset.py:96-103, so missing pixels are 0
 * before normalisation) and the raster rectangle [wx0,wx1) x [wy0,wy1) this window owns in the output (its margin-cropped
 * centre minus what later windows of the slicing job overwrite; stitching 'exact-clipping', compare.py:69-82).
 * flair_gather_tiles: the dataset's read + normalization (dataset.py:66-88,90-113) -> img_out fp32 (B, n_channels, S, S).
 * flair_detect_stitch: softmax + crop + convert as flair_detect_convert, written straight into raster_out
 *   ((2, raster_h, raster_w) fp32 for 'argmax', (C, raster_h, raster_w) uint8 for 'class_prob'). */
int flair_gather_tiles(const uint8_t* raster_u8, int bands, int raster_h, int raster_w, const int32_t* tiles, int B, int S,
                       const int* channels, int n_channels, int norm_type, const double* means, const double* stds,
                       float* img_out, void* stream);
/* flair_detect_stitch_preds: convert('argmax') + stitch (dataset.py:23-30, main.py:404-421) from the per-window class / probability maps
 * flair_unet_fwd_opts_t::preds_u8 / maxprob_f32 leave, instead of from logits: raster_out (2, raster_h, raster_w) fp32 = [class, its softmax probability]. */
int flair_detect_stitch_preds(const uint8_t* preds_u8, const float* maxprob_f32, int B, int S, int margin, const int32_t* tiles,
                              float* raster_out, int raster_h, int raster_w, void* stream);
int flair_detect_stitch(const float* logits_nchw, int B, int C, int S, int margin, int output_type, const int32_t* tiles,
                        void* raster_out, int raster_h, int raster_w, void* stream);
/* Overlap stitching of zone_detect ('average', 'average_weights', 'max'; src/zone_detect/compare.py:84-136, intent as DESIGN §8
 * states it): windows of the slicing job overlap (stride < S - 2m) and every window contributes its margin-cropped centre
 * [x0+m, x0+S-m) x [y0+m, y0+S-m) clipped to the raster.  Each call touches the raster rectangle [x_lo, x_hi) x [y_lo, y_hi)
 * only, one thread per pixel walking the call's B windows (tiles as above; only x0, y0 are read) in job order: no atomics,
 * the result does not depend on how the job is cut into calls.
 * flair_detect_blend_accum: ring (C+1, raster_h, S-2m) fp32, raster column x at ring column x mod (S-2m), += w * softmax(logits)
 *   per class and += w in plane C; w = 1 when cheb_weights is null, else cheb_weights[max(|i - S/2|, |j - S/2|)] at patch pixel
 *   (i, j) (S/2 + 1 fp32 entries: patch_weights(S, 0.5, 'exp') by Chebyshev distance).  x_hi - x_lo <= S - 2m.
 * flair_detect_blend_flush: ring columns of raster columns [x_lo, x_hi) (x_hi - x_lo <= ring_cols), every row: where plane C
 *   is > 0, raster_out (2, raster_h, raster_w) fp32 = [first argmax, max] of sum(w p) / sum(w); those ring entries are zeroed.
 * flair_detect_stitch_max(_preds): raster_out (2, raster_h, raster_w) fp32 holds a running [class, probability]; a window's
 *   (first argmax, its probability) — of softmax(logits), or the maps a forward with preds_u8 / maxprob_f32 leaves — replaces it unless the
 *   held probability is strictly greater. */
int flair_detect_blend_accum(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, const float* cheb_weights,
                             int x_lo, int x_hi, int y_lo, int y_hi, float* ring, int raster_h, int raster_w, void* stream);
int flair_detect_blend_flush(float* ring, int C, int ring_cols, int x_lo, int x_hi, float* raster_out, int raster_h, int raster_w,
                             void* stream);
int flair_detect_stitch_max(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, int x_lo, int x_hi,
                            int y_lo, int y_hi, float* raster_out, int raster_h, int raster_w, void* stream);
int flair_detect_stitch_max_preds(const uint8_t* preds_u8, const float* maxprob_f32, int B, int S, int margin, const int32_t* tiles,
                                  int x_lo, int x_hi, int y_lo, int y_hi, float* raster_out, int raster_h, int raster_w, void* stream);
/* The _q4 family: the function of the same name without the suffix, argument for argument, except that logits_nchw is the
 * QUARTER-resolution fp32 (B, C, S/4, S/4) tensor a HuggingFace-provider model's classifier writes (flair_segformer_forward's
 * logits_quarter_nchw, flair_upernet_forward_quarter).  S, margin, tiles and every rectangle stay in tile / raster pixels.  Each
 * thread computes, for its own pixel, the value nn.functional.interpolate(scale_factor=4, mode="bilinear", align_corners=False)
 * gives there — the arithmetic of flair_sf_bilinear_nchw_f32, operation for operation — and goes on as the full-resolution
 * function does, so the (B, C, S, S) tensor is never written.  S % 4 != 0 returns -2, as does whatever the full-resolution
 * function rejects. */
int flair_detect_convert_q4(const float* logits_nchw, int B, int C, int S, int margin, int output_type, void* out, void* stream);
int flair_detect_stitch_q4(const float* logits_nchw, int B, int C, int S, int margin, int output_type, const int32_t* tiles,
                           void* raster_out, int raster_h, int raster_w, void* stream);
int flair_detect_blend_accum_q4(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, const float* cheb_weights,
                                int x_lo, int x_hi, int y_lo, int y_hi, float* ring, int raster_h, int raster_w, void* stream);
int flair_detect_stitch_max_q4(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles, int x_lo, int x_hi,
                               int y_lo, int y_hi, float* raster_out, int raster_h, int raster_w, void* stream);

/* Test-time augmentation over the D4 group of the training augmentation (csrc/tta.hip).  `code` is the packing of
 * d4_flags above: bit 0 V-flip, bit 1 H-flip, bits 2-3 the rot90 count k; T = rot90^k(hflip(vflip(.))), numpy's counter-clockwise
 * rot90.  Codes outside 0..15 return -2, an odd k with H != W returns -19, null tensors -1; nothing is launched then.
 * flair_d4_nchw_f32: out = T(in) for fp32 (B, C, H, W), out of place (in == out returns -1): a pure permutation.
 * flair_tta_accum: one pass of the ensemble S = sum over codes of T^-1(softmax(f(T(x)))).  logits_nchw (B, C, H, W) are the
 *   model's logits of T(x); their per-pixel softmax (flair_softmax_argmax's arithmetic) is added into acc_nchw fp32 (B, C, H, W)
 *   at the pixel of x it belongs to.  first != 0: stored instead of added (acc may hold anything).  preds_u8 != NULL marks the
 *   last of n passes (n in 1..16): the sum is finished in registers, preds_u8 (B, H, W) = the lowest class of the largest sum,
 *   the optional prob_f32 (B, H, W) = that sum / n (fp32 division), and acc is not written.  A pass that is first and last never
 *   touches acc (which may be NULL then and only then).  prob_f32 without preds_u8 returns -1; C outside 1..32 or n outside
 *   1..16 returns -2.  No atomics: the sum at a pixel is the same fp32 additions in pass order on every run.
 * flair_tta_accum_q4: the same over QUARTER-resolution logits (B, C, H/4, W/4), resized x4 per pixel as the _q4 family above
 *   does (H == W, H % 4 == 0, else -2); acc, preds and prob stay (B, ., H, W). */
int flair_d4_nchw_f32(const float* in_nchw, float* out_nchw, int B, int C, int H, int W, int code, void* stream);
int flair_tta_accum(const float* logits_nchw, int B, int C, int H, int W, int code, int first, float* acc_nchw, uint8_t* preds_u8,
                    float* prob_f32, int n, void* stream);
int flair_tta_accum_q4(const float* logits_nchw, int B, int C, int H, int W, int code, int first, float* acc_nchw, uint8_t* preds_u8,
                       float* prob_f32, int n, void* stream);

/* zone_detect's comparison metrics against a ground-truth raster (src/zone_detect/test/metrics.py; csrc/zone_metrics.hip).
 * truth_u8 (raster_h, raster_w): the stored label raster; its class is (truth - 1) in uint8 arithmetic, so a 0 becomes 255.
 * Every count is sklearn's confusion_matrix(truth - 1, pred, labels=range(C)): rows truth, columns prediction, pairs with a
 * member outside range(C) dropped.  Matrices are int64 and ADDED to (callers zero them); C <= 32.
 * flair_zone_window_confmat_*: confmats (B, C, C), one per window b over its margin-cropped core
 *   [x0+m, x0+S-m) x [y0+m, y0+S-m) clipped to the raster (tiles as flair_detect_stitch; only x0, y0 are read), the prediction
 *   being the window's own u8 class tile (B, S, S) (_preds), the class flair_detect_stitch writes from its fp32 logits
 *   (B, C, S, S) (_logits), or band 0 of the finished fp32 raster (2, raster_h, raster_w) (_raster).
 * flair_zone_raster_confmat: confmat (C, C) of band 0 of the fp32 raster (2, raster_h, raster_w) over the whole raster.
 * flair_zone_error_map: error_rate_patch (metrics.py:350-442) of band 0: for the n_rows x n_cols patches at
 *   (row_origins[a], col_origins[b]) (device int32; each patch K x K inside the raster), the mean over patches of the K x K map
 *   [truth - 1 != class] (no-data counts as an error), then scipy.ndimage.gaussian_filter(., sigma, mode='reflect') with
 *   truncate radius `radius` (<= 32), in fp64 -> error_map (K, K).  Workspaces: mask_ws raster_h * raster_w bytes,
 *   colsum_ws raster_h * K int32, counts_ws K * K int32, tmp_ws K * K fp64. */
int flair_zone_window_confmat_preds(const uint8_t* preds_u8, int B, int C, int S, int margin, const int32_t* tiles,
                                    const uint8_t* truth_u8, int raster_h, int raster_w, int64_t* confmats, void* stream);
int flair_zone_window_confmat_logits(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles,
                                     const uint8_t* truth_u8, int raster_h, int raster_w, int64_t* confmats, void* stream);
/* as flair_zone_window_confmat_logits from quarter-resolution logits (B, C, S/4, S/4): see the _q4 family above */
int flair_zone_window_confmat_logits_q4(const float* logits_nchw, int B, int C, int S, int margin, const int32_t* tiles,
                                        const uint8_t* truth_u8, int raster_h, int raster_w, int64_t* confmats, void* stream);
int flair_zone_window_confmat_raster(const float* raster, int B, int C, int S, int margin, const int32_t* tiles, const uint8_t* truth_u8,
                                     int raster_h, int raster_w, int64_t* confmats, void* stream);
int flair_zone_raster_confmat(const float* raster, const uint8_t* truth_u8, int raster_h, int raster_w, int C, int64_t* confmat,
                              void* stream);
int flair_zone_error_map(const float* raster, const uint8_t* truth_u8, int raster_h, int raster_w, int K, const int32_t* row_origins,
                         int n_rows, const int32_t* col_origins, int n_cols, double sigma, int radius, uint8_t* mask_ws,
                         int32_t* colsum_ws, int32_t* counts_ws, double* tmp_ws, double* error_map, void* stream);

/* TIFF 6.0 LZW (Compression = 5, no predictor) of uint8 tiles on the device (csrc/tiff_lzw.hip): the streams of the PRED_*.tif files.
 * img (B, H, W) uint8.  Strip s of tile b covers rows [s*R, min(H, (s+1)*R)), R = rows_per_strip, as one byte stream; its LZW stream
 * (ClearCode first, EOI last, codes MSB first, the widths and the table reset of libtiff's encoder) is written to
 * out + (b*nstrips + s) * slot_bytes and its length in bytes to counts[b*nstrips + s], nstrips = ceil(H / R).  Bytes of a slot past
 * its count are unspecified; nothing is written outside a slot.
 * flair_tiff_lzw_slot_bytes: the smallest slot_bytes the encoder accepts, a multiple of 16 that holds the longest possible stream of
 *   a full strip; -1 for rows_per_strip < 1 or W < 1.
 * flair_tiff_lzw_encode: -1 for a null pointer or an extent / rows_per_strip < 1, -100 for slot_bytes below
 *   flair_tiff_lzw_slot_bytes, -2 unless out is 16-byte aligned, slot_bytes a multiple of 16 and counts 4-byte aligned. */
long flair_tiff_lzw_slot_bytes(int rows_per_strip, int W);
int flair_tiff_lzw_encode(const uint8_t* img, int B, int H, int W, int rows_per_strip, uint8_t* out, long slot_bytes, int32_t* counts,
                          void* stream);
/* The same streams, one per TIFF tile of a raster resident on the device (the file of zone_detect, flair_amd/raster_writer.py).
 * raster (bands, H, W) in band planes: uint8 (src_f32 = 0, scale unused) or fp32 (src_f32 = 1) with scale[bands] on the device,
 *   byte = (uint8) trunc(min(max(v * scale[band], 0), 255)), NaN -> 0: one fp32 multiply, no FMA.
 * Tiles are tile x tile pixels, tile a multiple of 16, ty = ceil(H / tile) by tx = ceil(W / tile) of them; pixels of a tile outside
 *   the raster are 0 (TIFF tiles are always full size).
 * interleave 0 (band, PlanarConfiguration 2): bands * ty * tx streams, stream (b * ty + y) * tx + x is the tile * tile bytes of band
 *   b's tile (y, x), row-major.  interleave 1 (pixel, PlanarConfiguration 1): ty * tx streams of tile * tile * bands bytes, byte k is
 *   row k / (tile * bands), column (k / bands) % tile, band k % bands.
 * Streams [first_stream, first_stream + n_streams) are encoded: stream first_stream + i goes to out + i * slot_bytes, its length to
 *   counts[i]; bytes of a slot past its count are unspecified, nothing is written outside a slot.
 * flair_tiff_lzw_tile_slot_bytes: the smallest slot_bytes accepted, flair_tiff_lzw_slot_bytes' bound for tile * tile * samples bytes
 *   (samples = 1 for band interleave, bands for pixel interleave); -1 for an argument < 1 or a stream above 2^30 bytes.
 * flair_tiff_lzw_encode_tiles: -1 for a null pointer (scale with src_f32 = 1 included), an extent < 1, a tile that is no multiple of
 *   16, a flag other than 0 / 1 or a window outside the streams; -100 for slot_bytes below flair_tiff_lzw_tile_slot_bytes; -2 unless
 *   out is 16-byte aligned, slot_bytes a multiple of 16 and counts, scale and an fp32 raster 4-byte aligned. */
long flair_tiff_lzw_tile_slot_bytes(int tile, int samples);
int flair_tiff_lzw_encode_tiles(const void* raster, int src_f32, const float* scale, int bands, int H, int W, int tile, int interleave,
                                long first_stream, long n_streams, uint8_t* out, long slot_bytes, int32_t* counts, void* stream);
/* Compaction of encoded streams: the counts[i] bytes at slots + i * slot_bytes are copied to dst + dst_off[i], i < n_streams, one
 * workgroup per stream, 16 bytes per lane.  dst_off (int64, on the device) holds multiples of 16; the bytes from the stream's end to
 * the next multiple of 16 are written as zeros, nothing else of dst is written: stream i owns
 * [dst_off[i], dst_off[i] + round_up(counts[i], 16)).  A stream with a count outside [0, slot_bytes], or whose offset is negative, no
 * multiple of 16 or leaves that range outside [0, dst_bytes), is skipped.  -1 for a null pointer, n_streams < 1, slot_bytes < 16 or
 * dst_bytes < 0; -2 unless slots and dst are 16-byte aligned, slot_bytes a multiple of 16, counts 4-byte and dst_off 8-byte aligned. */
int flair_tiff_pack_streams(const uint8_t* slots, long slot_bytes, const int32_t* counts, const int64_t* dst_off, long n_streams, uint8_t* dst,
                            long dst_bytes, void* stream);
/* The inverse on the device (the read path of metrics()): strip i, the bytes [strip_src_off[i], + strip_src_len[i]) of src, is
 * decoded into [strip_dst_off[i], + strip_dst_len[i]) of dst; strip_mode[i] 0 = stored (Compression 1: a copy), 1 = LZW (Compression
 * 5).  All pointers are device pointers, the five tables have nstrips entries, status receives one code per strip.  One wave per
 * strip, two launches (decoded LZW strips up to 16 KB, and up to flair_tiff_lzw_decode_max_strip() = 65 536 bytes, PIL's strip);
 * stored strips have no cap.  Returns -1 for a null pointer, nstrips < 1 or a negative size; no device sync.
 * Stream rules (TIFF 6.0 LZW as libtiff reads it, MSB-first codes, no predictor): a fresh table, next free code nxt = 258, width 9;
 * 256 clears (nxt = 258, width 9, no previous code); 257 ends the stream; the first code after a clear or the start must be a
 * literal; otherwise code < nxt emits its string, code == nxt emits string(old) + first(string(old)), anything larger is an error;
 * after each non-first code string(old) + first(string(code)) becomes entry nxt++ unless nxt is 4096 already; the width grows when
 * the decoder's nxt reaches 511, 1023 and 2047 and stops at 12.  Decoding stops once strip_dst_len bytes are produced: the last
 * string is clipped, the bytes after it are ignored, no EOI is needed.
 * status: 0 exactly strip_dst_len bytes produced; 1 the input ran out first; 2 EOI came first; 3 a non-literal code first after a
 * clear or the start; 4 code > nxt, or code == nxt with a full table; 5 a range or cap error (an offset or length below 0,
 * src_off + src_len > src_bytes, dst_off + dst_len > dst_bytes, dst_len < 1, a mode other than 0 / 1, an LZW dst_len above the
 * cap): nothing of that strip is written.  At status 1 - 4 the bytes decoded before the error are written, the rest of the strip's
 * region is left as it was.
 * Whatever the input bytes are the kernel terminates (every round consumes at least 9 bits of the strip), reads src only inside
 * the strip's own [src_off, src_off + src_len) and writes dst only inside its own [dst_off, dst_off + dst_len). */
int flair_tiff_lzw_decode_max_strip(void);
int flair_tiff_lzw_decode(const uint8_t* src, long src_bytes, const int64_t* strip_src_off, const int32_t* strip_src_len,
                          const int64_t* strip_dst_off, const int32_t* strip_dst_len, const int32_t* strip_mode, long nstrips, uint8_t* dst,
                          long dst_bytes, int32_t* status, void* stream);
/* The read path of zone_detect's input raster (csrc/tiff_read.hip, flair_amd/raster_reader.py): the chunks of a TIFF, its tiles or
 * strips, of any size.  Chunk i, the bytes [src_off[i], + src_len[i]) of src, is decoded as dst_len[i] bytes into the slot
 * scratch + i * slot_bytes; mode[i] 0 = stored, 1 = LZW.  All pointers are device pointers, the four tables and status have nchunks
 * entries, scratch holds nchunks slots and does not overlap src.  One wave per chunk, one launch, no device sync.
 * The stream rules, the status codes 0 - 4 and the clipping of the last string are word for word those of flair_tiff_lzw_decode
 * above.  status 5, a range or cap error: an offset or length below 0, src_off + src_len > src_bytes, dst_len < 1,
 * dst_len > slot_bytes, a mode other than 0 / 1, an LZW dst_len above flair_tiff_lzw_decode_chunks_cap() (16 MiB; stored chunks have
 * no cap): nothing of that slot is written.  At status 1 - 4 the bytes decoded before the error are written, at every status the
 * bytes of a slot from dst_len on are left as they were.
 * Whatever the input bytes are the kernel terminates (every round consumes at least 9 bits of the chunk), reads src only inside the
 * chunk's own [src_off, src_off + src_len) and writes (and reads back) only [0, dst_len) of the chunk's own slot.
 * flair_tiff_lzw_decode_chunks_window(): a code's source bytes less than this far behind the output position at which the code
 *   begins come from the LDS ring of recent output, older ones are read back from the slot (tests place references on both sides).
 * Returns -1 for a null pointer, nchunks < 1, src_bytes < 0 or slot_bytes < 1; -2 unless scratch is 128-byte aligned, slot_bytes a
 * multiple of 128, src_off 8-byte and the int32 tables 4-byte aligned. */
int flair_tiff_lzw_decode_chunks_cap(void);
int flair_tiff_lzw_decode_chunks_window(void);
int flair_tiff_lzw_decode_chunks(const uint8_t* src, long src_bytes, const int64_t* src_off, const int32_t* src_len, const int32_t* dst_len,
                                 const int32_t* mode, long nchunks, uint8_t* scratch, long slot_bytes, int32_t* status, void* stream);
/* The decoded slots into the raster planes (bands, H, W) uint8.  chunks (nchunks, 5) int32 on the device, row i = {x0, y0, width,
 * rows, band0}: slot i holds rows x width pixels of `samples` bytes each, row-major, the samples of a pixel next to each other;
 * sample k of the pixel at (r, x) is written to planes[band0 + k][y0 + r][x0 + x] if y0 + r < H and x0 + x < W and dropped otherwise
 * (TIFF tiles are always full size: edge tiles are clipped on the right and at the bottom).  samples is 1 (PlanarConfiguration 2, or
 * one band) or bands (PlanarConfiguration 1, band0 = 0).  predictor 1: the bytes as they are; 2 (TIFF horizontal differencing): per
 * chunk row and per sample the running sum modulo 256 along the row, starting afresh at the chunk's left edge.
 * A chunk whose status[i] is not 0 is skipped, and so is one with x0, y0 or band0 below 0, width or rows below 1,
 * band0 + samples > bands or width * rows * samples > slot_bytes; nothing else of planes is written.  max_rows: the largest `rows`
 * of the table, which the host knows; it sizes the launch only.
 * Returns -1 for a null pointer, nchunks, slot_bytes, max_rows or an extent < 1, samples other than 1 / bands or a predictor other
 * than 1 / 2; -2 unless chunks and status are 4-byte aligned.  No device sync. */
int flair_tiff_chunks_to_planes(const uint8_t* scratch, long slot_bytes, const int32_t* chunks, const int32_t* status, long nchunks,
                                int max_rows, int samples, int predictor, uint8_t* planes, int bands, int H, int W, void* stream);
/* The same scatter for the chunks of a batch of files (flair_amd/tile_loader.py), each chunk with the layout of its own file: planes
 * (n_planes, H, W) uint8 holds the planes of all files one behind the other, chunks (nchunks, 8) int32 on the device, row i = {x0, y0,
 * width, rows, plane0, samples, predictor, 0}.  Slot i holds rows x width pixels of samples[i] bytes each, row-major, the samples of a
 * pixel next to each other; sample k of the pixel at (r, x) is written to planes[plane0 + k][y0 + r][x0 + x] if y0 + r < H and
 * x0 + x < W and dropped otherwise.  For image b of a (B, bands, H, W) batch the host sets plane0 = b * bands + band0 (samples = bands
 * and band0 = 0 for PlanarConfiguration 1, samples = 1 for PlanarConfiguration 2), for mask b of a (B, H, W) batch plane0 = b and
 * samples = 1.  predictor[i] 1: the bytes as they are; 2: per chunk row and per sample the running sum modulo 256 along the row,
 * starting afresh at the chunk's left edge.  The eighth entry of a row is not read.  One launch takes tiles and strips, both
 * interleaves, both predictors and files that differ in all of them; that a slot came from a stored or an LZW chunk does not show.
 * A chunk whose status[i] is not 0 is skipped, and so is one with x0, y0 or plane0 below 0, width, rows or samples below 1,
 * plane0 + samples > n_planes, a predictor other than 1 / 2 or width * rows * samples > slot_bytes; nothing else of planes is written.
 * max_rows: the largest `rows` of the table, which the host knows; it sizes the launch only.
 * Returns -1 for a null pointer, nchunks, slot_bytes, max_rows, n_planes or an extent < 1; -2 unless chunks and status are 4-byte
 * aligned.  No device sync. */
int flair_tiff_chunks_to_batch(const uint8_t* scratch, long slot_bytes, const int32_t* chunks, const int32_t* status, long nchunks,
                               int max_rows, uint8_t* planes, int n_planes, int H, int W, void* stream);

int flair_sgd_step(float* params, const float* grads, int64_t n, float lr, void* stream);

/* Update rules of the fused trainer over one flat fp32 buffer of n elements (csrc/optim.hip, DESIGN §10 "Optimizers").  One pass
 * each, no atomics, no host sync.  In both rules the gradient enters as g' = g * grad_scale * coef; coef is read from a device float
 * when the pointer is non-NULL (flair_clip_coef writes one), else it is 1.  grads is never written; params and the state buffers are
 * updated in place.  All tensor pointers 16-byte aligned.
 * flair_optim_sgd: torch.optim.SGD's single-tensor rule.  weight_decay != 0: g' += weight_decay * p.  momentum != 0: buf = g' on a
 *   first step (first != 0; the buffer's content is not read), else buf = momentum * buf + (1 - dampening) * g'; then
 *   g' = nesterov ? g' + momentum * buf : buf.  p -= lr * g'.  momentum_buf may be NULL when momentum == 0.  With momentum ==
 *   weight_decay == 0, grad_scale == 1 and coef == NULL the result is flair_sgd_step's to the bit.
 * flair_optim_adamw: torch.optim.AdamW's single-tensor rule (decoupled decay, no amsgrad, no maximize): m += (g' - m)(1 - beta1),
 *   v = beta2 v + (1 - beta2) g'^2, p = p (1 - lr weight_decay) - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).  bc1 = 1 - beta1^t and
 *   bc2 = 1 - beta2^t come from the host.  first != 0 takes m and v as zero whatever the buffers hold.
 * flair_grad_sqnorm: *sum = (accumulate ? *sum : 0) + sum of g^2, in fp64.  A grid that depends on n alone writes one fp64 partial
 *   per block into `partials` (flair_grad_sqnorm_partials() doubles), one block adds them in index order: the same bits every run.
 * flair_clip_coef: *norm = (float)(sqrt(*sum) * grad_scale), *coef = min(1, max_norm / (*norm + 1e-6)) -- clip_grad_norm_'s rule.
 * Returns -1 for a NULL required pointer or n < 0; -2 for a misaligned pointer, nesterov with momentum == 0 or dampening != 0, a
 * negative lr / momentum / weight_decay / eps, a beta outside [0, 1), bc1 or bc2 <= 0, max_norm or grad_scale <= 0.  Nothing is
 * launched then. */
int flair_optim_sgd(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                    float weight_decay, int nesterov, int first, float grad_scale, const float* coef, void* stream);
int flair_optim_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float bc1, float bc2, int first, float grad_scale, const float* coef, void* stream);
int flair_grad_sqnorm_partials(void);
int flair_grad_sqnorm(const float* grads, int64_t n, double* partials, double* sum, int accumulate, void* stream);
int flair_clip_coef(const double* sum, float grad_scale, float max_norm, float* norm, float* coef, void* stream);
/* feats[-1] += x_enc.unsqueeze(1).unsqueeze(-1).repeat(1,512,1,16) — model.py:59-60: x (N,C,H,W) += v (N,H). */
int flair_add_rowvec_nchw(float* x, const float* v, int N, int C, int H, int W, void* stream);
/* The same add, in place, on an NHWC tensor of the compute dtype (the layout the executor keeps its features in):
 * x (N,H,W,C) += v (N,H) fp32, summed in fp32 and rounded to `dtype` once.  C must be a multiple of 8 and x 16-byte aligned (-2). */
int flair_add_rowvec_nhwc(int dtype, void* x, const float* v, int N, int H, int W, int C, void* stream);
/* The same add out of place: y (N,H,W,C) = dtype(float(x) + v (N,H)).  What a training forward needs, where x — the ReLU output of the
 * unit that produced it, the mask source of that unit's backward — must stay as it is.  Same arithmetic, chunking and refusals as
 * flair_add_rowvec_nhwc (both tensors 16-byte aligned); x == y is allowed and is that function. */
int flair_add_rowvec_nhwc_to(int dtype, const void* x, const float* v, void* y, int N, int H, int W, int C, void* stream);
/* The gradient of either add with respect to v: dv (N,H) fp32 = sum over w and c of dx (N,H,W,C).  Accumulated in fp32 in one fixed
 * order (one workgroup per row, no atomics): the same bits on every call.  Same refusals as flair_add_rowvec_nhwc. */
int flair_rowvec_grad_nhwc(int dtype, const void* dx, float* dv, int N, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Operator-level entry points (unit parity tests; same kernels the model object launches).
 * Activations NHWC in `dtype`; weights PyTorch OIHW fp32. */
size_t flair_conv2d_workspace_bytes(int dtype, int N, int H, int W, int C0, int C1, int up0, int Cout, int R,
                                    int stride, int pad);
/* y = conv2d(cat([up2(x0)?, x1]), w) (+bias); optional fp32 NCHW copy; optional BN batch statistics
 * (sum, sum of squares per channel, reduced) into stats[2][Cout]. */
int flair_conv2d_forward(int dtype, const void* x0, const void* x1, int N, int H, int W, int C0, int C1, int up0,
                         const float* w_oihw, const float* bias, int Cout, int R, int stride, int pad, void* y_nhwc,
                         float* y_nchw, float* stats, void* workspace, size_t workspace_bytes, void* stream);
/* dx = conv2d_backward_data(dy, w); dw = conv2d_backward_weight(x, dy) */
int flair_conv2d_backward(int dtype, const void* x0, int N, int H, int W, int Cin, const float* w_oihw, int Cout, int R,
                          int stride, int pad, const void* dy_nhwc, void* dx_nhwc, float* dw_oihw, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The fused forms of the two launchers above, as the network launches them: every option is a field of a plain struct
 * (zero / NULL = off) that is copied into the launcher's arguments; no kernel differs.  The return value is the launcher's own:
 * -6 where the kernel chosen for the shape does not implement a requested option.
 * flair_conv2d_ex, mode 0: the forward of flair_conv2d_forward.  mode 1: the stride-1 data gradient — x0 is dy with C0 channels,
 *   w_oihw the FORWARD layer's weights [C0][Cout][R][R], `pad` the forward padding, the output has Cout channels.
 *   in_scale / in_shift [C0 + C1]: the input is relu(x * in_scale[c] + in_shift[c]) inside the image, zero in the padding.
 *   oscale / oshift [Cout], ores (NHWC, as y_nhwc), orelu: y = [relu](acc * oscale + oshift (+ bias) (+ ores)).
 *   accumulate: y_nhwc += result; with acc_src the addend is read from acc_src (NHWC, as y_nhwc) instead of y_nhwc.
 *   pool_c0 > 0: output columns [0, pool_c0) are 2x2 sum-pooled into y_nhwc ([N][Ho/2][Wo/2][out_ld]), columns [pool_c0, Cout)
 *     go to out_skip ([N][Ho][Wo][out_skip_ld]; += with skip_accumulate) — the backward of "nearest x2 upsample ++ skip".
 *   out_ld: row stride of y_nhwc in elements (0 = Cout).  preds_u8 [N][Ho][Wo]: first argmax over the Cout outputs of a pixel,
 *     maxprob_f32 its softmax probability; y_nhwc may then be NULL.
 *   stats [2][Cout] as in flair_conv2d_forward.
 * flair_conv2d_wgrad_ex: dw[Cout][Cin_real][R][R] (+= with accumulate) of the convolution over cat([up2(x0)?, x1]) (H, W: extent
 *   of x0 as stored), lazy input as above, dy rows of dy_ld elements (0 = Cout), Cin_real = 0: C0 + C1.  dbias [Cout]: the column
 *   sums of dy from the same kernel (16 -> <= 16 channel layers with dy_ld == 16; -6 elsewhere).  cus: workgroup budget of the
 *   register-resident kernel (0 = default).
 *   bnr_partial: the fused first pass of the BatchNorm backward of the unit that produced this data gradient's target (halo-tile
 *     kernels, mode 1): y_nhwc (the pooled part with pool_c0) is the complete gradient dz; bnr_y is that unit's pre-BN tensor (shape
 *     and row stride of y_nhwc), m = [bnr_y * bnr_scale[c] + bnr_shift[c] > 0], or [bnr_out > 0] with bnr_out (NHWC, as y_nhwc).
 *     The kernel leaves sum(dz * m) and sum(dz * m * y) per row block in the caller's bnr_partial[2][out_ld][rows], rows =
 *     flair_conv2d_ex_grid_rows() of the same struct; bnr_rows is the capacity of the buffer in row blocks (-100 when too small).
 *     bnr_mask: store dz * m instead of dz (halo-GEMM only).
 *   mode 2: the stride-2 data gradient by output parity class, as the network's backward pass launches it.  x0 is dy [N][H][W][C0],
 *     w_oihw the FORWARD layer's [C0][Cout][R][R], y_nhwc is dx [N][2H][2W][out_ld].  R = 3, pad = 1: the four classes (1, 2, 2 and 4
 *     taps) in one launch, their weights packed by the network's own class descriptors; R = 1, pad = 0: the (even, even) pixels
 *     only (the network uses it with accumulate).  Any other geometry: -6.
 * Workspace: the _workspace_bytes call on the same struct (under the same flair_tune_set settings). */
typedef struct flair_conv_ex {
  int dtype, mode;
  const void* x0; const void* x1;
  int N, H, W, C0, C1, up0;
  const float* w_oihw; const float* bias;
  int Cout, R, stride, pad;
  void* y_nhwc; int out_ld;
  float* y_nchw; float* stats;
  const float* in_scale; const float* in_shift;
  const float* oscale; const float* oshift; const void* ores; int orelu;
  int accumulate; const void* acc_src;
  int pool_c0; void* out_skip; int out_skip_ld; int skip_accumulate;
  uint8_t* preds_u8; float* maxprob_f32;
  int ogelu;   /* y = gelu_erf(acc (+ bias)) before ores / orelu: the gather-form GEMM only (-6 elsewhere) */
  const void* bnr_y; const void* bnr_out; const float* bnr_scale; const float* bnr_shift;
  float* bnr_partial; int bnr_rows; int bnr_mask;
} flair_conv_ex_t;
typedef struct flair_wgrad_ex {
  int dtype;
  const void* x0; const void* x1;
  int N, H, W, C0, C1, up0;
  const void* dy; int dy_ld;
  int Cout, R, stride, pad;
  float* dw; int Cin_real; int accumulate;
  const float* in_scale; const float* in_shift;
  float* dbias; int cus;
  /* the stem's weight-gradient kernel only (-6 elsewhere): dy is the gradient w.r.t. the unit's ReLU output and the kernel stages
   * k1 * dz + k2 * y + k3, dz = dy * [fuse_y * fuse_msc + fuse_msh > 0], fuse_coef = k1 | k2 | k3 (Cout floats each) */
  const void* fuse_y; const float* fuse_coef; const float* fuse_msc; const float* fuse_msh;
} flair_wgrad_ex_t;
size_t flair_conv2d_ex_workspace_bytes(const flair_conv_ex_t* p);
int flair_conv2d_ex(const flair_conv_ex_t* p, void* workspace, size_t workspace_bytes, void* stream);
/* row blocks of the launch flair_conv2d_ex makes for this struct (= rows of stats / bnr_partial); bnr_y set counts as a request
 * for the fused reduction even while bnr_partial is still NULL.  Negative: the struct is refused. */
int flair_conv2d_ex_grid_rows(const flair_conv_ex_t* p);
size_t flair_conv2d_wgrad_ex_workspace_bytes(const flair_wgrad_ex_t* p);
int flair_conv2d_wgrad_ex(const flair_wgrad_ex_t* p, void* workspace, size_t workspace_bytes, void* stream);
/* workspace of flair_bn_relu_forward / _backward for `rows` rows of C channels */
size_t flair_bn_workspace_bytes(int64_t rows, int C);
int flair_bn_relu_forward(int dtype, const void* y, int64_t rows, int C, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int training, const void* residual, int relu,
                          void* out, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                          void* stream);
int flair_bn_relu_backward(int dtype, const void* dout, const void* out, const void* y, int64_t rows, int C,
                           const float* gamma, const float* save_mean, const float* save_invstd, int relu, void* dy,
                           void* dres, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                           void* stream);
/* bn_backward with every argument the network sets.  pre_nblk > 0: `partial` [2][C][pre_nblk] is the caller's and already holds
 * that many producer-side block sums (flair_conv2d_ex bnr_partial, flair_maxpool_backward_ex); premasked: dout is dz already.
 * pre_nblk == 0: the reduction runs here on workspace (flair_bn_workspace_bytes), mask from `out` (> 0), else from
 * y * mscale + mshift > 0, else none.  dgamma / dbeta (+= with accumulate_param), dy = k1 dz + k2 y + k3, dres (+)= dz;
 * dy == dres == NULL: coefficients only.  coef (optional) receives k1 | k2 | k3, 3 * C floats. */
typedef struct flair_bn_bwd_ex {
  int dtype;
  const void* dout; const void* out; const void* y;
  const float* mean; const float* invstd; const float* gamma;
  int64_t rows; int C;
  float* partial; int pre_nblk; int premasked;
  const float* mscale; const float* mshift;
  float* dgamma; float* dbeta; int accumulate_param;
  void* dy; void* dres; int dres_accumulate;
  float* coef;
} flair_bn_bwd_ex_t;
int flair_bn_backward_ex(const flair_bn_bwd_ex_t* p, void* workspace, size_t workspace_bytes, void* stream);
/* The fused backward of a 3x3 / stride-1 / pad-1 convolution with 16 input and <= 16 output channels, bf16 (csrc/bwd_halo16.hip),
 * as the network launches it for the segmentation head and decoder block 4's second convolution: one kernel for the data gradient
 * with the BatchNorm-backward sums of the unit that produced the layer input, the weight gradient and (head flavour) the bias
 * gradient.  All tensors NHWC bf16, 16 channels.
 *   g: the output gradient [N][H][W][16].  gy != NULL (unit flavour): g is the gradient w.r.t. the unit's ReLU output, gy the unit's
 *     pre-BatchNorm tensor, and the kernel forms dy = k1 dz + k2 y + k3, dz = g * [gy * gmsc + gmsh > 0], gcoef = k1 | k2 | k3.
 *   x: the producing unit's pre-BatchNorm tensor; the layer input is relu(x * in_scale + in_shift).
 *   w_oihw: the forward layer's [Cout][16][3][3]; dx [N][H][W][16]; dw [Cout][16][3][3]; dbias [Cout] (optional, head flavour).
 *   bnr_partial [2][16][rows], rows = flair_bwd16_ex_grid_rows(): sum(dx * m), sum(dx * m * x), m = [x * bnr_scale + bnr_shift > 0].
 * -2: H % 8 or W % 32; -100: workspace or bnr_rows too small. */
typedef struct flair_bwd16_ex {
  const void* g; const void* gy; const float* gcoef; const float* gmsc; const float* gmsh;
  const void* x; const float* in_scale; const float* in_shift;
  const float* w_oihw; int Cout;
  int N, H, W;
  void* dx;
  const float* bnr_scale; const float* bnr_shift; float* bnr_partial; int bnr_rows;
  float* dw; float* dbias;
} flair_bwd16_ex_t;
size_t flair_bwd16_ex_workspace_bytes(const flair_bwd16_ex_t* p);
int flair_bwd16_ex_grid_rows(const flair_bwd16_ex_t* p);   /* workgroups of the launch under the current flair_tune_set settings */
int flair_bwd16_ex(const flair_bwd16_ex_t* p, void* workspace, size_t workspace_bytes, void* stream);
int flair_maxpool_forward(int dtype, const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int flair_maxpool_backward(int dtype, const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C,
                           void* stream);
/* dx (+= with accumulate); bnr_partial [2][C][N * H]: per input row, sum(dx * m) and sum(dx * m * bnr_y), m = [bnr_y * bnr_msc +
 * bnr_msh > 0], of the stored dx (the stem's BatchNorm-backward reduction) */
int flair_maxpool_backward_ex(int dtype, const void* dy, const uint8_t* idx, void* dx, int accumulate, int N, int H, int W, int C,
                              const void* bnr_y, const float* bnr_msc, const float* bnr_msh, float* bnr_partial, void* stream);
int flair_bn_act(int dtype, const void* y, const float* scale, const float* shift, void* out, int64_t rows, int C, int relu,
                 void* stream);   /* out = [relu](y * scale[c] + shift[c]) */
/* act = relu(y * scale + shift) [N][H][W][C] and its 3x3 / stride-2 max pool out, idx [N][H/2][W/2][C] in one pass */
int flair_bn_act_maxpool(int dtype, const void* y, const float* scale, const float* shift, void* act, void* out, uint8_t* idx, int N,
                         int H, int W, int C, void* stream);
/* backward of cat([up2(x0), skip]): dcat [N][H][W][C0 + C1] -> dx0 [N][H/2][W/2][C0] (2x2 sums), dskip [N][H][W][C1] */
int flair_upcat_bwd(int dtype, const void* dcat, void* dx0, int dx0_accumulate, void* dskip, int dskip_accumulate, int N, int H, int W,
                    int C0, int C1, void* stream);
int flair_ew_add(int dtype, void* dst, const void* src, int64_t n, void* stream);   /* dst += src, n elements */
/* out[c] = sum over rows of x[rows][ld], c < C; workspace: flair_bn_workspace_bytes(rows, ld) */
int flair_colsum(int dtype, const void* x, int64_t rows, int ld, int C, float* out, void* workspace, size_t workspace_bytes,
                 void* stream);
/* pack_weights_all: n (<= 64) fp32 OIHW masters at params + w_off -> packed copies at base + dst_off (bytes) in one launch.
 * tf = 0: dst[k][tap * Cin_p + c] = w[k][c][r][s]; tf = 1: dst[c][tap * Cin_p + k] = w[k][c][R-1-r][S-1-s]; rows_pad x Kpad
 * elements, everything outside the real region zero.  Rc > 0: packed tap (ri, si), ri < Rc, si < Sc, is tap (r0 + ri * rstep,
 * s0 + si * sstep) of the full pack.  In bf16 the 3x3 packs whose channel counts allow it (tf = 0: Cin % 4 == 0 and no tap
 * subset; tf = 1: Cin % 32 == 0 and Cout % 32 == 0) read their master 16 bytes at a time: params 16-byte aligned and
 * w_off % 4 == 0, else -2. */
typedef struct flair_pack_desc {
  int64_t w_off; uint64_t dst_off;
  int Cout, Cin, R, S, Cin_p, rows_pad, Kpad, tf;
  int r0, rstep, Rc, s0, sstep, Sc;
} flair_pack_desc_t;
int flair_pack_weights(int dtype, const float* params, const flair_pack_desc_t* descs, int n, void* base, void* stream);
/* pack_weight, the single-layer packer of the operator entry points above: the same layout (no tap subsets) into
 * dst[rows_pad][Kpad]. */
int flair_pack_weight(int dtype, const float* w_oihw, void* dst, int Cout, int Cin, int R, int S, int Cin_p, int rows_pad, int Kpad,
                      int tf, void* stream);
int flair_nchw_to_nhwc(int dtype, const float* x_nchw, void* y_nhwc, int N, int C, int H, int W, int Cpad, void* stream);
int flair_nhwc_to_nchw(int dtype, const void* x_nhwc, float* y_nchw, int N, int C, int H, int W, int Cpad, void* stream);

/* The SegFormer / UperNet-Swin kernels one at a time, as the two executors launch them (csrc/segformer_ops.h, csrc/swin_ops.h
 * say what each computes).  All pointers are device pointers; activations token-major NHWC in `dtype`, parameters fp32 unless
 * noted; the return value is the launcher's own (-2: a shape the kernel does not take).  The _ok predicates return 0 / 1. */
int flair_sf_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int C, float eps,
                       void* stream);
int flair_sf_dwconv3x3_gelu(int dtype, const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C,
                            void* stream);
int flair_sf_bilinear_nhwc(int dtype, const void* x, void* y, int B, int h, int w, int C, int H, int W, int ld, void* stream);
int flair_sf_bilinear_nchw_f32(const float* x, float* y, int64_t planes, int h, int w, int H, int W, void* stream);
int flair_sf_slice_cols(int dtype, const float* src, int ld, int col0, int ncols, int64_t rows, void* dst, void* stream);
int flair_sf_fuse_bias(const float* wf, int D, const float* b3, const float* b2, const float* b1, const float* b0,
                       const float* scale, const float* shift, float* shift2, void* stream);
int flair_sf_upsample_sum_bn_relu(int dtype, const void* g0, const void* g1, const void* g2, const void* g3, const float* scale,
                                  const float* shift2, void* z, int B, int H, int W, int D, void* stream);
int flair_sf_ffn_fused_ok(int dtype, int C, int H, int W);
int flair_sf_ffn_dw_pack(const float* w, const float* b, float* out, int nch, void* stream);
/* x / out / out_ln bf16 [B][H][W][C]; w1 [4C][C], w2 [C][4C] bf16 row-major; dwp from flair_sf_ffn_dw_pack */
int flair_sf_ffn_fused(const void* x, const float* ln_g, const float* ln_b, const void* w1, const float* b1, const float* dwp,
                       const void* w2, const float* b2, void* out, int B, int H, int W, int C, float eps, const float* ln2_g,
                       const float* ln2_b, void* out_ln, void* stream);
int flair_sf_head_fused_ok(int dtype, int H, int W, int C0, int D, int labels);
int flair_sf_head_wint(void* wint_bf16_128x96, void* stream);
/* f0 [B][H][W][64], w0 [D][64], g1..g3 [B][H >> i][W >> i][D], wint, wc [32][D] (rows >= labels zero): bf16; out fp32 NCHW */
int flair_sf_head_fused(const void* f0, const void* w0, const void* g1, const void* g2, const void* g3, const void* wint,
                        const float* scale, const float* shift2, const void* wc, const float* bc, float* out, int B, int H, int W,
                        int D, int labels, void* stream);
int flair_sf_attention(int dtype, const void* q, const void* k, const void* v, void* out, int B, int N, int Nk, int hidden,
                       int kv_ld, void* stream);
int flair_swin_window_attention(int dtype, const void* qkv, const float* qkv_bias, const float* table, void* out, int B, int H,
                                int W, int C, int heads, int shift, void* stream);
int flair_swin_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int C, int ld,
                         float eps, void* stream);
int flair_swin_patch_merge_ln(int dtype, const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C,
                              float eps, void* stream);
int flair_swin_adaptive_avgpool(int dtype, const void* x, int ld, void* y, int B, int h, int w, int C, int S, void* stream);
int flair_swin_bilinear_add(int dtype, const void* x, void* y, int B, int h, int w, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MetadataMLP (replaces /root/reference/src/flair/model.py:74-96, called at model.py:58): Linear(45,64) -> Dropout(0.4) ->
 * ReLU -> Linear(64,32) -> Dropout -> ReLU -> Linear(32,16) -> Dropout -> ReLU.  x [B][45] fp32; w[i] / b[i] the three
 * nn.Linear weights ([out][in]) and biases; mask[i] optional [B][64|32|16] dropout masks ALREADY scaled by 1/(1-p)
 * (NULL array or NULL entries: eval mode); h1 [B][64], h2 [B][32] receive the hidden activations (needed by backward,
 * may be NULL); out [B][16].  backward: dout [B][16] -> dw[i] / db[i] (overwritten); scratch >= B*112 floats; B <= 256.
 * The metadata vector is a model input: no gradient w.r.t. x is produced (the reference never asks for one). */
int flair_metadata_mlp_forward(const float* x, const float* const w[3], const float* const b[3], const float* const mask[3],
                               float* h1, float* h2, float* out, int B, void* stream);
int flair_metadata_mlp_backward(const float* x, const float* h1, const float* h2, const float* out, const float* const w[3],
                                const float* const mask[3], const float* dout, int B, float* const dw[3], float* const db[3],
                                float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement aid (bench.py "roofline"): while enabled every kernel launch of the library is bracketed by
 * HIP events on its launch stream.  stop() synchronises the device and returns the number of distinct
 * kernels; kernel(i) gives total time, launch count and the ALGORITHMIC flops / bytes of those launches. */
int flair_profile_start(int max_records);
int flair_profile_stop(void);
int flair_profile_kernel(int i, char* name, int name_cap, double* total_ms, int64_t* launches, double* flops,
                         double* bytes);

/* ------------------------------------------------------------------------------------------------
 * SegFormer (MiT encoder + all-MLP decode head), inference only: the HuggingFace provider of zone_detect —
 * /root/reference/src/zone_detect/model.py:42-50 (AutoModelForSemanticSegmentation.from_pretrained) and
 * compare.py:31-36 (`model(imgs).logits`); BASELINE config 5 names SegFormer-MiT-B2 with 5 input channels.
 * Replaces transformers' SegformerForSemanticSegmentation.forward in eval mode.  Tensor names / shapes
 * (flair_segformer_tensor_info) are that library's state_dict keys; every tensor, BatchNorm running
 * statistics included (kind 1), lives in ONE flat fp32 buffer.  Geometry: MiT-B1..B5 (heads of 64 channels,
 * reduction ratios 8/4/2/1); H, W multiples of 32 with (H/32)*(W/32) a multiple of 16 and <= 256. */
typedef struct flair_segformer flair_segformer_t;
int flair_segformer_create(flair_segformer_t** out, int in_channels, int num_labels, const int depths[4],
                           const int hidden_sizes[4], const int num_heads[4], const int sr_ratios[4],
                           int decoder_hidden_size, int dtype);
void flair_segformer_destroy(flair_segformer_t* h);
int64_t flair_segformer_param_count(const flair_segformer_t* h);
int flair_segformer_num_tensors(const flair_segformer_t* h);
int flair_segformer_tensor_info(const flair_segformer_t* h, int i, char* name, int name_cap, int64_t shape[4], int* ndim,
                                int64_t* offset, int* kind);
int64_t flair_segformer_workspace_bytes(flair_segformer_t* h, int B, int H, int W);
/* The forward keeps what depends on the weights alone (packed GEMM operands, folded BatchNorm, the decode head's
 * pre-multiplied matrices) at the front of the workspace and reuses it while `params` and `workspace` are the
 * same pointers as in the previous call.  Call this after changing the parameter buffer's CONTENTS in place
 * (transformers has no counterpart: its modules read their weights on every call). */
void flair_segformer_weights_changed(flair_segformer_t* h);
/* logits_quarter_nchw: fp32 (B, labels, H/4, W/4) = the library's `.logits`; logits_full_nchw: the same after
 * nn.functional.interpolate(size=(H, W), mode="bilinear", align_corners=False), what softmax / margin crop /
 * convert (compare.py:35, 69-82) need at tile resolution.  Either may be NULL, not both. */
int flair_segformer_forward(flair_segformer_t* h, const float* params, const float* x_nchw, float* logits_quarter_nchw,
                            float* logits_full_nchw, int B, int H, int W, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * UperNet with a Swin backbone (upernet-swin-tiny / -small), inference only: the HuggingFace provider's default model
 * (`openmmlab/upernet-swin-small` in the reference's configs).  Replaces transformers' UperNetForSemanticSegmentation.forward
 * in eval mode; the auxiliary head's tensors are in the table and are never computed.  Tensor names / shapes
 * (flair_upernet_tensor_info) are that library's state_dict keys (transformers 5.x names); every tensor, BatchNorm running
 * statistics included (kind 1), lives in ONE flat fp32 buffer.  Geometry: window 7, heads of 32 channels; H, W multiples of
 * 32 from 64 to 2048 (other sizes: -14). */
typedef struct flair_upernet flair_upernet_t;
int flair_upernet_create(flair_upernet_t** out, int in_channels, int num_labels, int embed_dim, const int depths[4],
                         const int num_heads[4], int window_size, int hidden_size, const int pool_scales[4],
                         int auxiliary_in_channels, int auxiliary_channels, int dtype);
void flair_upernet_destroy(flair_upernet_t* h);
int64_t flair_upernet_param_count(const flair_upernet_t* h);
int flair_upernet_num_tensors(const flair_upernet_t* h);
int flair_upernet_tensor_info(const flair_upernet_t* h, int i, char* name, int name_cap, int64_t shape[4], int* ndim,
                              int64_t* offset, int* kind);
int64_t flair_upernet_workspace_bytes(flair_upernet_t* h, int B, int H, int W);
/* as flair_segformer_weights_changed: the packed weights and folded BatchNorm at the front of the workspace are reused
 * while `params` and `workspace` are the same pointers; call this after changing the parameter buffer's contents in place */
void flair_upernet_weights_changed(flair_upernet_t* h);
/* logits_nchw: fp32 (B, labels, H, W) = the library's `.logits` (already resized to the input size) */
int flair_upernet_forward(flair_upernet_t* h, const float* params, const float* x_nchw, float* logits_nchw, int B, int H, int W,
                          void* workspace, size_t workspace_bytes, void* stream);
/* logits_quarter_nchw: fp32 (B, labels, H/4, W/4), the classifier's output before the resize to the input size (what the _q4
 * zone_detect functions consume); the same passes through the same workspace as flair_upernet_forward.  H % 4 or W % 4: -2. */
int flair_upernet_forward_quarter(flair_upernet_t* h, const float* params, const float* x_nchw, float* logits_quarter_nchw, int B, int H,
                                  int W, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic tuning switch (kernel-variant A/B timing inside one process; keys are the FLAIR_* environment
 * variables DESIGN.md lists, the environment supplies the default).  Returns 0. */
int flair_tune_set(const char* key, int value);
/* Diagnostic: device buffer of [workgroups][8] uint64 that the next halo-GEMM launches fill with s_memtime stamps
 * (kernel start, main loop start, main loop end, accumulators staged, stored; + 100 MHz real-time start / end); NULL
 * switches it off.  Only the diagnostic build (FLAIR_STAMPS=1 python flair-1_amd/build.py) contains the stamps: the shipped
 * library returns -7 and its kernels execute none. */
int flair_debug_buffer(void* device_u64);

#ifdef __cplusplus
}
#endif
#endif /* FLAIR_HIP_H */
