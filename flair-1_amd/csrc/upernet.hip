// Native inference executor for transformers' UperNetForSemanticSegmentation with a SwinBackbone (upernet-swin-tiny / -small),
// the HuggingFace provider's default model in the reference's configs.  Eval mode only.  The algorithm is the library's published
// one (modeling_swin.py / modeling_upernet.py of transformers 5.15):
//   backbone: 4x4 stride-4 patch embedding + LayerNorm; per stage, Swin blocks (LayerNorm, window attention over 7 x 7 windows of
//   the grid padded to multiples of 7 AFTER the norm, cyclic shift by -3 on odd blocks with the -100 region mask, relative-position
//   bias; residual; LayerNorm, fc1, erf-GELU, fc2; residual), then patch merging (2 x 2 gather, LayerNorm(4C), Linear 4C -> 2C).
//   SwinBackbone partitions always (no window clamping on small grids) and returns every stage's state BEFORE its downsampling
//   through hidden_states_norms.
//   head: lateral 1x1 conv + BatchNorm + ReLU on stages 1-3; pyramid pooling on stage 4 (adaptive average pools 1, 2, 3, 6, 1x1
//   conv + BN + ReLU, bilinear back) and a 3x3 bottleneck over the concatenation; top-down path lat[i-1] += up(lat[i]); 3x3 FPN
//   convs on levels 0-2; every level resized to level 0 and concatenated; 3x3 fpn_bottleneck; 1x1 classifier; bilinear to the
//   input size.  The auxiliary head's tensors are in the table (they load) and are never computed.
// Parameter names and shapes are that library's state_dict keys.  Matrix products run on conv_igemm.hip / conv_hg.hip with their
// fused epilogues (bias, residual, erf-GELU, folded BatchNorm + ReLU, fp32 NCHW logits); the rest is swin_ops.hip.
#include "upernet.h"

#include "segformer_ops.h"
#include "swin_ops.h"

namespace flair {

int UperNet::add_cbn(const std::string& name, int cin, int cout, int k) {
  UpConvBn c;
  c.conv = add_lin(name + ".conv#conv", cin, cout, k, 1, k / 2, false);
  c.g = add_tensor(name + ".batch_norm.weight", 1, cout, 1, 1, 1, 0);
  c.b = add_tensor(name + ".batch_norm.bias", 1, cout, 1, 1, 1, 0);
  c.rm = add_tensor(name + ".batch_norm.running_mean", 1, cout, 1, 1, 1, 1);
  c.rv = add_tensor(name + ".batch_norm.running_var", 1, cout, 1, 1, 1, 1);
  cbs.push_back(c);
  return (int)cbs.size() - 1;
}

UperNet::UperNet(int in_ch, int labels, int embed, const int* depths_, const int* heads_, int hidden_, const int* pool_scales_, int aux_in,
                 int aux_channels, int dt)
    : TfExec(dt), in_channels(in_ch), num_labels(labels), embed_dim(embed), hidden(hidden_) {
  for (int i = 0; i < 4; ++i) {
    depths[i] = depths_[i]; heads[i] = heads_[i]; pool_scales[i] = pool_scales_[i]; dims[i] = embed << i;
  }
  patch = add_lin("backbone.swin.embeddings.patch_embeddings.projection#conv", in_ch, embed, 4, 4, 0, true);
  patch_ln = add_ln("backbone.swin.embeddings.norm", embed);
  for (int i = 0; i < 4; ++i) {
    const std::string st = "backbone.swin.encoder.layers." + std::to_string(i);
    const int C = dims[i];
    SwStage S;
    for (int b = 0; b < depths[i]; ++b) {
      const std::string bl = st + ".blocks." + std::to_string(b) + ".";
      SwBlock K;
      K.qw = add_tensor(bl + "attention.q_proj.weight", 2, C, C, 1, 1, 0);
      K.qb = add_tensor(bl + "attention.q_proj.bias", 1, C, 1, 1, 1, 0);
      K.kw = add_tensor(bl + "attention.k_proj.weight", 2, C, C, 1, 1, 0);
      K.kb = add_tensor(bl + "attention.k_proj.bias", 1, C, 1, 1, 1, 0);
      K.vw = add_tensor(bl + "attention.v_proj.weight", 2, C, C, 1, 1, 0);
      K.vb = add_tensor(bl + "attention.v_proj.bias", 1, C, 1, 1, 1, 0);
      K.o = add_lin(bl + "attention.o_proj", C, C, 1, 1, 0, true);
      K.table = add_tensor(bl + "attention.relative_position_bias.relative_position_bias_table", 2, 13 * 13, heads[i], 1, 1, 0);
      K.ln1 = add_ln(bl + "layernorm_before", C);
      K.ln2 = add_ln(bl + "layernorm_after", C);
      K.fc1 = add_lin(bl + "mlp.fc1", C, 4 * C, 1, 1, 0, true);
      K.fc2 = add_lin(bl + "mlp.fc2", 4 * C, C, 1, 1, 0, true);
      S.blocks.push_back(K);
    }
    if (i < 3) {
      S.reduction = add_lin(st + ".downsample.reduction", 4 * C, 2 * C, 1, 1, 0, false);
      S.merge_ln = add_ln(st + ".downsample.norm", 4 * C);
    }
    stages.push_back(S);
  }
  add_ln("backbone.swin.layernorm", dims[3]);   // SwinModel's final norm: in the state dict, not on the backbone's outputs
  for (int i = 0; i < 4; ++i) hs_norm[i] = add_ln("backbone.hidden_states_norms.stage" + std::to_string(i + 1), dims[i]);
  cls = add_lin("decode_head.classifier#conv", hidden, labels, 1, 1, 0, true);
  for (int j = 0; j < 4; ++j) psp[j] = add_cbn("decode_head.psp_modules." + std::to_string(j) + ".1", dims[3], hidden, 1);
  bottleneck = add_cbn("decode_head.bottleneck", dims[3] + 4 * hidden, hidden, 3);
  for (int i = 0; i < 3; ++i) lateral[i] = add_cbn("decode_head.lateral_convs." + std::to_string(i), dims[i], hidden, 1);
  for (int i = 0; i < 3; ++i) fpn[i] = add_cbn("decode_head.fpn_convs." + std::to_string(i), hidden, hidden, 3);
  fpn_bottleneck = add_cbn("decode_head.fpn_bottleneck", 4 * hidden, hidden, 3);
  // auxiliary FCN head: loaded, never computed (its output is not `.logits`)
  add_tensor("auxiliary_head.convs.0.conv.weight", 4, aux_channels, aux_in, 3, 3, 0);
  add_tensor("auxiliary_head.convs.0.batch_norm.weight", 1, aux_channels, 1, 1, 1, 0);
  add_tensor("auxiliary_head.convs.0.batch_norm.bias", 1, aux_channels, 1, 1, 1, 0);
  add_tensor("auxiliary_head.convs.0.batch_norm.running_mean", 1, aux_channels, 1, 1, 1, 1);
  add_tensor("auxiliary_head.convs.0.batch_norm.running_var", 1, aux_channels, 1, 1, 1, 1);
  add_tensor("auxiliary_head.classifier.weight", 4, labels, aux_channels, 1, 1, 0);
  add_tensor("auxiliary_head.classifier.bias", 1, labels, 1, 1, 1, 0);
}

bool UperNet::shape_ok(int H, int W) { return H >= 64 && W >= 64 && H <= 2048 && W <= 2048 && H % 32 == 0 && W % 32 == 0; }

// the largest tensors of one image: the FPN concatenation (H / 4)(W / 4) x 4 hidden and the stage-1 MLP (H / 4)(W / 4) x 4 embed;
// the kernels index elements with 32-bit arithmetic
int UperNet::max_batch(int H, int W) const {
  const long per = (long)(H / 4) * (W / 4) * 4 * (hidden > embed_dim ? hidden : embed_dim) + (long)(H / 32) * (W / 32) * (dims[3] + 4 * hidden);
  const long n = ((1L << 31) - 1) / per;
  return (int)(n < 1 ? 1 : n > 1024 ? 1024 : n);
}

void UperNet::conv_bn_relu(int i, const void* in, int B, int Hin, int Win, void* out, int out_ld) {
  gemm(lins[cbs[i].conv], in, B, Hin, Win, out, out_ld, nullptr, bn_sc_[i], bn_sh_[i], 1, nullptr);
}

void UperNet::layernorm(const SfNorm& n, const void* x, void* y, long rows, int ld) {
  RUN(swin_layernorm(dtype, x, params_ + n.g_off, params_ + n.b_off, y, rows, n.C, ld, 1e-5f, s_));
}

int UperNet::run(const float* params, const float* x_nchw, float* logits, int B, int H, int W, void* ws, size_t ws_bytes, hipStream_t s,
                 bool dry, bool quarter) {
  if (!shape_ok(H, W)) return -10;
  const size_t es = dtype_size(dtype);
  // ---- what depends on the weights alone (packed operands, fused q / k / v, folded BatchNorm) sits at the front of the arena
  // at shape-independent offsets and is rebuilt only when the parameter buffer or the workspace changes, or after weights_changed()
  const bool fresh = begin(params, ws, ws_bytes, s, dry, 0);
  pack_lins(fresh);
  // q, k and v of a block as ONE product over [q_proj.weight; k_proj.weight; v_proj.weight] (3C rows) with the concatenated bias
  qkv_w_.clear(); qkv_b_.clear();
  for (int si = 0; si < 4; ++si)
    for (const SwBlock& K : stages[si].blocks) {
      const SfPart qkv[3] = {{K.qw, K.qb}, {K.kw, K.kb}, {K.vw, K.vb}};
      float* bias;
      qkv_w_.push_back(fuse_rows(make_lin(dims[si], 3 * dims[si], 1, 1, 0), qkv, 3, fresh, &bias));
      qkv_b_.push_back(bias);
    }
  flush_packs();
  bn_sc_.clear(); bn_sh_.clear();
  for (const UpConvBn& c : cbs) {
    const int n = lins[c.conv].cout;
    float* sc = (float*)alloc((size_t)n * 4);
    float* sh = (float*)alloc((size_t)n * 4);
    bn_sc_.push_back(sc); bn_sh_.push_back(sh);
    if (!fresh) RUN(bn_eval_coeffs(n, params_ + c.g, params_ + c.b, params_ + c.rm, params_ + c.rv, 1e-5f, sc, sh, s_));
  }
  // ---- input, the backbone's outputs, the pyramid-pooling concatenation (stage 4's output is its first dims[3] channels)
  const int Cin_p = lins[patch].cin_p;
  void* xin = alloc((size_t)B * H * W * Cin_p * es);
  RUN(nchw_f32_to_nhwc(dtype, x_nchw, xin, B, in_channels, H, W, Cin_p, s_));
  int fh[4], fw[4];
  for (int i = 0; i < 4; ++i) { fh[i] = H >> (i + 2); fw[i] = W >> (i + 2); }
  void* feat[3];
  for (int i = 0; i < 3; ++i) feat[i] = alloc((size_t)B * fh[i] * fw[i] * dims[i] * es);
  const int D = hidden, pc_ld = dims[3] + 4 * D;
  unsigned char* ppm_cat = (unsigned char*)alloc((size_t)B * fh[3] * fw[3] * pc_ld * es);
  // ---- backbone
  void* x = alloc((size_t)B * fh[0] * fw[0] * dims[0] * es);
  {
    const size_t mark = ar_.top;
    void* t = alloc((size_t)B * fh[0] * fw[0] * dims[0] * es);
    gemm(lins[patch], xin, B, H, W, t, dims[0], nullptr, nullptr, nullptr, 0, nullptr);   // 4x4 stride-4 conv + bias
    layernorm(norms[patch_ln], t, x, (long)B * fh[0] * fw[0], dims[0]);
    ar_.release(mark);
  }
  size_t blk = 0;
  for (int i = 0; i < 4; ++i) {
    const SwStage& S = stages[i];
    const int C = dims[i], h = fh[i], w = fw[i];
    const long tokens = (long)B * h * w;
    void* xn = i < 3 ? alloc((size_t)tokens / 4 * 2 * C * es) : nullptr;
    const size_t mark = ar_.top;
    void* ln = alloc((size_t)tokens * C * es);
    void* qkv = alloc((size_t)tokens * 3 * C * es);
    void* ctx = alloc((size_t)tokens * C * es);
    void* f1 = alloc((size_t)tokens * 4 * C * es);
    const SfLin Lq = make_lin(C, 3 * C, 1, 1, 0);
    for (size_t bi = 0; bi < S.blocks.size(); ++bi, ++blk) {
      const SwBlock& K = S.blocks[bi];
      layernorm(norms[K.ln1], x, ln, tokens, C);
      gemm(Lq, ln, B, h, w, qkv, 3 * C, nullptr, nullptr, nullptr, 0, nullptr, 0, ar_.base + qkv_w_[blk], qkv_b_[blk]);
      RUN(swin_window_attention(dtype, qkv, qkv_b_[blk], params_ + K.table, ctx, B, h, w, C, heads[i], (bi & 1) ? 3 : 0, s_));
      gemm(lins[K.o], ctx, B, h, w, x, C, /*residual*/ x, nullptr, nullptr, 0, nullptr);   // x = o_proj(ctx) + x in place
      layernorm(norms[K.ln2], x, ln, tokens, C);
      gemm(lins[K.fc1], ln, B, h, w, f1, 4 * C, nullptr, nullptr, nullptr, 0, nullptr, /*gelu*/ 1);
      gemm(lins[K.fc2], f1, B, h, w, x, C, /*residual*/ x, nullptr, nullptr, 0, nullptr);
    }
    if (i < 3) layernorm(norms[hs_norm[i]], x, feat[i], tokens, C);
    else layernorm(norms[hs_norm[3]], x, ppm_cat, tokens, pc_ld);
    if (i < 3) {   // patch merging: gather + LayerNorm(4C) into `ln` (tokens / 4 rows of 4C), reduction 4C -> 2C
      RUN(swin_patch_merge_ln(dtype, x, params_ + norms[S.merge_ln].g_off, params_ + norms[S.merge_ln].b_off, ln, B, h, w, C, 1e-5f, s_));
      gemm(lins[S.reduction], ln, B, h / 2, w / 2, xn, 2 * C, nullptr, nullptr, nullptr, 0, nullptr);
    }
    ar_.release(mark);   // the stage's scratch is free again (one stream: later launches are ordered behind its readers)
    x = xn;
  }
  // ---- head: laterals, pyramid pooling + bottleneck
  void* lat[4];
  for (int i = 0; i < 4; ++i) lat[i] = alloc((size_t)B * fh[i] * fw[i] * D * es);
  for (int i = 0; i < 3; ++i) conv_bn_relu(lateral[i], feat[i], B, fh[i], fw[i], lat[i], D);
  {
    const size_t mark = ar_.top;
    for (int j = 0; j < 4; ++j) {
      const int Sc = pool_scales[j];
      void* pooled = alloc((size_t)B * Sc * Sc * dims[3] * es);
      void* pp = alloc((size_t)B * Sc * Sc * D * es);
      RUN(swin_adaptive_avgpool(dtype, ppm_cat, pc_ld, pooled, B, fh[3], fw[3], dims[3], Sc, s_));
      conv_bn_relu(psp[j], pooled, B, Sc, Sc, pp, D);
      RUN(sf_bilinear_nhwc(dtype, pp, ppm_cat + (size_t)(dims[3] + j * D) * es, B, Sc, Sc, D, fh[3], fw[3], pc_ld, s_));
    }
    conv_bn_relu(bottleneck, ppm_cat, B, fh[3], fw[3], lat[3], D);
    ar_.release(mark);
  }
  // ---- top-down path: each step reads the level the previous step updated
  for (int i = 3; i > 0; --i) RUN(swin_bilinear_add(dtype, lat[i], lat[i - 1], B, fh[i], fw[i], D, fh[i - 1], fw[i - 1], s_));
  // ---- FPN convs, every level at level 0's size in its channel slice of the concatenation, fpn_bottleneck, classifier
  unsigned char* fcat = (unsigned char*)alloc((size_t)B * fh[0] * fw[0] * 4 * D * es);
  conv_bn_relu(fpn[0], lat[0], B, fh[0], fw[0], fcat, 4 * D);
  for (int i = 1; i < 3; ++i) {
    const size_t mark = ar_.top;
    void* t = alloc((size_t)B * fh[i] * fw[i] * D * es);
    conv_bn_relu(fpn[i], lat[i], B, fh[i], fw[i], t, D);
    RUN(sf_bilinear_nhwc(dtype, t, fcat + (size_t)i * D * es, B, fh[i], fw[i], D, fh[0], fw[0], 4 * D, s_));
    ar_.release(mark);
  }
  RUN(sf_bilinear_nhwc(dtype, lat[3], fcat + (size_t)3 * D * es, B, fh[3], fw[3], D, fh[0], fw[0], 4 * D, s_));
  void* z = alloc((size_t)B * fh[0] * fw[0] * D * es);
  conv_bn_relu(fpn_bottleneck, fcat, B, fh[0], fw[0], z, D);
  float* lq = (float*)alloc((size_t)B * num_labels * fh[0] * fw[0] * 4);
  // 1x1 conv + bias: fp32 NCHW at 1/4, for a quarter-resolution caller straight into its tensor (the workspace plan is the same)
  gemm(lins[cls], z, B, fh[0], fw[0], nullptr, 0, nullptr, nullptr, nullptr, 0, quarter ? logits : lq);
  if (!quarter) RUN(sf_bilinear_nchw_f32(lq, logits, (long)B * num_labels, fh[0], fw[0], H, W, s_));
  return end();
}

size_t UperNet::workspace_bytes(int B, int H, int W) {
  const int bc = max_batch(H, W);
  return planned(run(nullptr, nullptr, reinterpret_cast<float*>(16), B < bc ? B : bc, H, W, nullptr, 0, nullptr, true, false));
}

int UperNet::forward(const float* params, const float* x_nchw, float* logits, int B, int H, int W, void* ws, size_t ws_bytes, hipStream_t s,
                     bool quarter) {
  if (!params || !x_nchw || !logits || !ws || B < 1) return -1;
  const int bc = max_batch(H, W);
  for (int b0 = 0; b0 < B; b0 += bc) {   // passes of at most bc images through the same workspace
    const int nb = B - b0 < bc ? B - b0 : bc;
    const size_t out_px = quarter ? (size_t)(H / 4) * (W / 4) : (size_t)H * W;
    const int rc = run(params, x_nchw + (size_t)b0 * in_channels * H * W, logits + (size_t)b0 * num_labels * out_px, nb, H, W, ws, ws_bytes,
                       s, false, quarter);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace flair
