// Native inference executor of UperNetForSemanticSegmentation with a SwinBackbone (see upernet.hip).
#pragma once
#include <string>
#include <vector>

#include "tf_exec.h"

namespace flair {

struct SwBlock { int ln1, o, ln2, fc1, fc2; long qw, qb, kw, kb, vw, vb, table; };
struct SwStage { std::vector<SwBlock> blocks; int merge_ln = -1, reduction = -1, out_ln = -1; };
struct UpConvBn { int conv; long g, b, rm, rv; };   // conv (no bias) + BatchNorm (eval) + ReLU

class UperNet : public TfExec {
 public:
  UperNet(int in_channels, int num_labels, int embed_dim, const int* depths, const int* heads, int hidden, const int* pool_scales,
          int aux_in, int aux_channels, int dtype);
  int in_channels, num_labels, embed_dim, hidden;
  int depths[4], heads[4], pool_scales[4], dims[4];
  static bool shape_ok(int H, int W);
  int max_batch(int H, int W) const;   // images per internal pass (every tensor below 2^31 elements)
  size_t workspace_bytes(int B, int H, int W);
  // logits: fp32 NCHW (B, labels, H, W) = the library's `.logits` (decode head at 1/4 resolution, then bilinear to the input size);
  // quarter: (B, labels, H/4, W/4), the classifier's own output, and no x4 pass
  int forward(const float* params, const float* x_nchw, float* logits, int B, int H, int W, void* ws, size_t ws_bytes, hipStream_t s,
              bool quarter);

 private:
  std::vector<SwStage> stages;
  int patch, patch_ln, hs_norm[4], cls;
  std::vector<UpConvBn> cbs;   // order: psp 0..3, bottleneck, lateral 0..2, fpn 0..2, fpn_bottleneck
  int psp[4], bottleneck, lateral[3], fpn[3], fpn_bottleneck;
  std::vector<size_t> qkv_w_;   // per block, in stage order: arena offset of the fused [q; k; v] packed weight, its concatenated bias
  std::vector<float*> qkv_b_;
  std::vector<float*> bn_sc_, bn_sh_;   // per entry of cbs: folded BatchNorm
  int add_cbn(const std::string& name, int cin, int cout, int k);
  void conv_bn_relu(int i, const void* in, int B, int Hin, int Win, void* out, int out_ld);
  void layernorm(const SfNorm& n, const void* x, void* y, long rows, int ld);
  int run(const float* params, const float* x_nchw, float* logits, int B, int H, int W, void* ws, size_t ws_bytes, hipStream_t s, bool dry,
          bool quarter);
};

}  // namespace flair
