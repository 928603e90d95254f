// Native inference executor of SegformerForSemanticSegmentation (see segformer.hip).
#pragma once
#include <string>
#include <vector>

#include "tf_exec.h"

namespace flair {

struct SfBlock { int ln1, q, k, v, o, sr, sr_ln, ln2, fc1, fc2; long dw_w, dw_b; };
struct SfStage { int patch, patch_ln, out_ln; std::vector<SfBlock> blocks; };

class SegFormer : public TfExec {
 public:
  SegFormer(int in_channels, int num_labels, const int* depths, const int* hidden, const int* heads, const int* sr, int dec_hidden,
            int dtype);
  int in_channels, num_labels, dec_hidden;
  int depths[4], hidden[4], heads[4], sr[4];
  bool shape_ok(int H, int W) const;
  size_t workspace_bytes(int B, int H, int W);
  // logits_quarter: fp32 NCHW (B, labels, H/4, W/4) = the library's `.logits`; logits_full: the same upsampled x4 (bilinear,
  // align_corners = False) to the tile size.  Either may be null, not both.
  int forward(const float* params, const float* x_nchw, float* logits_quarter, float* logits_full, int B, int H, int W, void* ws,
              size_t ws_bytes, hipStream_t s);

 private:
  std::vector<SfStage> stages;
  int dec_proj[4], fuse, cls;
  long bn_g, bn_b, bn_rm, bn_rv;
  std::vector<size_t> kv_w_;   // per block, in stage order: arena offset of the fused [k; v] packed weight, its concatenated bias
  std::vector<float*> kv_b_;
  std::vector<float*> ffn_dw_;   // per block: regrouped depth-wise weights for the fused Mix-FFN kernel (null: not applicable)
  void layernorm(const SfNorm& n, const void* x, void* y, long rows);
  int run(const float* params, const float* x_nchw, float* logits_quarter, float* logits_full, int B, int H, int W, void* ws,
          size_t ws_bytes, hipStream_t s, bool dry);
};

}  // namespace flair
