// Launchers of swin_ops.hip (see there): the Swin-backbone and UperNet-head kernels the SegFormer path does not have.
#pragma once
#include "common.h"

namespace flair {
// Shifted-window multi-head self-attention of one Swin block, window 7 x 7, heads of 32 channels.  qkv [B][H][W][3C] is the fused
// [q | k | v] projection (biases included) over the UNPADDED token grid; the padding to multiples of 7, the cyclic shift by
// -shift, the window split, the merge back and the crop are the kernel's addressing.  Pad tokens take part as keys and values
// with q / k / v = the projection biases (qkv_bias [3C]); table = relative_position_bias_table [169][heads].  out [B][H][W][C].
int swin_window_attention(int dtype, const void* qkv, const float* qkv_bias, const float* table, void* out, int B, int H, int W, int C,
                          int heads, int shift, hipStream_t s);
// nn.LayerNorm over rows of C channels (dense input), output rows of ld elements (ld >= C)
int swin_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* y, long rows, int C, int ld, float eps,
                   hipStream_t s);
// SwinPatchMerging up to its reduction: x [B][H][W][C] (H, W even) -> LayerNorm(4C) of the concatenation
// [x(0::2, 0::2) | x(1::2, 0::2) | x(0::2, 1::2) | x(1::2, 1::2)], y [B][H/2][W/2][4C]
int swin_patch_merge_ln(int dtype, const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps,
                        hipStream_t s);
// nn.AdaptiveAvgPool2d(S): x rows of ld elements, channels [0, C) of [B][h][w]; y [B][S][S][C]
int swin_adaptive_avgpool(int dtype, const void* x, int ld, void* y, int B, int h, int w, int C, int S, hipStream_t s);
// y [B][H][W][C] += bilinear(x [B][h][w][C]) (size=(H, W), align_corners=False): the top-down path of the FPN
int swin_bilinear_add(int dtype, const void* x, void* y, int B, int h, int w, int C, int H, int W, hipStream_t s);
}  // namespace flair
