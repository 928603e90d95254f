// Native executor for the smp-0.3.3 Unet(resnet34) graph the reference instantiates at
// /root/reference/src/flair/model.py:37-41 and runs at model.py:57-64.
// Owns the layer table, the flat parameter layout, the workspace arena and
// launches every kernel of forward / backward back-to-back on the caller's HIP stream.
#pragma once
#include <string>
#include <vector>

#include "arena.h"
#include "bwd_halo16.h"
#include "ops.h"

namespace flair {

struct Act {
  void* p = nullptr;
  int N = 0, H = 0, W = 0, C = 0;  // C = stored (padded) channel count
  // "lazy" activation: p is the producing unit's PRE-BatchNorm tensor and consumers apply relu(x*lz_scale + lz_shift)
  // while they stage it (ConvArgs::in_scale) — the activation itself is never written
  const float* lz_scale = nullptr;
  const float* lz_shift = nullptr;
  long rows() const { return (long)N * H * W; }
  long elems() const { return rows() * C; }
};

struct ConvDesc {
  std::string name;
  int Cin, Cout, R, S, stride, pad;
  int Cin_p, Cout_p;      // stored channel counts of the NHWC input / output tensors
  bool bias;
  long w_off = -1, b_off = -1;  // float offsets in the flat parameter buffer
  // packed copies (byte offsets into the workspace weight arena)
  size_t wf = 0, wd = 0;
  int Kpad, rows_f;       // forward pack (K = R*S*Cin_p, padded to whole K steps)
  int Kpad_d, rows_d;     // data-gradient pack (rows = Cin_p, K = R*S*Cout_p)
  // 3x3 stride-2 layers: the data gradient splits by output parity (py, px) into four stride-1 convolutions over dY
  // with 1, 2, 2 and 4 of the nine taps (class = 2*py + px) — a quarter of the gather-form kernel's MFMA work
  size_t wd_cls[4] = {0, 0, 0, 0};
  int Kpad_cls[4] = {0, 0, 0, 0};
  bool parity_dgrad() const { return stride == 2 && R == 3 && S == 3 && pad == 1; }
};

struct BnDesc {
  std::string name;
  int C;
  long g_off, b_off;      // flat parameter buffer
  long rm_off, rv_off;    // flat running-stat buffer
};

struct TensorInfo {
  std::string name;
  int ndim;
  long shape[4];
  long offset;
  int kind;  // 0 parameter (flat param buffer), 1 running statistic (flat buffer)
  int stage; // 0 stem, 1..4 encoder layers, 5 decoder, 6 head (gradient bucket id)
};

// Backward hand-off from the one consumer of a unit's `out` to that unit: the consumer's data-gradient kernel already reduced
// sum(dz), sum(dz*y) per pixel tile in its epilogue (ConvArgs::bnr_*, UNet::attach_bn_reduce).  masked: it also stored the gradient
// MASKED by the unit's ReLU (ConvArgs::bnr_mask), so the gradient buffer of `out` holds dz: what the identity branch of a BasicBlock
// receives and what the fused BatchNorm-backward apply of the unit's own data gradient (ConvArgs::ap_*) expects.
struct BnReduce {
  float* partial = nullptr;
  int nblk = 0;
  bool masked = false;
  BnReduce take() { const BnReduce r = *this; *this = BnReduce(); return r; }   // unit_backward consumes it
};

struct Unit {  // conv -> BN -> (+ residual) -> ReLU
  int conv = -1, bn = -1;
  Act in0, in1;
  bool up0 = false;
  Act y, out;
  float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
  bool relu = true;
  int res_unit = -1;   // downsample unit whose BN output is the residual
  Act res;             // identity residual
  BnReduce bnr;
};

// run_unit: what the unit's convolution reads, [up2(in0) if up0] ++ in1, and the ONE 3x3 convolution `cons` that reads its output,
// as [up2(out) if up0] ++ skip: it may take the pre-BatchNorm tensor and apply BN + ReLU while it stages (UNet::lazy_into_hg)
struct UnitIn { Act in0, in1; bool up0 = false; };
struct LazyOut { int cons = -1; bool up0 = false; Act skip; };

// unit_backward: dout = gradient w.r.t. the unit's `out`; a call site names what differs from the defaults
struct UnitBwd {
  const void* dout = nullptr;
  void* dres = nullptr; bool dres_acc = false;   // the residual branch's gradient dz is written (dres_acc: added) here
  bool dgrad = true;               // false: the stem, whose input needs no gradient
  bool upcat = false;              // decoder conv1: the input was cat([up2(in0), in1])
  const void* acc_src = nullptr;   // conv1 of a BasicBlock: the identity branch's share of dX as a tensor of its own (the masked
                                   // gradient of the block's output), added by the data gradient instead of a copy written as dres
};

// The data gradient of one layer, described before anything is launched (UNet::describe_dgrad)
struct DgradDesc {
  enum Form { DG_NONE, DG_PLAIN, DG_UPCAT_TILE, DG_UPCAT_SPLIT, DG_PARITY } form = DG_NONE;
  ConvArgs a;
  void *dx0 = nullptr, *dsk = nullptr, *dcat = nullptr;   // the upcat forms: gradient of in0, of the skip partner, of the concat
  bool acc0 = false, acc1 = false;
  int producer = -1;   // the unit whose BatchNorm-backward reduction rides in this launch's epilogue (attach_bn_reduce), or -1
};

// What one forward() does besides the plain pass (flair_unet_fwd_opts_t, include/flair_hip.h): arguments of that call, read while
// it runs and never kept, so no forward can meet what an earlier call left behind
struct FwdOpts {
  // The caller vouches that parameters and buffers are unchanged since the previous eval-mode forward on this handle: an eval-mode
  // forward with the same arena, shape, params and buffers addresses then skips the weight pack and the 46 BatchNorm-coefficient
  // launches (both still sit in the arena at the same offsets)
  bool reuse_constants = false;
  // an eval-mode forward without fp32 logits writes argmax predictions [B][H][W] uint8 (and the winner's probability) here
  unsigned char* preds = nullptr;
  float* maxprob = nullptr;
  // labels != null: an eval-mode forward without fp32 logits evaluates the per-pixel head of step() on its logits: weighted CE
  // mean -> loss, argmax -> preds (optional), confmat += bincount (optional); ws: ce_workspace_floats(B, H, W) floats
  struct Ce {
    const void* labels = nullptr; int kind = 0; const float* weight = nullptr;
    float* loss = nullptr; unsigned char* preds = nullptr; long long* confmat = nullptr; float* ws = nullptr;
  } ce;
  // rows (fp32 [B][H/32], device) join the bottleneck feature f_[5] between the encoder and the decoder, element [b][h][w][c] +
  // rows[b][h], the metadata fusion of model.py:59-60.  Eval mode: every unit materialises its output and f_[5] is read by decoder
  // block 0 alone, so the add happens in place; the arena layout does not change.  Training: the decoder gets a SECOND tensor,
  // f5m = T(float(f_[5]) + rows), and f_[5] stays — it is the ReLU mask source of layer4's last block in the backward (bn_backward,
  // the bnr_out of a residual producer), and out + rows reads as "ReLU on" wherever out == 0 < rows.  The backward of that forward
  // writes drows[b][h] = sum over w, c of the gradient that reaches f5m (complete and unmasked after the decoder's backward: nothing
  // produces f5m, so no data-gradient epilogue masks it) and hands that buffer to the encoder as the gradient of f_[5] (d f5m /
  // d f_[5] is the identity)
  const float* rows = nullptr;
  float* drows = nullptr;
  // 0, or the code forward() returns before it touches the handle or the device: a function of these arguments alone
  int refusal(int training, bool fp32_logits, int H, int W) const;
};

class UNet {
 public:
  UNet(int in_channels, int classes, int dtype);
  ~UNet();
  int in_channels, classes, dtype;
  std::vector<ConvDesc> convs;
  std::vector<BnDesc> bns;
  std::vector<TensorInfo> tensors;
  long n_params = 0, n_buffers = 0;
  long stage_begin[8];  // flat-parameter offset where each stage starts (stage_begin[7] = n_params)

  size_t workspace_bytes(int B, int H, int W, int training) const;   // side-effect free

  // stage entry points; features cross the boundary as NCHW fp32 only in the split path
  int forward(const float* params, float* buffers, const float* x_nchw, float* logits_nchw, int B, int H, int W,
              int training, void* ws, size_t ws_bytes, hipStream_t s, const FwdOpts& o);
  // stage_events: optional 7 hipEvent_t recorded on `s` as soon as the gradients of stage k
  // (6 head, 5 decoder, 4..1 encoder layers, 0 stem) are complete — lets the host overlap the
  // bucketed RCCL all-reduce with the rest of the backward pass.
  int backward(const float* params, const float* dlogits_nchw, const void* dlogits_nhwc, float* grads, void* ws,
               size_t ws_bytes, hipStream_t s, void* const* stage_events = nullptr);

  int encoder_forward(const float* params, float* buffers, const float* x_nchw, float* const feats_nchw[5], int B,
                      int H, int W, int training, void* ws, size_t ws_bytes, hipStream_t s);
  int decoder_forward(const float* params, float* buffers, const float* const feats_nchw[5], float* out_nchw, int B,
                      int H, int W, int training, void* ws, size_t ws_bytes, hipStream_t s);
  int head_forward(const float* params, const float* x_nchw, float* logits_nchw, int B, int H, int W, int training,
                   void* ws, size_t ws_bytes, hipStream_t s);
  int head_backward(const float* params, const float* dlogits_nchw, float* dx_nchw, float* grads, void* ws,
                    size_t ws_bytes, hipStream_t s);
  int decoder_backward(const float* params, const float* dout_nchw, float* const dfeats_nchw[5], float* grads,
                       void* ws, size_t ws_bytes, hipStream_t s);
  int encoder_backward(const float* params, const float* const dfeats_nchw[5], float* grads, void* ws,
                       size_t ws_bytes, hipStream_t s);

  // every entry point other than forward() lays the arena out differently (the split path re-imports five feature tensors
  // in front of the decoder units) or overwrites it: the constants of the last eval forward are gone
  void invalidate_reuse() { last_valid_ = false; last_params_ = nullptr; last_buffers_ = nullptr; }
  const void* logits_nhwc() const { return logits_nhwc_; }
  int head_ld() const { return convs.back().Cout_p; }

 private:
  // ---- arena (and the error of the call that runs on it)
  Arena ar_;
  hipStream_t s_ = nullptr;
  void* alloc(size_t bytes) { return ar_.get(bytes); }
  Act alloc_act(int N, int H, int W, int C);
  float* alloc_f(long n) { return (float*)alloc((size_t)n * 4); }

  // ---- per-call state
  const float* params_ = nullptr;
  float* buffers_ = nullptr;
  float* grads_ = nullptr;
  int B_ = 0, H_ = 0, W_ = 0, training_ = 0;
  std::vector<Unit> units_;
  Act xin_, f_[6], dec_in_[6], pool_, dec_out_;
  unsigned char* pool_idx_ = nullptr;
  int enc_units_end_ = 0, dec_units_begin_ = 0;
  int dec_conv0_ = 0, dec_bn0_ = 0;   // the first decoder convolution / BatchNorm of the table (build_table)
  size_t fwd_top_ = 0;      // arena top after forward (backward scratch starts here)
  bool packed_d_ = false;
  bool reuse_ = false, last_valid_ = false;
  const void* last_ws_ = nullptr;
  const void* last_params_ = nullptr;   // the flat buffers the packed weights / BatchNorm coefficients in the arena came from
  const void* last_buffers_ = nullptr;
  int last_B_ = 0, last_H_ = 0, last_W_ = 0;
  bool lazy_ok_ = false;
  int lazy_max_c_ = 16;    // widest unit that hands out a lazy activation (FLAIR_LAZY_BN=2: 32)
  // weight-gradient kernels run on an internal side stream, forked from / joined to the caller's stream with events, so
  // that their tails overlap the BatchNorm / data-gradient chain of the following units (FLAIR_WGRAD_STREAM=0: off)
  hipStream_t side_ = nullptr;
  hipStream_t note_ = nullptr;   // carries the listened-for stage events: waits for s_ and side_, blocks neither
  std::vector<hipEvent_t> fork_ev_;
  hipEvent_t join_ev_ = nullptr;
  size_t fork_next_ = 0;
  bool side_pending_ = false;
  Act f5m_;                         // the decoder's bottleneck input of the last training forward with rows, for its backward
  float* drows_pending_ = nullptr;  // where that backward writes the row sums; cleared once written and by every later forward that runs
  bool side_init();
  hipStream_t wgrad_stream();     // forks the side stream behind everything queued on s_ so far
  int side_cus() const;           // WgradArgs::cus of a launch on the side stream
  void side_join();
  void* logits_nhwc_ = nullptr;   // head output kept in NHWC T when forward() was called without an NCHW logits buffer
  void* const* stage_events_ = nullptr;
  void stage_done(int stage);

  struct GradBuf { void* act; void* g; bool init; };
  // unit whose ReLU output is `a`, if `a` has exactly one consumer and the unit's mask comes from y; else -1
  int sole_producer(const Act& a) const;
  int residual_producer(const Act& a) const;
  // asks the data gradient `a`, which completes the gradient of `target`, to run the first pass of the BatchNorm backward of the
  // unit that produced `target` in its epilogue; returns that unit (its Unit::bnr is set), or -1 when nothing was attached
  int attach_bn_reduce(ConvArgs& a, const Act& target);
  // the fused backward of a 16 -> 16 layer (bwd16_fusable): `a` / `w` as the separate path would launch them, x the layer input,
  // producer the unit attach_bn_reduce(a, x) returned
  bool bwd16_ok(int flavour, const ConvArgs& a, const WgradArgs& w, int producer) const;
  void bwd16_run(Bwd16Args& f, const ConvArgs& a, const WgradArgs& w, const Act& x, int producer);
  std::vector<GradBuf> gbufs_;
  // FLAIR_BWD_FUSE (0 / 1, default on): the halo-GEMM data gradients store their result masked by the consumer unit's ReLU, the
  // BatchNorm-backward apply pass then reads no mask source, and the identity branch takes the masked gradient without a copy
  bool bwd_fuse() const;
  void* grad_of(const Act& a, bool* accumulate);
  void* grad_peek(const Act& a);

  size_t plan_bytes(int B, int H, int W, int training);   // the dry run itself (clobbers per-call state)
  size_t plan_step_bytes(int B, int H, int W);            // the same for forward(training) + backward() as they run (training == 2)
  void build_table();
  int add_conv(const std::string& name, int cin, int cout, int k, int stride, int pad, bool bias, int stage);
  int add_bn(const std::string& name, int c, int stage);
  void begin(void* ws, size_t ws_bytes, hipStream_t s, bool dry);
  void set_lazy_policy();   // FLAIR_LAZY_BN -> lazy_ok_, lazy_max_c_
  size_t plan_end();        // closes a dry run: the plan, and a handle with no arena
  // backward-side entry points: -11 unless `ws` holds a training forward, else per-call state and the data-gradient packs
  int bwd_begin(const float* params, float* grads, void* ws, hipStream_t s);
  // decoder_forward / head_forward: -11 unless they resume the split forward on the same arena and shape
  int fwd_resume(const float* params, int B, int H, int W, int training, void* ws, hipStream_t s);
  void pack_forward_weights();
  void pack_dgrad_weights();
  int run_unit(int conv, int bn, const UnitIn& in, bool relu, int res_unit, const Act& res, bool materialize,
               const LazyOut& lazy = LazyOut());
  bool lazy_into_hg(const Act& y, const LazyOut& lazy) const;
  void encoder_fwd_impl(const float* x_nchw);
  void decoder_fwd_impl(const Act* f);   // over the features f[1..5]: f_, or what the split path re-imported (dec_in_)
  void head_fwd_impl(float* logits_nchw, const FwdOpts& o);
  // data gradient of layer `c` from dy (the gradient of its output, with that tensor's geometry) to the layer's input
  // [up2(in0)] ++ in1 of extent Hin x Win; takes the gradient buffers (grad_of) and attaches the upstream reduction
  DgradDesc describe_dgrad(const ConvDesc& c, const Act& dy, const Act& in0, const Act& in1, int Hin, int Win, bool upcat,
                           const void* acc_src);
  void unit_backward(int ui, const UnitBwd& g);
  const void* import_dlogits(const float* dlogits_nchw);
  void head_bwd_impl(const void* dl);
  void decoder_bwd_impl();
  void encoder_bwd_impl();
  void fwd_common_begin(const float* params, float* buffers, int B, int H, int W, int training);
};

}  // namespace flair
