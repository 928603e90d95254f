// Executor for smp-0.3.3 Unet(resnet34) on gfx950 — see unet.h.
// Reference call sites replaced: /root/reference/src/flair/model.py:57-64 (encoder / decoder /
// segmentation_head / whole-model forward) and their autograd backward.
#include <stdlib.h>

#include "unet.h"
#include "conv_args.h"
#include "conv_route.h"
#include "parity_pack.h"
#include "tune.h"

namespace flair {

static const int kBlocks[4] = {3, 4, 6, 3};   // BasicBlocks per ResNet34 layer

// ------------------------------------------------------------------------------------------ table
int UNet::add_conv(const std::string& name, int cin, int cout, int k, int stride, int pad, bool bias, int stage) {
  ConvDesc c;
  c.name = name; c.Cin = cin; c.Cout = cout; c.R = k; c.S = k; c.stride = stride; c.pad = pad; c.bias = bias;
  c.Cin_p = (int)round_up(cin, 8);
  // stored output channels: whole 32-byte (bf16) / 64-byte (fp32) groups.  Every layer of the graph is a multiple of 16 already;
  // the head's 13 classes take 16 columns, 19 classes 32 — with 24 (whole 16-byte chunks only, rounds 1-2) the head's backward had
  // no tile kernel (its data gradient has Cout_p INPUT channels, its weight gradient dy rows of Cout_p) and the lazy-BN training
  // path of the fused trainer refused 19 classes
  c.Cout_p = (int)round_up(cout < 16 ? 16 : cout, 16);
  c.w_off = n_params;
  TensorInfo t;
  t.name = name + ".weight"; t.ndim = 4; t.shape[0] = cout; t.shape[1] = cin; t.shape[2] = k; t.shape[3] = k;
  t.offset = n_params; t.kind = 0; t.stage = stage;
  tensors.push_back(t);
  n_params += (long)cout * cin * k * k;
  if (bias) {
    c.b_off = n_params;
    TensorInfo b;
    b.name = name + ".bias"; b.ndim = 1; b.shape[0] = cout; b.shape[1] = b.shape[2] = b.shape[3] = 1;
    b.offset = n_params; b.kind = 0; b.stage = stage;
    tensors.push_back(b);
    n_params += cout;
  }
  c.Kpad = conv_kpad(dtype, k * k * c.Cin_p);
  c.rows_f = conv_weight_rows_pad(cout);
  c.Kpad_d = conv_kpad(dtype, k * k * c.Cout_p);
  c.rows_d = conv_weight_rows_pad(c.Cin_p);
  convs.push_back(c);
  return (int)convs.size() - 1;
}

int UNet::add_bn(const std::string& name, int C, int stage) {
  BnDesc b;
  b.name = name; b.C = C;
  const char* suffix[4] = {".weight", ".bias", ".running_mean", ".running_var"};
  long* const off[4] = {&b.g_off, &b.b_off, &b.rm_off, &b.rv_off};
  for (int i = 0; i < 4; ++i) {
    long& n = i < 2 ? n_params : n_buffers;   // parameters, then running statistics
    TensorInfo t;
    t.name = name + suffix[i]; t.ndim = 1; t.shape[0] = C; t.shape[1] = t.shape[2] = t.shape[3] = 1;
    t.offset = n; t.kind = i < 2 ? 0 : 1; t.stage = stage;
    tensors.push_back(t);
    *off[i] = n;
    n += C;
  }
  bns.push_back(b);
  return (int)bns.size() - 1;
}

// Layer order == forward order == flat parameter order, so the gradient of stage k occupies
// [stage_begin[k], stage_begin[k+1]) and becomes ready in reverse order during backward
// (bucketed RCCL all-reduce).  Every stage start is padded to 4 floats.
void UNet::build_table() {
  auto pad4 = [&]() { n_params = round_up(n_params, 4); };
  stage_begin[0] = 0;
  add_conv("encoder.conv1", in_channels, 64, 7, 2, 3, false, 0);
  add_bn("encoder.bn1", 64, 0);
  const int planes[4] = {64, 128, 256, 512};
  int inpl = 64;
  for (int L = 0; L < 4; ++L) {
    pad4();
    stage_begin[L + 1] = n_params;
    for (int b = 0; b < kBlocks[L]; ++b) {
      const std::string p = "encoder.layer" + std::to_string(L + 1) + "." + std::to_string(b);
      const int stride = (b == 0 && L > 0) ? 2 : 1;
      add_conv(p + ".conv1", inpl, planes[L], 3, stride, 1, false, L + 1);
      add_bn(p + ".bn1", planes[L], L + 1);
      add_conv(p + ".conv2", planes[L], planes[L], 3, 1, 1, false, L + 1);
      add_bn(p + ".bn2", planes[L], L + 1);
      if (b == 0 && (stride != 1 || inpl != planes[L])) {
        add_conv(p + ".downsample.0", inpl, planes[L], 1, stride, 0, false, L + 1);
        add_bn(p + ".downsample.1", planes[L], L + 1);
      }
      inpl = planes[L];
    }
  }
  pad4();
  stage_begin[5] = n_params;
  dec_conv0_ = (int)convs.size(); dec_bn0_ = (int)bns.size();
  const int din[5] = {512, 256, 128, 64, 32}, dskip[5] = {256, 128, 64, 64, 0}, dout[5] = {256, 128, 64, 32, 16};
  for (int i = 0; i < 5; ++i) {
    const std::string p = "decoder.blocks." + std::to_string(i);
    add_conv(p + ".conv1.0", din[i] + dskip[i], dout[i], 3, 1, 1, false, 5);
    add_bn(p + ".conv1.1", dout[i], 5);
    add_conv(p + ".conv2.0", dout[i], dout[i], 3, 1, 1, false, 5);
    add_bn(p + ".conv2.1", dout[i], 5);
  }
  pad4();
  stage_begin[6] = n_params;
  add_conv("segmentation_head.0", 16, classes, 3, 1, 1, true, 6);
  pad4();
  stage_begin[7] = n_params;
}

UNet::UNet(int in_ch, int cls, int dt) : in_channels(in_ch), classes(cls), dtype(dt) { build_table(); }

UNet::~UNet() {
  for (hipEvent_t e : fork_ev_) (void)hipEventDestroy(e);
  if (join_ev_) (void)hipEventDestroy(join_ev_);
  if (side_) (void)hipStreamDestroy(side_);
  if (note_) (void)hipStreamDestroy(note_);
}

// a non-blocking stream; prio 1 / 2: of the device's lowest / highest priority level, where it has more than one
static hipError_t make_stream(hipStream_t* s, int prio) {
  int least = 0, greatest = 0;
  if (prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio == 2 ? greatest : least);
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

bool UNet::side_init() {
  if (!tune("FLAIR_WGRAD_STREAM", 1)) return false;
  if (side_) return true;
  // LOW priority: (a) the weight gradients are off the critical path — when both streams have workgroups to dispatch,
  // the BatchNorm / data-gradient chain goes first; (b) a priority level has hardware queues of its own, so the side
  // stream can never be mapped onto the caller's queue.  (HIP multiplexes streams over a few hardware queues; with RCCL's
  // and torch's extra streams alive the round-robin put this stream on the caller's queue and the overlap was gone:
  // +1.4 ms per step in the single-rank rehearsal of the exchange, gpurun_out/prof_exch Queue_Id column.)
  if (make_stream(&side_, tune("FLAIR_SIDE_PRIO", 1) != 0 ? 1 : 0) != hipSuccess) { side_ = nullptr; return false; }
  // The fork / join events order streams of ONE device: no system-scope fence (the default makes every record write back and
  // invalidate the caches — 50 times per step, in front of the kernels that re-read what was just written)
  const unsigned evflags = hipEventDisableTiming | (tune("FLAIR_EVENT_SYSFENCE", 0) ? 0u : hipEventDisableSystemFence);
  fork_ev_.resize(128);
  for (auto& e : fork_ev_)
    if (hipEventCreateWithFlags(&e, evflags) != hipSuccess) return false;
  return hipEventCreateWithFlags(&join_ev_, evflags) == hipSuccess;
}

// Space sharing instead of time sharing: on the side stream the persistent weight-gradient kernel takes only HALF of the
// CUs (FLAIR_WG_CUS, 128), for twice as long.  The caller's stream always finds free CUs — its BatchNorm kernels, HBM-bound,
// lose little on the other half and no longer queue behind 256 persistent workgroups (the "35 us bn_bwd_finalize" of the
// round-2 trace) — and half the workgroups means half the fp32 slabs (75 -> 37 MB written and re-read per launch).
// Step 13.2 -> 12.4 ms (192 CUs: 12.55, 144: 12.48, 112: 12.56, 96: 12.87; giving the last units of backward, when the
// caller's stream runs dry, the whole chip again: +0.05 ... +0.3 ms).
int UNet::side_cus() const {
  if (!tune("FLAIR_WGRAD_STREAM", 1)) return 0;
  // fp32 mode: everything is matrix-pipe-bound there (fp32 MFMA is 16x slower), the BatchNorm kernels are a small share and
  // halving the weight-gradient kernels' CUs costs more than it frees: 57.4 ms with the whole chip, 58.4 with 192, 62.2 with 128
  const int v = tune("FLAIR_WG_CUS", 0);   // (tune() caches its default per key: the dtype-dependent default lives here)
  return v > 0 ? v : (dtype == DT_F32 ? 256 : 128);
}

hipStream_t UNet::wgrad_stream() {
  if (ar_.dry || ar_.err || !side_init()) return s_;
  hipEvent_t e = fork_ev_[fork_next_++ % fork_ev_.size()];
  if (hipEventRecord(e, s_) != hipSuccess || hipStreamWaitEvent(side_, e, 0) != hipSuccess) return s_;
  side_pending_ = true;
  return side_;
}

void UNet::side_join() {
  if (!side_pending_ || ar_.dry) return;
  side_pending_ = false;
  if (hipEventRecord(join_ev_, side_) != hipSuccess || hipStreamWaitEvent(s_, join_ev_, 0) != hipSuccess) {
    if (!ar_.err) ar_.err = -13;
  }
}

// ------------------------------------------------------------------------------------------ arena
Act UNet::alloc_act(int N, int H, int W, int C) {
  Act a;
  a.N = N; a.H = H; a.W = W; a.C = C;
  a.p = alloc((size_t)a.elems() * dtype_size(dtype));
  return a;
}

void UNet::begin(void* ws, size_t ws_bytes, hipStream_t s, bool dry) {
  ar_.reset(ws, ws_bytes, dry);
  s_ = s;
  units_.clear();
  gbufs_.clear();
  packed_d_ = false;
  logits_nhwc_ = nullptr;
  // weight arena
  for (auto& c : convs) {
    c.wf = ar_.top; alloc((size_t)c.rows_f * c.Kpad * dtype_size(dtype));
  }
  for (auto& c : convs) {
    c.wd = ar_.top; alloc((size_t)c.rows_d * c.Kpad_d * dtype_size(dtype));
  }
  for (auto& c : convs) {
    if (!c.parity_dgrad()) continue;
    for (int cls = 0, kg; cls < 4; ++cls) {
      parity_class_geom(dtype, c.Cout_p, cls, kg, c.Kpad_cls[cls]);
      c.wd_cls[cls] = ar_.top; alloc((size_t)c.rows_d * c.Kpad_cls[cls] * dtype_size(dtype));
    }
  }
}

// fp32 OIHW masters -> packed T copies, all 47 convolutions in one launch
void UNet::pack_forward_weights() {
  PackTable tb;
  tb.n = 0;
  for (auto& c : convs) tb.d[tb.n++] = pack_desc(c.w_off, c.wf, c.Cout, c.Cin, c.R, c.Cin_p, c.rows_f, c.Kpad, 0);
  RUN(pack_weights_all(dtype, params_, ar_.base, tb, s_));
}

void UNet::pack_dgrad_weights() {
  if (packed_d_) return;
  packed_d_ = true;
  PackTable tb;
  tb.n = 0;
  for (size_t i = 1; i < convs.size(); ++i) {  // the stem needs no data gradient
    auto& c = convs[i];
    const PackDesc full = tb.d[tb.n++] = pack_desc(c.w_off, c.wd, c.Cout, c.Cin, c.R, c.Cout_p, c.rows_d, c.Kpad_d, 1);
    if (c.parity_dgrad()) {
      for (int cls = 0; cls < 4; ++cls) tb.d[tb.n++] = parity_class_pack(full, cls, c.wd_cls[cls], c.Kpad_cls[cls]);
    }
  }
  RUN(pack_weights_all(dtype, params_, ar_.base, tb, s_));
}

void* UNet::grad_of(const Act& a, bool* accumulate) {
  for (auto& g : gbufs_)
    if (g.act == a.p) { *accumulate = g.init; g.init = true; return g.g; }
  GradBuf g;
  g.act = a.p;
  g.g = alloc((size_t)a.elems() * dtype_size(dtype));
  g.init = true;
  *accumulate = false;
  gbufs_.push_back(g);
  return g.g;
}

void* UNet::grad_peek(const Act& a) {
  for (auto& g : gbufs_)
    if (g.act == a.p) return g.g;
  return nullptr;
}

// ------------------------------------------------------------------------------------------ forward
static ConvInput conv_input(const Act& in0, const Act& in1, bool up0) {
  return ConvInput{in0.p, in1.p, in0.C, in1.p ? in1.C : 0, up0 ? 1 : 0, in0.N, in0.H, in0.W};
}

// forward launch of layer `c` over [up2(in0) if up0] ++ in1 into the tensor at `y` with rows of c.Cout_p stored channels
static void fill_conv_args(ConvArgs& a, int dtype, const ConvDesc& c, const Act& in0, const Act& in1, bool up0, void* y, const void* wpacked) {
  conv_fwd_args(a, dtype, conv_input(in0, in1, up0), c.R, c.stride, c.pad, c.Cout);
  a.w = wpacked;
  a.out = y; a.out_ld = c.Cout_p;
  a.in_scale = in0.lz_scale; a.in_shift = in0.lz_shift;   // lazy producers never feed a concat partner (in1)
}

// Can the unit producing `y` (conv + BN + ReLU, no residual) hand its PRE-BatchNorm tensor to its single consumer, the
// 3x3 convolution `cons` (input = [up2(y) if up0] ++ skip), which then applies BN + ReLU while it stages its halo — in
// the forward pass (halo-GEMM kernel) and again in its weight gradient (wgrad3x3_big)?
bool UNet::lazy_into_hg(const Act& y, const LazyOut& lazy) const {
  if (!training_ || !tune("FLAIR_LAZY_HG", 1)) return false;
  const ConvDesc& c = convs[lazy.cons];
  const Act& skip = lazy.skip;
  const bool up0 = lazy.up0;
  if (c.R != 3 || c.stride != 1) return false;
  Act in0 = y;
  in0.p = reinterpret_cast<void*>(16);   // (the predicates only look at which pointers are set)
  ConvArgs a;
  fill_conv_args(a, dtype, c, in0, skip, up0, in0.p, in0.p);
  a.in_scale = a.in_shift = reinterpret_cast<const float*>(16);
  if (!conv_hg_applicable(dtype, a)) return false;
  WgradArgs w;
  wgrad_args(w, conv_input(in0, skip, up0), c.R, c.stride, c.pad, in0.p, c.Cout_p, c.Cout, nullptr, c.Cin);
  w.in_scale = w.in_shift = reinterpret_cast<const float*>(16);
  return wgrad_big_applicable(dtype, w);
}

int UNet::run_unit(int ci, int bi, const UnitIn& in, bool relu, int res_unit, const Act& res, bool materialize,
                   const LazyOut& lazy_out) {
  const ConvDesc& c = convs[ci];
  const BnDesc& b = bns[bi];
  const Act &in0 = in.in0, &in1 = in.in1;
  const bool up0 = in.up0;
  Unit u;
  u.conv = ci; u.bn = bi; u.in0 = in0; u.in1 = in1; u.up0 = up0; u.relu = relu; u.res_unit = res_unit; u.res = res;
  const int Ho = conv_out_extent(up0 ? in0.H * 2 : in0.H, c.R, c.stride, c.pad);
  const int Wo = conv_out_extent(up0 ? in0.W * 2 : in0.W, c.S, c.stride, c.pad);
  u.y = alloc_act(in0.N, Ho, Wo, c.Cout_p);
  u.scale = alloc_f(b.C); u.shift = alloc_f(b.C); u.mean = alloc_f(b.C); u.invstd = alloc_f(b.C);
  ConvArgs a;
  fill_conv_args(a, dtype, c, in0, in1, up0, u.y.p, ar_.base + c.wf);
  if (!training_) {
    // inference: BatchNorm (running statistics) is a per-channel affine -> folded, together with the residual
    // add and the ReLU, into the conv epilogue; the pre-BN tensor is never written
    if (!reuse_)   // constant weights: the coefficients of the previous eval forward are still at u.scale / u.shift
      RUN(bn_eval_coeffs(b.C, params_ + b.g_off, params_ + b.b_off, buffers_ + b.rm_off, buffers_ + b.rv_off, 1e-5f,
                         u.scale, u.shift, s_));
    u.out = u.y;
    a.oscale = u.scale; a.oshift = u.shift; a.orelu = relu ? 1 : 0;
    a.ores = res_unit >= 0 ? units_[res_unit].out.p : res.p;
    RUN(launch_conv(dtype, a, s_));
    units_.push_back(u);
    return (int)units_.size() - 1;
  }
  const int nblk = conv_grid_rows(dtype, a);
  float* partial = alloc_f((long)nblk * 2 * b.C);
  a.stats = partial;
  RUN(launch_conv(dtype, a, s_));
  RUN(bn_finalize(partial, nblk, b.C, u.y.rows(), params_ + b.g_off, params_ + b.b_off, buffers_ + b.rm_off,
                  buffers_ + b.rv_off, 0.1f, 1e-5f, u.scale, u.shift, u.mean, u.invstd, s_));
  // The 16-channel decoder units (block 4: 45 % of all BN-apply bytes) feed only small-channel halo kernels,
  // which can apply BN + ReLU while staging their input: skip the activation pass and hand out the pre-BN tensor.
  // The >= 64-channel units whose single consumer is a halo-GEMM convolution do the same (conv1 of every BasicBlock,
  // decoder conv1 / conv2 of the wide blocks): bn_act and the normalised activation tensor vanish for them.
  const bool plain = lazy_ok_ && materialize && relu && res_unit < 0 && !res.p;
  bool lazy = plain && c.R == 3 && c.stride == 1 && c.Cout_p <= lazy_max_c_ && (Ho % 8) == 0 && (Wo % 32) == 0;
  if (!lazy && plain && lazy_out.cons >= 0) lazy = lazy_into_hg(u.y, lazy_out);
  if (lazy) {
    u.out = u.y;
    u.out.lz_scale = u.scale; u.out.lz_shift = u.shift;
  } else if (materialize) {
    u.out = alloc_act(in0.N, Ho, Wo, c.Cout_p);
    const void* rp = nullptr;
    const float *rs = nullptr, *rh = nullptr;
    if (res_unit >= 0) { rp = units_[res_unit].y.p; rs = units_[res_unit].scale; rh = units_[res_unit].shift; }
    else if (res.p) rp = res.p;
    RUN(bn_act(dtype, u.y.p, u.scale, u.shift, rp, rs, rh, u.out.p, u.y.rows(), b.C, relu ? 1 : 0, s_));
  }
  units_.push_back(u);
  return (int)units_.size() - 1;
}

void UNet::fwd_common_begin(const float* params, float* buffers, int B, int H, int W, int training) {
  params_ = params; buffers_ = buffers; B_ = B; H_ = H; W_ = W; training_ = training;
}

void UNet::set_lazy_policy() {
  const int lazy_env = tune("FLAIR_LAZY_BN", 1);
  lazy_ok_ = lazy_env != 0;
  lazy_max_c_ = lazy_env >= 2 ? 32 : 16;
}

int UNet::fwd_resume(const float* params, int B, int H, int W, int training, void* ws, hipStream_t s) {
  invalidate_reuse();
  if (ws != ar_.base || B != B_ || H != H_ || W != W_) return -11;
  s_ = s; params_ = params; training_ = training;
  return 0;
}

void UNet::encoder_fwd_impl(const float* x_nchw) {
  xin_ = alloc_act(B_, H_, W_, convs[0].Cin_p);
  RUN(nchw_f32_to_nhwc(dtype, x_nchw, xin_.p, B_, in_channels, H_, W_, xin_.C, s_));
  const Act none;
  int ci = 0, bi = 0;
  // training: the stem's BatchNorm + ReLU pass and the max pool read the pre-BN tensor together (bn_act_maxpool_kernel)
  const bool fuse_pool = training_ && tune("FLAIR_STEM_POOL", 1);
  int u = run_unit(ci++, bi++, {xin_}, /*relu*/ true, /*res_unit*/ -1, /*res*/ none, /*materialize*/ !fuse_pool);
  if (fuse_pool) units_[u].out = alloc_act(units_[u].y.N, units_[u].y.H, units_[u].y.W, units_[u].y.C);
  f_[1] = units_[u].out;
  pool_ = alloc_act(B_, f_[1].H / 2, f_[1].W / 2, 64);
  pool_idx_ = training_ ? (unsigned char*)alloc((size_t)pool_.elems()) : nullptr;
  if (fuse_pool)
    RUN(bn_act_maxpool3x3s2(dtype, units_[u].y.p, units_[u].scale, units_[u].shift, f_[1].p, pool_.p, pool_idx_, B_, f_[1].H, f_[1].W, 64, s_));
  else
    RUN(maxpool3x3s2_fwd(dtype, f_[1].p, pool_.p, pool_idx_, B_, f_[1].H, f_[1].W, 64, s_));
  Act x = pool_;
  for (int L = 0; L < 4; ++L) {
    for (int b = 0; b < kBlocks[L]; ++b) {
      // BasicBlock: x -> conv1 -> conv2, + (downsample(x) or x) -> ReLU
      const bool ds = (b == 0 && L > 0);
      const int c1 = ci++, b1 = bi++, c2 = ci++, b2 = bi++;
      const int u1 = run_unit(c1, b1, {x}, /*relu*/ true, /*res_unit*/ -1, /*res*/ none, /*materialize*/ true, /*read by conv2 alone*/ LazyOut{c2});
      int ud = -1;   // the downsample unit stays pre-BatchNorm: conv2's BN-apply pass adds it
      if (ds) { const int cd = ci++, bd = bi++; ud = run_unit(cd, bd, {x}, /*relu*/ false, /*res_unit*/ -1, /*res*/ none, /*materialize*/ false); }
      const int u2 = run_unit(c2, b2, {units_[u1].out}, /*relu*/ true, /*res_unit*/ ud, /*res*/ ds ? none : x, /*materialize*/ true);
      x = units_[u2].out;
    }
    f_[L + 2] = x;
  }
  enc_units_end_ = (int)units_.size();
}

void UNet::decoder_fwd_impl(const Act* f) {
  const Act none;
  dec_units_begin_ = (int)units_.size();
  int ci = dec_conv0_, bi = dec_bn0_;
  Act x = f[5];
  for (int i = 0; i < 5; ++i) {
    // DecoderBlock: cat([up2(x), skip]) -> conv1 -> conv2
    const Act skip = i < 4 ? f[4 - i] : none;
    const int c1 = ci++, b1 = bi++, c2 = ci++, b2 = bi++;
    // conv1's output is read by conv2 alone, conv2's by the next block's conv1, upsampled and next to that block's skip partner
    // (the last block's by the head: no lazy consumer)
    const LazyOut to_next = i < 4 ? LazyOut{c2 + 1, true, i < 3 ? f[3 - i] : none} : LazyOut();
    const int u1 = run_unit(c1, b1, {x, skip, true}, /*relu*/ true, /*res_unit*/ -1, /*res*/ none, /*materialize*/ true, LazyOut{c2});
    const int u2 = run_unit(c2, b2, {units_[u1].out}, /*relu*/ true, /*res_unit*/ -1, /*res*/ none, /*materialize*/ true, to_next);
    x = units_[u2].out;
  }
  dec_out_ = x;
}

void UNet::head_fwd_impl(float* logits_nchw, const FwdOpts& o) {
  const ConvDesc& c = convs.back();
  Act none;
  ConvArgs a;
  fill_conv_args(a, dtype, c, dec_out_, none, false, nullptr, ar_.base + c.wf);
  if (logits_nchw || ar_.dry) {
    a.out = nullptr;
    a.out_nchw = logits_nchw;
    logits_nhwc_ = nullptr;
  }
  if (!logits_nchw) {
    // nobody asked for fp32 NCHW logits (the fused trainer): keep them in the network's layout, [B*H*W][Cout_p] T, for
    // flair_ce_head_nhwc — 40 % fewer bytes than the NCHW fp32 tensor and contiguous rows on both sides
    logits_nhwc_ = alloc((size_t)dec_out_.rows() * c.Cout_p * dtype_size(dtype));
    if (!ar_.dry) { a.out = logits_nhwc_; a.out_ld = c.Cout_p; a.out_nchw = nullptr; }
  }
  a.bias = params_ + c.b_off;
  unsigned char* preds = (!logits_nchw && !training_) ? o.preds : nullptr;
  float* maxprob = preds ? o.maxprob : nullptr;
  const FwdOpts::Ce& ce = o.ce;   // (FwdOpts::refusal lets it through for eval-mode calls without fp32 logits only)
  if (ce.labels && !ar_.dry) {
    // validation: loss term, argmax and confusion-matrix increment in the head convolution's register epilogue, between the label
    // pass and the fp64 sum of ce_head (the logits never reach HBM); otherwise the head convolution to NHWC logits and ce_head on
    // them — one behaviour for the caller on every shape
    const long npix = dec_out_.rows();
    const CeWorkspace w = ce_workspace_layout(ce.ws, npix);
    ConvArgs b = a;
    b.out = nullptr; b.preds_u8 = ce.preds;
    b.ce_lab8 = w.lab8; b.ce_weight = ce.weight; b.ce_loss_partial = w.loss_partial; b.ce_confmat = ce.confmat;
    if (conv_halo_ce_ok(dtype, b)) {
      logits_nhwc_ = nullptr;
      RUN(ce_labels(ce.labels, ce.kind, ce.weight, dec_out_.N, c.Cout, dec_out_.H, dec_out_.W, nullptr, ce.ws, s_));
      RUN(launch_conv(dtype, b, s_));
      RUN(ce_finish(ce.ws, npix, conv_grid_rows(dtype, b), ce.loss, s_));
      return;
    }
    RUN(launch_conv(dtype, a, s_));
    CeArgs h;
    h.logits = nullptr; h.logits_nhwc = logits_nhwc_; h.logits_dtype = dtype; h.logits_ld = c.Cout_p;
    h.labels = ce.labels; h.label_kind = ce.kind; h.weight = ce.weight;
    h.B = dec_out_.N; h.C = c.Cout; h.H = dec_out_.H; h.W = dec_out_.W; h.loss = ce.loss;
    h.dlogits_nchw = nullptr; h.dlogits_nhwc = nullptr; h.dlogits_dtype = dtype; h.dlogits_ld = c.Cout_p;
    h.preds_u8 = ce.preds; h.preds_i64 = nullptr; h.targets_i32 = nullptr; h.confmat = ce.confmat; h.workspace = ce.ws;
    RUN(ce_head(h, s_));
    return;
  }
  if (preds && !ar_.dry) {
    // predict: argmax in the head convolution's register epilogue, the logits never reach HBM (536 MB of traffic and the
    // softmax_argmax launch saved); otherwise the separate kernel over the NHWC logits
    ConvArgs b = a;
    b.out = nullptr; b.preds_u8 = preds; b.maxprob_f32 = maxprob;
    if (conv_halo_preds_ok(dtype, b)) {
      logits_nhwc_ = nullptr;
      RUN(launch_conv(dtype, b, s_));
      return;
    }
  }
  RUN(launch_conv(dtype, a, s_));
  if (preds && !ar_.dry)
    RUN(softmax_argmax_nhwc(logits_nhwc_, dtype, c.Cout_p, dec_out_.rows(), c.Cout, preds, nullptr, maxprob, s_));
}

int FwdOpts::refusal(int training, bool fp32_logits, int H, int W) const {
  if ((maxprob && !preds) || (drows && !rows)) return -1;
  if (ce.labels && (!ce.loss || !ce.ws || ce.kind < 0 || ce.kind > 3)) return -1;
  // two heads asked of one forward, or the CE head of a forward that is not an eval-mode one without fp32 logits
  if (ce.labels && (preds || training || fp32_logits)) return -15;
  // in a training forward f_[5] is still needed as it is (the ReLU mask source of the unit that produced it): the rows go into a
  // second tensor, whose gradient somebody has to take
  if (rows && training && !drows) return -16;
  if (drows && !training) return -17;
  if ((H % 32) || (W % 32)) return -10;
  return 0;
}

int UNet::forward(const float* params, float* buffers, const float* x_nchw, float* logits_nchw, int B, int H, int W,
                  int training, void* ws, size_t ws_bytes, hipStream_t s, const FwdOpts& o) {
  if (const int rc = o.refusal(training, logits_nchw != nullptr, H, W)) return rc;
  f5m_ = Act(); drows_pending_ = nullptr;   // (a backward belongs to the forward just before it)
  // (the caller vouches for the CONTENTS of params / buffers; other addresses are other tensors, whatever it believes)
  reuse_ = o.reuse_constants && !training && last_valid_ && ws == last_ws_ && params == last_params_ && buffers == last_buffers_ &&
           B == last_B_ && H == last_H_ && W == last_W_;
  begin(ws, ws_bytes, s, false);
  fwd_common_begin(params, buffers, B, H, W, training);
  set_lazy_policy();
  if (!reuse_) pack_forward_weights();
  encoder_fwd_impl(x_nchw);
  // metadata fusion (model.py:59-60): f_[5] is the materialised output of layer4's last block, read by decoder block 0 only
  if (o.rows && !training) RUN(add_rowvec_nhwc(dtype, f_[5].p, o.rows, f_[5].N, f_[5].H, f_[5].W, f_[5].C, s_));
  const Act f5 = f_[5];
  if (o.rows && training) {
    // training: the decoder reads a second tensor (as decoder_forward's reads dec_in_), f_[5] stays for the backward
    f5m_ = alloc_act(f5.N, f5.H, f5.W, f5.C);
    RUN(add_rowvec_nhwc_to(dtype, f5.p, o.rows, f5m_.p, f5.N, f5.H, f5.W, f5.C, s_));
    f_[5] = f5m_;
    drows_pending_ = o.drows;
  }
  decoder_fwd_impl(f_);
  f_[5] = f5;
  head_fwd_impl(logits_nchw, o);
  fwd_top_ = ar_.top;
  reuse_ = false;
  last_valid_ = !training && !ar_.err;   // (a training forward lays the arena out differently)
  last_ws_ = ws; last_params_ = params; last_buffers_ = buffers; last_B_ = B; last_H_ = H; last_W_ = W;
  return ar_.err;
}

int UNet::encoder_forward(const float* params, float* buffers, const float* x_nchw, float* const feats[5], int B, int H,
                          int W, int training, void* ws, size_t ws_bytes, hipStream_t s) {
  invalidate_reuse();
  f5m_ = Act(); drows_pending_ = nullptr;
  if ((H % 32) || (W % 32)) return -10;
  begin(ws, ws_bytes, s, false);
  fwd_common_begin(params, buffers, B, H, W, training);
  lazy_ok_ = false;   // split path: the decoder output crosses the boundary, every activation is materialised
  pack_forward_weights();
  encoder_fwd_impl(x_nchw);
  for (int i = 0; i < 5; ++i) {
    const Act& f = f_[i + 1];
    RUN(nhwc_to_nchw_f32(dtype, f.p, feats[i], f.N, f.C, f.H, f.W, f.C, nullptr, s_));
  }
  fwd_top_ = ar_.top;
  return ar_.err;
}

int UNet::decoder_forward(const float* params, float* buffers, const float* const feats[5], float* out_nchw, int B, int H,
                          int W, int training, void* ws, size_t ws_bytes, hipStream_t s) {
  if (const int rc = fwd_resume(params, B, H, W, training, ws, s)) return rc;  // must follow encoder_forward on the same arena
  buffers_ = buffers;
  for (int i = 0; i < 5; ++i) {  // re-import: the caller may have modified feats[-1] (model.py:60)
    Act f = alloc_act(f_[i + 1].N, f_[i + 1].H, f_[i + 1].W, f_[i + 1].C);
    RUN(nchw_f32_to_nhwc(dtype, feats[i], f.p, f.N, f.C, f.H, f.W, f.C, s_));
    dec_in_[i + 1] = f;
  }
  decoder_fwd_impl(dec_in_);
  RUN(nhwc_to_nchw_f32(dtype, dec_out_.p, out_nchw, dec_out_.N, 16, dec_out_.H, dec_out_.W, dec_out_.C, nullptr, s_));
  fwd_top_ = ar_.top;
  return ar_.err;
}

int UNet::head_forward(const float* params, const float* x_nchw, float* logits_nchw, int B, int H, int W, int training,
                       void* ws, size_t ws_bytes, hipStream_t s) {
  if (const int rc = fwd_resume(params, B, H, W, training, ws, s)) return rc;
  Act x = alloc_act(B, H, W, 16);
  RUN(nchw_f32_to_nhwc(dtype, x_nchw, x.p, B, 16, H, W, 16, s_));
  dec_out_ = x;
  head_fwd_impl(logits_nchw, FwdOpts());
  fwd_top_ = ar_.top;
  return ar_.err;
}

// ------------------------------------------------------------------------------------------ backward
// conv1 of every BasicBlock feeds conv2 only, decoder conv1 feeds conv2 only, decoder conv2 feeds the next block's
// upsample (or the head) only: for these units the data-gradient kernel of the single consumer writes the COMPLETE dz,
// so it can also do the first pass of their BatchNorm backward in its epilogue.
int UNet::sole_producer(const Act& a) const {
  if (!a.p) return -1;
  for (int i = 0; i < (int)units_.size(); ++i) {
    const Unit& u = units_[i];
    if (u.out.p != a.p) continue;
    const bool mask_from_y = u.relu && u.res_unit < 0 && !u.res.p;
    if (!mask_from_y) return -1;
    int consumers = 0;
    for (const Unit& v : units_) consumers += (v.in0.p == a.p) + (v.in1.p == a.p) + (v.res.p == a.p);
    for (int f = 1; f <= 5; ++f) consumers += (f_[f].p == a.p);  // encoder features also feed the decoder
    if (a.p == dec_out_.p) consumers += 1;                        // the head
    return consumers == 1 ? i : -1;
  }
  return -1;
}

// Residual units (conv2 of a BasicBlock: out = relu(bn(y) + x)) have two consumers inside the encoder, the next block's
// conv1 and its identity branch.  Backward visits the identity branch first (the BN-backward apply of that block's conv2
// writes dres) and conv1's data gradient last: an ACCUMULATING epilogue that completes the gradient.  Returns the
// producing unit when `a` is such an activation (mask from the ReLU output), else -1.
int UNet::residual_producer(const Act& a) const {
  if (!a.p) return -1;
  for (int f = 1; f <= 5; ++f)
    if (f_[f].p == a.p) return -1;   // encoder features also feed the decoder / the next stage
  if (a.p == dec_out_.p) return -1;
  for (int i = 0; i < (int)units_.size(); ++i) {
    const Unit& u = units_[i];
    if (u.out.p != a.p) continue;
    if (!u.relu || (u.res_unit < 0 && !u.res.p)) return -1;
    int convs_in = 0, res_in = 0;
    for (const Unit& v : units_) { convs_in += (v.in0.p == a.p) + (v.in1.p == a.p); res_in += (v.res.p == a.p); }
    return (convs_in == 1 && res_in == 1) ? i : -1;
  }
  return -1;
}

int UNet::attach_bn_reduce(ConvArgs& a, const Act& target) {
  const int mode = tune("FLAIR_BNR_RES", 1);   // 0: never fuse the reduction of residual units
  int p = sole_producer(target);
  bool from_out = false;
  if (p < 0 && a.accumulate && mode) { p = residual_producer(target); from_out = p >= 0; }
  if (p < 0) return -1;
  Unit& u = units_[p];
  a.bnr_y = u.y.p; a.bnr_scale = u.scale; a.bnr_shift = u.shift; a.bnr_C = u.y.C;
  a.bnr_out = from_out ? u.out.p : nullptr;
  a.bnr_partial = reinterpret_cast<float*>(1);  // provisional, so that the geometry check sees the request
  // only where the data-gradient kernel is MFMA-bound (the extra read of y hides under it); the small-channel
  // halo kernels are HBM-bound and gain nothing over the separate streaming reduction
  if ((a.accumulate && !from_out) || u.y.C != a.out_ld || !conv_tile_epilogue_ok(dtype, a) || !conv_mfma_bound(dtype, a)) {
    a.bnr_y = nullptr; a.bnr_out = nullptr; a.bnr_partial = nullptr; a.bnr_scale = a.bnr_shift = nullptr; a.bnr_C = 0;
    return -1;
  }
  u.bnr.nblk = conv_grid_rows(dtype, a);
  u.bnr.partial = a.bnr_partial = alloc_f((long)u.bnr.nblk * 2 * u.y.C);
  // the halo-GEMM epilogue has the ReLU mask in hand: it stores dz = gradient * mask, and the unit's own backward needs no mask
  // source, no copy for the identity branch and no separate BatchNorm-backward apply pass (unit_backward)
  if (bwd_fuse() && conv_family(dtype, a) == CONV_HG) { a.bnr_mask = 1; u.bnr.masked = true; }
  return p;
}

bool UNet::bwd_fuse() const { return tune("FLAIR_BWD_FUSE", 1) != 0; }

// Gather-form convolution over dy with the flipped / transposed pack, in one of four forms.  The first touch of a gradient buffer
// (grad_of) decides who initialises it and who accumulates, so the calls below happen in the order the backward walk issues them.
DgradDesc UNet::describe_dgrad(const ConvDesc& c, const Act& dy, const Act& in0, const Act& in1, int Hin, int Win, bool upcat,
                               const void* acc_src) {
  DgradDesc d;
  ConvArgs& a = d.a;
  d.form = DgradDesc::DG_PLAIN;
  conv_dgrad_args(a, dtype, ConvInput{dy.p, nullptr, dy.C, 0, 0, dy.N, dy.H, dy.W}, c.R, c.stride, c.pad, Hin, Win, c.Cin_p);
  a.w = ar_.base + c.wd;
  a.out_ld = c.Cin_p;
  if (upcat) {
    // decoder conv1: the input was cat([up2(in0), in1]).  Halo-tile kernels pool / split the gradient in their
    // epilogue; other shapes write the concatenated gradient and run the separate upcat_bwd pass.
    const int C0 = in0.C, C1 = in1.p ? in1.C : 0;
    d.dx0 = grad_of(in0, &d.acc0);
    d.dsk = C1 ? grad_of(in1, &d.acc1) : nullptr;
    a.pool_c0 = C0; a.out = d.dx0; a.out_ld = C0; a.accumulate = d.acc0 ? 1 : 0;
    a.out_skip = d.dsk; a.out_skip_ld = C1; a.skip_accumulate = d.acc1 ? 1 : 0;
    if (conv_tile_epilogue_ok(dtype, a)) {
      d.form = DgradDesc::DG_UPCAT_TILE;
      d.producer = attach_bn_reduce(a, in0);   // the pooled half is the whole gradient of the previous block's output
      // ... or of f5m_, which no unit produces: the row sums need it complete and UNMASKED, so a fused reduction / mask on it
      // (there is none today: attach_bn_reduce finds no producer) is an error, never silently wrong sums
      if (drows_pending_ && in0.p == f5m_.p && (a.bnr_partial || a.bnr_mask) && !ar_.err) ar_.err = -18;
    } else {
      d.form = DgradDesc::DG_UPCAT_SPLIT;
      d.dcat = alloc((size_t)dy.rows() * (C0 + C1) * dtype_size(dtype));
      a.pool_c0 = 0; a.out_skip = nullptr; a.out = d.dcat; a.out_ld = C0 + C1; a.accumulate = 0;
    }
    return d;
  }
  bool acc = false;
  a.out = grad_of(in0, &acc);
  a.accumulate = acc ? 1 : 0;
  if (acc_src) {
    // the identity branch's share arrives as a tensor of its own (the masked gradient of the block's output)
    ConvArgs t = a;
    t.accumulate = 1; t.acc_src = acc_src;
    if (!acc && conv_acc_src_ok(dtype, t)) {
      a = t;
    } else {   // some other kernel takes this layer: put the share into the buffer first
      if (acc) RUN(ew_add(dtype, a.out, acc_src, in0.elems(), s_));
      else if (!ar_.dry && !ar_.err && hipMemcpyAsync(a.out, acc_src, (size_t)in0.elems() * dtype_size(dtype), hipMemcpyDeviceToDevice, s_) != hipSuccess) ar_.err = -14;
      a.accumulate = 1;
    }
  }
  d.producer = attach_bn_reduce(a, in0);
  const bool doubled = c.stride == 2 && a.Hout == 2 * dy.H && a.Wout == 2 * dy.W;
  if (doubled && (c.parity_dgrad() || (c.R == 1 && c.S == 1 && c.pad == 0 && a.accumulate))) {
    // stride-2 data gradient by output parity class: stride-1 convolutions over dY, stores interleaved into dX.
    // A 1x1 stride-2 layer only reaches the (even, even) pixels; when accumulating, the other classes add nothing.
    d.form = DgradDesc::DG_PARITY;
    conv_parity_args(a, dtype, c.R);
    if (a.ncls) {   // the packs of the four classes (UNet::begin)
      a.w = ar_.base + c.wd_cls[3];
      for (int cls = 0; cls < 4; ++cls) a.cls_w[cls] = ar_.base + c.wd_cls[cls];
    }
  }
  return d;
}

// Backward of one conv->BN->(+res)->ReLU unit.  g.dout = gradient w.r.t. u.out (or w.r.t. the BN output when the unit was not
// materialised).  Produces parameter gradients, optionally the residual-branch gradient dz (g.dres) and the input gradient (into
// grad_of(in0)).
//
// FLAIR_BWD_FUSE (bwd_fuse(), default on): the halo-GEMM data gradient that completed dout stored it masked by this unit's ReLU
// (BnReduce::masked), so dout is dz already.  bn_bwd_apply then needs no mask source (no read of `out` for residual units, no
// recomputation of relu'(y) for the others), and the identity branch of a BasicBlock takes dz as it stands (UnitBwd::acc_src of
// the block's conv1) instead of a copy written as dres.
void UNet::unit_backward(int ui, const UnitBwd& g) {
  Unit& u = units_[ui];
  const ConvDesc& c = convs[u.conv];
  const BnDesc& b = bns[u.bn];
  const long rows = u.y.rows();
  // ---- 1. the hand-off: what the consumer's data gradient already did of this unit's BatchNorm backward
  const BnReduce pre = u.bnr.take();
  const bool masked = pre.masked && pre.nblk > 0;
  float* partial = pre.nblk > 0 ? pre.partial : alloc_f((long)bn_bwd_blocks(rows) * 2 * b.C);
  float* coef = alloc_f(3 * b.C);
  // ReLU mask: units without a residual recompute it from y (out > 0 <=> y*scale + shift > 0) and skip
  // reading the activation tensor in both backward passes
  const bool mask_from_y = u.relu && u.res_unit < 0 && !u.res.p;
  // A 16 -> 16 unit whose backward may run as ONE kernel (bwd_halo16.hip), which forms dy while it stages dz and y: no dy tensor
  // then.  Decided in step 4, once the data gradient is described; until then dout stands in for dy in the descriptors
  const bool cand16 = dtype == DT_BF16 && g.dgrad && !g.dres && !g.upcat && mask_from_y && pre.nblk > 0 && !masked && !g.acc_src &&
                      c.R == 3 && c.stride == 1 && c.pad == 1 && u.y.C == 16 && b.C == 16 && c.Cin_p == 16 && !u.in1.p && !u.up0 &&
                      u.in0.lz_scale;
  Act dy = u.y;   // the gradient of the pre-BatchNorm tensor
  dy.p = cand16 ? const_cast<void*>(g.dout) : alloc((size_t)u.y.elems() * dtype_size(dtype));
  // ---- 2. weight gradient (described first: a unit without a data gradient may fold the BatchNorm-backward apply into it)
  WgradArgs w;
  wgrad_args(w, conv_input(u.in0, u.in1, u.up0), c.R, c.stride, c.pad, dy.p, u.y.C, c.Cout, grads_ + c.w_off, c.Cin);
  // the stem: dy feeds nothing but the weight gradient, whose kernel stages it chunk by chunk — it applies the affine itself and
  // the tensor is never written (bn_bwd_apply: 804 MB of traffic for a 268 MB operand read once)
  const bool fuse_apply = !g.dgrad && !g.dres && mask_from_y && wgrad_bnapply_fusable(dtype, w);
  w.in_scale = u.in0.lz_scale; w.in_shift = u.in0.lz_shift;
  // ---- 3. data gradient
  DgradDesc d;
  if (g.dgrad) d = describe_dgrad(c, dy, u.in0, u.in1, w.Hin, w.Win, g.upcat, g.acc_src);
  // ---- 4. the fusion
  const bool fuse16 = cand16 && d.form == DgradDesc::DG_PLAIN && bwd16_ok(BWD16_UNIT, d.a, w, d.producer);
  if (cand16 && !fuse16) {   // the separate kernels after all: they need the tensor
    dy.p = alloc((size_t)u.y.elems() * dtype_size(dtype));
    w.dy = dy.p; d.a.src0 = dy.p;
  }
  // ---- 5. BatchNorm backward
  // a masked gradient needs no mask source in the apply pass: the residual units' read of `out` and the others' recomputation
  // of relu'(y) go (bn_backward still needs one on paper when it runs the reduction itself, which it does not here: pre.nblk > 0)
  const bool nomask = masked && !g.dres && bwd_fuse();
  RUN(bn_backward(dtype, g.dout, (u.relu && !mask_from_y && !nomask) ? u.out.p : nullptr, u.y.p, u.mean, u.invstd, params_ + b.g_off,
                  rows, b.C, partial, coef, grads_ + b.g_off, grads_ + b.b_off, 0, (fuse_apply || fuse16) ? nullptr : dy.p, g.dres,
                  g.dres_acc ? 1 : 0, (mask_from_y && !nomask) ? u.scale : nullptr, (mask_from_y && !nomask) ? u.shift : nullptr,
                  pre.nblk, nomask ? 1 : 0, s_));
  // ---- 6. launches
  if (fuse16) {   // bn_backward above ran the finalize only: the kernel applies k1*dz*m + k2*y + k3 itself
    Bwd16Args f;
    memset(&f, 0, sizeof(f));
    f.g = g.dout; f.gy = u.y.p; f.gcoef = coef; f.gmsc = u.scale; f.gmsh = u.shift;
    bwd16_run(f, d.a, w, u.in0, d.producer);
    return;
  }
  if (fuse_apply) { w.dy = g.dout; w.fuse_y = u.y.p; w.fuse_coef = coef; w.fuse_msc = u.scale; w.fuse_msh = u.shift; }
  w.cus = side_cus();
  w.partial = (float*)alloc(wgrad_workspace_bytes(dtype, w));
  {
    hipStream_t ws = wgrad_stream();   // dy is complete on s_; nothing later on s_ writes what this kernel reads
    RUN(launch_wgrad(dtype, w, ws));
  }
  if (d.form == DgradDesc::DG_NONE) return;
  RUN(launch_conv(dtype, d.a, s_));
  if (d.form == DgradDesc::DG_UPCAT_SPLIT)
    RUN(upcat_bwd(dtype, d.dcat, d.dx0, d.acc0 ? 1 : 0, d.dsk, d.acc1 ? 1 : 0, u.y.N, u.y.H, u.y.W, u.in0.C, u.in1.p ? u.in1.C : 0, s_));
}

// The fused backward of a 16 -> 16 layer (bwd_halo16.hip) in place of its data-gradient, weight-gradient and (unit flavour)
// BatchNorm-backward apply launches.  It carries the data gradient, so it runs on the caller's stream, and the slab reduce follows
// it there: the weight gradient is complete on s_ and the side stream is not touched.
// bwd16_fusable, and the fused kernel forms every per-workgroup sum as the separate kernels would: its grid is the separate weight
// gradient's, and the partial columns the separate data gradient was sized for (attach_bn_reduce) are that grid's or one per tile.
// Where the two separate grids disagree the layer keeps its three kernels, unless FLAIR_BWD16_WGS asks for a grid of its own.
bool UNet::bwd16_ok(int flavour, const ConvArgs& a, const WgradArgs& w, int producer) const {
  if (producer < 0 || !bwd16_fusable(dtype, flavour, a, w)) return false;
  if (tune("FLAIR_BWD16_WGS", 0) > 0) return true;
  const int nblk = units_[producer].bnr.nblk, grid = bwd16_grid(w);
  if (nblk == grid || nblk == (long)a.N * a.Hout * a.Wout / 256) return true;
  // the two separate kernels' occupancy answers disagree (another compiler or runtime): the layer keeps its three kernels, and says so
  // once, since a speed-up that turns itself off silently is a regression nobody sees (tests/test_gpu_bwd16_fuse.py runs a step at
  // default grids above the grid size and asserts that the fused kernels are in it)
  static bool told = false;
  if (!told && !ar_.dry) {
    told = true;
    fprintf(stderr, "flair: fused 16-channel backward not used: the data gradient's %d partial columns are not the weight gradient's grid "
                    "of %d workgroups (FLAIR_BWD16_WGS overrides)\n", nblk, grid);
  }
  return false;
}

void UNet::bwd16_run(Bwd16Args& f, const ConvArgs& a, const WgradArgs& w, const Act& x, int producer) {
  Unit& up = units_[producer];
  // the reduction's partial columns: one per workgroup of THIS kernel; one per tile where the separate data gradient would have run
  // one tile per workgroup (small inputs) keeps that layout
  const int grid = bwd16_grid(w);
  const long ntiles = (long)a.N * a.Hout * a.Wout / 256;
  // (only under FLAIR_BWD16_WGS: by default bwd16_ok() has seen to it that the columns attach_bn_reduce sized are these)
  if (up.bnr.nblk != grid && up.bnr.nblk != ntiles) { up.bnr.partial = alloc_f((long)grid * 2 * up.y.C); up.bnr.nblk = grid; }
  f.x = x.p; f.in_scale = w.in_scale; f.in_shift = w.in_shift;
  f.w = a.w; f.Kpad = a.Kpad; f.dx = a.out;
  f.bnr_scale = a.bnr_scale; f.bnr_shift = a.bnr_shift; f.bnr_partial = up.bnr.partial; f.bnr_C = a.bnr_C; f.bnr_cols = up.bnr.nblk;
  f.slabs = (float*)alloc(bwd16_workspace_bytes(grid));
  f.grid = grid;
  f.dw = w.dw; f.Cout = w.Cout; f.Cin_real = w.Cin_real;
  f.N = a.N; f.H = a.Hout; f.W = a.Wout;
  RUN(launch_bwd16(f, s_));
}

void UNet::head_bwd_impl(const void* dl) {
  const ConvDesc& c = convs.back();
  Act none;
  WgradArgs w;
  wgrad_args(w, conv_input(dec_out_, none, false), c.R, c.stride, c.pad, dl, c.Cout_p, c.Cout, grads_ + c.w_off, c.Cin);
  w.in_scale = dec_out_.lz_scale; w.in_shift = dec_out_.lz_shift;
  // the data gradient, described before anything is launched
  Act dy;
  dy.p = const_cast<void*>(dl); dy.N = dec_out_.N; dy.H = dec_out_.H; dy.W = dec_out_.W; dy.C = c.Cout_p;
  DgradDesc d = describe_dgrad(c, dy, dec_out_, none, dec_out_.H, dec_out_.W, false, nullptr);
  // bias gradient = column sums of dl: inside the weight-gradient kernel where it stages dl anyway, else a pass of its own
  const bool fuse_db = wgrad_dbias_fusable(dtype, w);
  const bool fuse16 = bwd16_ok(BWD16_HEAD, d.a, w, d.producer);
  if (fuse_db) { w.dbias = grads_ + c.b_off; w.dbias_partial = alloc_f((long)WGRAD_DBIAS_ROWS * c.Cout_p); }
  if (fuse16) {
    Bwd16Args f;
    memset(&f, 0, sizeof(f));
    f.g = dl; f.dbias = w.dbias; f.dbias_partial = w.dbias_partial;
    bwd16_run(f, d.a, w, dec_out_, d.producer);
  } else {
    w.partial = (float*)alloc(wgrad_workspace_bytes(dtype, w));
    hipStream_t ws = wgrad_stream();
    RUN(launch_wgrad(dtype, w, ws));
  }
  if (!fuse_db) {
    const long rows = dec_out_.rows();
    float* partial = alloc_f((long)bn_bwd_blocks(rows) * c.Cout_p);
    RUN(colsum(dtype, dl, rows, c.Cout_p, c.Cout, partial, grads_ + c.b_off, s_));
  }
  if (!fuse16) RUN(launch_conv(dtype, d.a, s_));
}

void UNet::decoder_bwd_impl() {
  for (int i = 4; i >= 0; --i) {
    const int u1 = dec_units_begin_ + 2 * i, u2 = u1 + 1;
    unit_backward(u2, {grad_peek(units_[u2].out)});
    // conv1: gradient w.r.t. the virtual concat: 2x2 sum-pool -> x, rest -> skip (fused in the epilogue)
    UnitBwd g1{grad_peek(units_[u1].out)};
    g1.upcat = true;
    unit_backward(u1, g1);
  }
}

void UNet::encoder_bwd_impl() {
  // walk the encoder units backwards; layout per block: u1, [ud], u2
  int ui = enc_units_end_ - 1;
  for (int L = 3; L >= 0; --L) {
    for (int b = kBlocks[L] - 1; b >= 0; --b) {
      const bool ds = (b == 0 && L > 0);
      const int u2 = ui, ud = ds ? ui - 1 : -1, u1 = ds ? ui - 2 : ui - 1;
      ui = u1 - 1;
      const Act& X = units_[u1].in0;
      const void* dO = grad_peek(units_[u2].out);
      // dO stored masked by the block's last ReLU (the data gradient that completed it, BnReduce::masked): it IS dz2, the
      // identity / downsample branch takes it as it stands and bn_bwd_apply need not write a copy
      const bool dz_ready = units_[u2].bnr.masked && units_[u2].bnr.nblk > 0 && bwd_fuse();
      UnitBwd g2{dO};
      if (!dz_ready && !ds) {   // identity branch: dX (+)= dz2
        g2.dres = grad_of(X, &g2.dres_acc);
      } else if (!dz_ready) {   // downsample branch: dz2 as a tensor of its own
        g2.dres = alloc((size_t)units_[u2].y.elems() * dtype_size(dtype));
      }
      unit_backward(u2, g2);
      UnitBwd g1{grad_peek(units_[u1].out)};
      if (dz_ready && !ds) g1.acc_src = dO;   // conv1's data gradient: dX = dz2 + its own result
      unit_backward(u1, g1);
      // conv1 first: its stride-2 data gradient writes every pixel of dX, so the 1x1 stride-2 downsample branch
      // (no ReLU) then only accumulates into the (even, even) ones
      if (ds) unit_backward(ud, {dz_ready ? dO : g2.dres});
    }
    stage_done(L + 1);
  }
  // maxpool: d f1 (+)= scatter(d pool)
  bool acc = false;
  void* df1 = grad_of(f_[1], &acc);
  {
    // the max-pool backward completes the gradient of the stem's ReLU output: it also runs the first pass of the stem's
    // BatchNorm backward on it (mask from y; the stem has no residual)
    Unit& u0 = units_[0];
    const bool fuse = tune("FLAIR_POOL_BNR", 1) && u0.relu && u0.res_unit < 0 && !u0.res.p && u0.y.C == 64;
    float* part = nullptr;
    const int nblk = B_ * f_[1].H;
    if (fuse) { part = alloc_f((long)nblk * 2 * u0.y.C); u0.bnr.partial = part; u0.bnr.nblk = nblk; }
    RUN(maxpool3x3s2_bwd(dtype, grad_peek(pool_), pool_idx_, df1, acc ? 1 : 0, B_, f_[1].H, f_[1].W, 64, s_,
                         fuse ? u0.y.p : nullptr, fuse ? u0.scale : nullptr, fuse ? u0.shift : nullptr, part));
  }
  UnitBwd g0{df1};
  g0.dgrad = false;   // stem: no data gradient
  unit_backward(0, g0);
  stage_done(0);
}

void UNet::stage_done(int stage) {
  const bool listened = stage_events_ && stage_events_[stage] && !ar_.dry && !ar_.err;
  if (stage == 0) side_join();   // end of backward: everything is back on the caller's stream
  if (!listened) return;
  hipEvent_t ev = (hipEvent_t)stage_events_[stage];
  if (stage != 0 && side_pending_) {
    // The stage's weight gradients live on the side stream, the rest on s_.  Neither stream may wait for the other
    // here (that would serialise the weight-gradient tails behind the data-gradient chain six times per step): a third
    // stream waits for the current position of both and carries the stage event, which fires when both are done.
    if (!note_) {
      // LOW priority, like the side stream: a stream of the caller's priority level may share the caller's hardware queue, and its
      // wait for the side stream's position would then hold back every kernel the caller queues behind it
      if (make_stream(&note_, tune("FLAIR_NOTE_PRIO", 1)) != hipSuccess) note_ = nullptr;
    }
    if (note_) {
      hipEvent_t e1 = fork_ev_[fork_next_++ % fork_ev_.size()];
      hipEvent_t e2 = fork_ev_[fork_next_++ % fork_ev_.size()];
      hipError_t e = hipEventRecord(e1, s_);
      if (e == hipSuccess) e = hipEventRecord(e2, side_);
      if (e == hipSuccess) e = hipStreamWaitEvent(note_, e1, 0);
      if (e == hipSuccess) e = hipStreamWaitEvent(note_, e2, 0);
      if (e == hipSuccess) e = hipEventRecord(ev, note_);
      if (e != hipSuccess) ar_.err = (int)e;
      return;
    }
    side_join();   // no third stream: fold the side stream back in and record on s_
  }
  const hipError_t e = hipEventRecord(ev, s_);
  if (e != hipSuccess) ar_.err = (int)e;
}

int UNet::bwd_begin(const float* params, float* grads, void* ws, hipStream_t s) {
  invalidate_reuse();
  if (ws != ar_.base || !training_) return -11;
  s_ = s; params_ = params; grads_ = grads;
  pack_dgrad_weights();
  return 0;
}

// the fp32 NCHW logit gradient in the head's layout: NHWC rows of Cout_p columns of T
const void* UNet::import_dlogits(const float* dlogits_nchw) {
  const int ld = convs.back().Cout_p;
  void* t = alloc((size_t)dec_out_.rows() * ld * dtype_size(dtype));
  RUN(nchw_f32_to_nhwc(dtype, dlogits_nchw, t, B_, classes, H_, W_, ld, s_));
  return t;
}

int UNet::backward(const float* params, const float* dlogits_nchw, const void* dlogits_nhwc, float* grads, void* ws,
                   size_t ws_bytes, hipStream_t s, void* const* stage_events) {
  if (const int rc = bwd_begin(params, grads, ws, s)) return rc;
  ar_.release(fwd_top_);
  stage_events_ = stage_events;
  gbufs_.clear();
  head_bwd_impl(dlogits_nhwc ? dlogits_nhwc : import_dlogits(dlogits_nchw));
  stage_done(6);
  decoder_bwd_impl();
  stage_done(5);   // (bucket 5 is the decoder's weights; the row sums below belong to no bucket and stay behind its event)
  if (drows_pending_) {
    // decoder block 0's conv1 wrote its pooled half into the buffer keyed by f5m_: the complete gradient of the row add's output.
    // Its row sums are d rows; the values are also the gradient of f_[5], which the encoder walk asks for under that key
    float* const drows = drows_pending_;
    drows_pending_ = nullptr;
    void* g = grad_peek(f5m_);
    if (!g) { if (!ar_.err) ar_.err = -11; }
    else {
      RUN(rowvec_grad_nhwc(dtype, g, drows, f5m_.N, f5m_.H, f5m_.W, f5m_.C, s_));
      for (auto& gb : gbufs_)
        if (gb.act == f5m_.p) gb.act = f_[5].p;
    }
  }
  encoder_bwd_impl();
  stage_events_ = nullptr;
  return ar_.err;
}

int UNet::head_backward(const float* params, const float* dlogits_nchw, float* dx_nchw, float* grads, void* ws,
                        size_t ws_bytes, hipStream_t s) {
  if (const int rc = bwd_begin(params, grads, ws, s)) return rc;
  head_bwd_impl(import_dlogits(dlogits_nchw));
  side_join();
  RUN(nhwc_to_nchw_f32(dtype, grad_peek(dec_out_), dx_nchw, B_, 16, H_, W_, 16, nullptr, s_));
  return ar_.err;
}

int UNet::decoder_backward(const float* params, const float* dout_nchw, float* const dfeats[5], float* grads, void* ws,
                           size_t ws_bytes, hipStream_t s) {
  if (const int rc = bwd_begin(params, grads, ws, s)) return rc;
  const Act& out = units_.back().out;  // decoder output (last unit)
  bool acc = false;
  void* g = grad_of(out, &acc);
  RUN(nchw_f32_to_nhwc(dtype, dout_nchw, g, out.N, 16, out.H, out.W, out.C, s_));
  decoder_bwd_impl();
  side_join();
  for (int i = 0; i < 5; ++i) {
    const Act& f = dec_in_[i + 1];
    RUN(nhwc_to_nchw_f32(dtype, grad_peek(f), dfeats[i], f.N, f.C, f.H, f.W, f.C, nullptr, s_));
  }
  return ar_.err;
}

int UNet::encoder_backward(const float* params, const float* const dfeats[5], float* grads, void* ws, size_t ws_bytes,
                           hipStream_t s) {
  if (const int rc = bwd_begin(params, grads, ws, s)) return rc;
  for (int i = 0; i < 5; ++i) {
    const Act& f = f_[i + 1];
    bool acc = false;
    void* g = grad_of(f, &acc);
    if (acc) { if (!ar_.err) ar_.err = -12; }
    RUN(nchw_f32_to_nhwc(dtype, dfeats[i], g, f.N, f.C, f.H, f.W, f.C, s_));
  }
  encoder_bwd_impl();
  return ar_.err;
}

// Upper bound of the arena: dry run of the split sequence (superset of the fused one) on a SCRATCH executor, so that
// sizing a workspace between a training forward and its backward (an eval forward does that) leaves the recorded graph
// of the live handle alone.
// training == 2: the arena of the whole-model training step as forward() + backward() run it under the current tune state (lazy
// BatchNorm, fused 16-channel backward: no dy tensor for the layers that take it) — a tight bound for a caller that runs nothing
// else on the workspace; training == 0 / 1: the split sequence, the upper bound for every entry point
size_t UNet::workspace_bytes(int B, int H, int W, int training) const {
  UNet scratch(in_channels, classes, dtype);
  return training == 2 ? scratch.plan_step_bytes(B, H, W) : scratch.plan_bytes(B, H, W, training);
}

// Dry run of forward(training, no fp32 logits) and backward() in their own order.  Counted whether the call uses them or not: the
// second bottleneck tensor of a forward with metadata rows, and the NHWC copy backward() makes of an fp32 NCHW logit gradient.
size_t UNet::plan_step_bytes(int B, int H, int W) {
  begin(nullptr, 0, nullptr, true);
  fwd_common_begin(nullptr, nullptr, B, H, W, 1);
  set_lazy_policy();
  encoder_fwd_impl(nullptr);
  alloc_act(f_[5].N, f_[5].H, f_[5].W, f_[5].C);
  decoder_fwd_impl(f_);
  head_fwd_impl(nullptr, FwdOpts());
  grads_ = nullptr;
  head_bwd_impl(import_dlogits(nullptr));
  decoder_bwd_impl();
  encoder_bwd_impl();
  return plan_end();
}

size_t UNet::plan_end() {
  const size_t need = ar_.top + (1 << 20);
  ar_.dry = false;
  ar_.base = nullptr;
  units_.clear();
  gbufs_.clear();
  return need;
}

size_t UNet::plan_bytes(int B, int H, int W, int training) {
  begin(nullptr, 0, nullptr, true);
  fwd_common_begin(nullptr, nullptr, B, H, W, training);
  lazy_ok_ = false;   // the materialised (split) sequence is the upper bound
  encoder_fwd_impl(nullptr);
  for (int i = 1; i <= 5; ++i) dec_in_[i] = alloc_act(f_[i].N, f_[i].H, f_[i].W, f_[i].C);
  decoder_fwd_impl(dec_in_);
  dec_out_ = alloc_act(B, H, W, 16);
  head_fwd_impl(nullptr, FwdOpts());
  if (training) {
    grads_ = nullptr;
    head_bwd_impl(import_dlogits(nullptr));
    bool acc;
    grad_of(units_.back().out, &acc);
    decoder_bwd_impl();
    for (int i = 1; i <= 5; ++i) grad_of(f_[i], &acc);
    encoder_bwd_impl();
  }
  return plan_end();
}

}  // namespace flair
