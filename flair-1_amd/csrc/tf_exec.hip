// Host-side core of the transformer inference executors (see tf_exec.h).  No kernels here: every launch goes to misc.hip
// (weight packing) or conv_igemm.hip (the products).
#include "tf_exec.h"
#include "conv_args.h"

namespace flair {

long TfExec::add_tensor(const std::string& name, int ndim, long d0, long d1, long d2, long d3, int kind) {
  SfTensor t;
  t.name = name; t.ndim = ndim; t.shape[0] = d0; t.shape[1] = d1; t.shape[2] = d2; t.shape[3] = d3; t.kind = kind;
  long n = 1;
  for (int i = 0; i < ndim; ++i) n *= t.shape[i];
  t.offset = n_params;
  n_params = round_up(n_params + n, 4);   // every tensor 16-byte aligned in the flat buffer
  tensors.push_back(t);
  return t.offset;
}

SfLin TfExec::make_lin(int cin, int cout, int k, int stride, int pad) const {
  SfLin L;
  L.cin = cin; L.cout = cout; L.k = k; L.stride = stride; L.pad = pad;
  L.cin_p = (int)round_up(cin, 8);
  L.w_off = -1; L.b_off = -1;
  L.Kpad = conv_kpad(dtype, k * k * L.cin_p);   // whole K steps of the kernel
  L.rows = conv_weight_rows_pad(cout);
  return L;
}

int TfExec::add_lin(const std::string& name, int cin, int cout, int k, int stride, int pad, bool bias) {
  SfLin L = make_lin(cin, cout, k, stride, pad);
  const bool conv = name.find("#conv") != std::string::npos;
  const std::string base = name.substr(0, name.find('#'));
  L.w_off = conv ? add_tensor(base + ".weight", 4, cout, cin, k, k, 0) : add_tensor(base + ".weight", 2, cout, cin, 1, 1, 0);
  L.b_off = bias ? add_tensor(base + ".bias", 1, cout, 1, 1, 1, 0) : -1;
  lins.push_back(L);
  return (int)lins.size() - 1;
}

int TfExec::add_ln(const std::string& name, int C) {
  SfNorm n;
  n.C = C;
  n.g_off = add_tensor(name + ".weight", 1, C, 1, 1, 1, 0);
  n.b_off = add_tensor(name + ".bias", 1, C, 1, 1, 1, 0);
  norms.push_back(n);
  return (int)norms.size() - 1;
}

bool TfExec::begin(const float* params, void* ws, size_t ws_bytes, hipStream_t s, bool dry, int mode_key) {
  ar_.reset(ws, ws_bytes, dry);
  s_ = s; params_ = params; mode_key_ = mode_key;
  packs_.n = 0;
  return !dry && cache_ok_ && cache_params_ == params && cache_ws_ == ws && cache_mode_ == mode_key;
}

int TfExec::end() {
  need_ = ar_.peak + (1 << 20);
  if (!ar_.dry) { cache_ok_ = ar_.err == 0; cache_params_ = params_; cache_ws_ = ar_.base; cache_mode_ = mode_key_; }
  return ar_.err;
}

void TfExec::flush_packs() {
  if (packs_.n) RUN(pack_weights_all(dtype, params_, ar_.base, packs_, s_));
  packs_.n = 0;
}

void TfExec::pack_lins(bool fresh) {
  const size_t es = dtype_size(dtype);
  for (auto& L : lins) { L.packed = ar_.top; alloc((size_t)L.rows * L.Kpad * es); }
  if (fresh || ar_.dry) return;
  for (const SfLin& L : lins) {
    if (packs_.n == PackTable::MAX) flush_packs();
    packs_.d[packs_.n++] = pack_desc(L.w_off, L.packed, L.cout, L.cin, L.k, L.cin_p, L.rows, L.Kpad, 0);
  }
  flush_packs();
}

size_t TfExec::fuse_rows(const SfLin& G, const SfPart* parts, int n, bool fresh, float** bias) {
  const size_t es = dtype_size(dtype), off = ar_.top;
  const int C = G.cout / n;
  alloc((size_t)G.rows * G.Kpad * es);
  *bias = (float*)alloc((size_t)n * C * 4);
  if (fresh || ar_.dry) return off;
  for (int part = 0; part < n; ++part) {
    packs_.d[packs_.n++] = pack_desc(parts[part].w_off, off + (size_t)part * C * G.Kpad * es, C, G.cin, 1, G.cin_p,
                                     part + 1 < n ? C : G.rows - (n - 1) * C, G.Kpad, 0);   // the last part carries the padding rows
    if (!ar_.err && hipMemcpyAsync(*bias + part * C, params_ + parts[part].b_off, (size_t)C * 4, hipMemcpyDeviceToDevice, s_) != hipSuccess)
      ar_.err = -101;
  }
  if (packs_.n + n > PackTable::MAX) flush_packs();   // room for the next call's n
  return off;
}

void TfExec::gemm(const SfLin& L, const void* in, int B, int Hin, int Win, void* out, int out_ld, const void* res, const float* oscale,
                  const float* oshift, int relu, float* out_nchw, int gelu, const void* wpacked, const float* bias) {
  ConvArgs a;
  conv_fwd_args(a, dtype, ConvInput{in, nullptr, L.cin_p, 0, 0, B, Hin, Win}, L.k, L.stride, L.pad, L.cout);
  a.w = wpacked ? wpacked : ar_.base + L.packed;
  a.bias = bias ? bias : L.b_off >= 0 ? params_ + L.b_off : nullptr;
  a.out = out; a.out_ld = out_ld; a.out_nchw = out_nchw;
  a.ores = res; a.oscale = oscale; a.oshift = oshift; a.orelu = relu; a.ogelu = gelu;
  RUN(launch_conv(dtype, a, s_));
}

}  // namespace flair
