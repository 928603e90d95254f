// What the native transformer inference executors (segformer.hip, upernet.hip) share on the host side: the tensor table, the
// Linear / LayerNorm records, the workspace arena with its cache of packed weights, and the implicit-GEMM launch.
#pragma once
#include <string>
#include <vector>

#include "arena.h"
#include "ops.h"

namespace flair {

struct SfTensor {
  std::string name;
  int ndim;
  long shape[4];
  long offset;   // floats into the flat buffer
  int kind;      // 0 parameter, 1 BatchNorm running statistic
};

struct SfLin {   // Linear (k = 1) or Conv2d(k, stride, pad) as an implicit GEMM
  int cin, cout, k, stride, pad, cin_p;
  long w_off, b_off;
  int Kpad, rows;
  size_t packed = 0;
};
struct SfNorm { int C; long g_off, b_off; };
struct SfPart { long w_off, b_off; };   // one projection of a row-stacked product (fuse_rows)

class TfExec {
 public:
  int dtype;
  std::vector<SfTensor> tensors;
  long n_params = 0;
  // The packed weights at the front of the workspace are reused while `params` and `ws` stay the same pointers; call this after
  // changing the parameter buffer's contents in place.
  void weights_changed() { cache_ok_ = false; }

 protected:
  explicit TfExec(int dt) : dtype(dt) {}
  std::vector<SfLin> lins;
  std::vector<SfNorm> norms;
  long add_tensor(const std::string& name, int ndim, long d0, long d1, long d2, long d3, int kind);
  SfLin make_lin(int cin, int cout, int k, int stride, int pad) const;   // the geometry alone: no tensors, not in `lins`
  int add_lin(const std::string& name, int cin, int cout, int k, int stride, int pad, bool bias);   // "...#conv": a 4-d weight
  int add_ln(const std::string& name, int C);

  // ---- the arena of one run(); scratch is released with ar_.release(mark), and the plan is the high-water mark
  Arena ar_;
  hipStream_t s_ = nullptr;
  const float* params_ = nullptr;
  void* alloc(size_t bytes) { return ar_.get(bytes); }
  // Resets the arena.  True: the weight-only front of the arena (everything allocated before the first shape-dependent tensor)
  // is still valid from the last run — same parameter buffer, workspace and mode_key, no weights_changed() since.
  bool begin(const float* params, void* ws, size_t ws_bytes, hipStream_t s, bool dry, int mode_key);
  int end();                                                   // closes the run: the plan, the cache fields; returns the error
  size_t planned(int dry_rc) const { return dry_rc ? 0 : need_; }   // workspace_bytes() of a finished dry run

  // ---- the weight-only front of the arena
  void pack_lins(bool fresh);   // a packed copy of every lins[i] (L.packed); packs them unless fresh
  // n projections of G.cout / n rows each over the same input as ONE product of geometry G: allocates the packed weight (its arena
  // offset is returned) and then the concatenated fp32 bias; unless fresh, copies the biases and queues the packs for flush_packs()
  size_t fuse_rows(const SfLin& G, const SfPart* parts, int n, bool fresh, float** bias);
  void flush_packs();

  // one product on the implicit-GEMM kernel; wpacked / bias override L's own packed weight and bias
  void gemm(const SfLin& L, const void* in, int B, int Hin, int Win, void* out, int out_ld, const void* res, const float* oscale,
            const float* oshift, int relu, float* out_nchw, int gelu = 0, const void* wpacked = nullptr, const float* bias = nullptr);

 private:
  size_t need_ = 0;
  PackTable packs_;
  int mode_key_ = 0;
  bool cache_ok_ = false;
  const float* cache_params_ = nullptr;
  const void* cache_ws_ = nullptr;
  int cache_mode_ = -1;
};

}  // namespace flair
