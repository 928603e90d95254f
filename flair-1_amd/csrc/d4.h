// The D4 packing every kernel of the library shares (data_feed.pack_d4): bit 0 V-flip, bit 1 H-flip, bits 2-3 the rot90 count k;
// the code means rot90^k(hflip(vflip(a))) with numpy's counter-clockwise rot90 (src/flair/tasks_utils.py:37-41).  An odd k needs
// H == W.
#pragma once
#include <hip/hip_runtime.h>

namespace flair {

// where output pixel (i, j) of rot90^k(hflip(vflip(a))) comes from (numpy: rot90 is counter-clockwise,
// r[i][j] = m[j][N-1-i]); flags: bit0 V-flip, bit1 H-flip, bits 2-3 k
__device__ __forceinline__ void d4_source(int flags, int i, int j, int H, int W, int& si, int& sj) {
  const int k = (flags >> 2) & 3;
  if (k == 0) { si = i; sj = j; }
  else if (k == 1) { si = j; sj = W - 1 - i; }
  else if (k == 2) { si = H - 1 - i; sj = W - 1 - j; }
  else { si = H - 1 - j; sj = i; }
  if (flags & 2) sj = W - 1 - sj;
  if (flags & 1) si = H - 1 - si;
}

// the inverse: the output pixel (i, j) that d4_source sends to source pixel (si, sj)
__device__ __forceinline__ void d4_dest(int flags, int si, int sj, int H, int W, int& i, int& j) {
  const int k = (flags >> 2) & 3;
  const int a = (flags & 1) ? H - 1 - si : si, b = (flags & 2) ? W - 1 - sj : sj;
  if (k == 0) { i = a; j = b; }
  else if (k == 1) { i = W - 1 - b; j = a; }
  else if (k == 2) { i = H - 1 - a; j = W - 1 - b; }
  else { i = b; j = H - 1 - a; }
}

}  // namespace flair
