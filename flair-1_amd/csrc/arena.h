// The workspace arena of every host-side executor (unet.hip, tf_exec.hip) and operator entry point (capi.hip): a bump allocator
// over one caller-owned buffer, and the error slot of the run that uses it.
#pragma once
#include <stddef.h>

namespace flair {

struct Arena {
  unsigned char* base = nullptr;
  size_t cap = 0, top = 0, peak = 0;
  bool dry = false;   // sizing run: nothing is launched, `base` is never dereferenced
  int err = 0;        // first error of the run: -100 when the arena overflowed, else what a launch returned (RUN)
  Arena() = default;
  Arena(void* ws, size_t bytes) { reset(ws, bytes, false); }
  // dry runs use a fake base so that tensors keep distinct identities
  void reset(void* ws, size_t bytes, bool dry_run) {
    base = dry_run ? (unsigned char*)0x100000 : (unsigned char*)ws;
    cap = bytes; top = 0; peak = 0; dry = dry_run; err = 0;
  }
  // every block starts on a 256-byte boundary (rounded: what a block of `bytes` takes); the first overflow is error -100 and
  // hands out `base`
  static size_t rounded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  void* get(size_t bytes) {
    const size_t off = top;
    top = rounded(top + bytes);
    if (top > peak) peak = top;
    if (!dry && top > cap) { if (!err) err = -100; return base; }
    return base + off;
  }
  // scratch is released by going back to an earlier `top` (one stream: later launches are ordered behind its readers)
  void release(size_t mark) { top = mark; }
};

// a launch of an executor whose arena is the member `ar_`: skipped in the dry run and after the first error, which it records
#define RUN(expr)                          \
  do {                                     \
    if (!ar_.dry && !ar_.err) {            \
      int rc__ = (expr);                   \
      if (rc__) ar_.err = rc__;            \
    }                                      \
  } while (0)

}  // namespace flair
