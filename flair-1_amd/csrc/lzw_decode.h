// The rules of a TIFF 6.0 LZW stream (Compression = 5) as libtiff writes and reads it, and the one decode loop over them:
// lzw_decode_stream<Sink>, the decode-side twin of lzw_encode_stream<Src> (tiff_lzw.hip).  Codes MSB first, ClearCode 256, EOI 257,
// first free code 258, 9-bit codes widening to 10 / 11 / 12 when the decoder's next free code reaches 511 / 1023 / 2047.
//
// One wave per stream.  Every string a code can name already lies contiguously in the decoded output: entry k, added after the code
// that follows `old`, is string(old) plus the first byte of what came next, i.e. the bytes at [old_pos, old_pos + old_len + 1) of the
// output.  So a table entry is (position, length), 3838 of them (literals need none), and a code is emitted as a copy from earlier
// output, 64 bytes per step across the lanes: the serial chain is per code, not per byte.
// Bit parsing is wave-uniform: the input is held 256 bytes per register of the wave (4 bytes per lane, big-endian words), one chunk
// ahead, and a code is cut out of two words read with v_readlane.  Lane 0 alone writes the table.
//
// Where the decoded bytes live, how an entry is packed and what happens after a code are the Sink's (LzwStageSink in tiff_lzw.hip,
// LzwRingSink in tiff_read.hip):
//   void literal(int op, int c)                      byte c to position op (lane 0 stores)
//   void copy(int op, int from, int n, int wrap)     n >= 1 bytes to [op, op + n): byte j from position from + (j < wrap ? j : 0) < op
//   void entry(int k, int& pos, int& len) const      entry k of the table, wave-uniform
//   void set_entry(int k, int pos, int len)          called by lane 0 alone
//   void after_code(int op)                          [0, op) is produced and visible to every lane
#pragma once
#include <hip/hip_runtime.h>

namespace flair {

constexpr int LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258;
constexpr int LZW_CHUNK = 256;                       // input bytes per fetch: 64 lanes x 4
constexpr int LZW_DEC_ENTRIES = 4096 - LZW_FIRST;    // the decoder's table; its longest string has LZW_DEC_ENTRIES + 1 bytes

// what lzw_decode_stream returns; 5, a range or cap error of the arguments, is the kernels' own
enum { LZW_ST_OK = 0, LZW_ST_SRC_END = 1, LZW_ST_EOI = 2, LZW_ST_TABLE_CODE_FIRST = 3, LZW_ST_UNKNOWN_CODE = 4 };

// 4 bytes of the stream at `off` (any alignment, 64-bit offsets) as one big-endian word; offsets past the stream's end are clamped to
// its last byte (n >= 1) rather than branched around
__device__ __forceinline__ unsigned lzw_fetch_be(const unsigned char* __restrict__ src, long off, long n) {
  unsigned w = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) w = (w << 8) | src[min(off + e, n - 1)];
  return w;
}

// LDS stores of some lanes are read by other lanes afterwards: complete them, and keep the compiler from moving accesses across
__device__ __forceinline__ void lzw_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The stream s[0, sn), sn >= 1, decoded until dn >= 1 bytes exist, by the whole wave.  Returns the status: 0 when dn bytes were
// produced (a last string is clipped to them; neither EOI nor the rest of the stream is looked at), 1 when the stream ran out first,
// 2 at an EOI before that, 3 at a table code first after a Clear (or first of all: a stream need not begin with one), 4 at a code the
// table does not hold.  `produced` receives the number of bytes that exist, whatever the status.
template <class Sink>
__device__ __forceinline__ int lzw_decode_stream(const unsigned char* s, int sn, int dn, int lane, Sink& sink, int& produced) {
  const long nbits = (long)sn * 8;
  unsigned cur = lzw_fetch_be(s, 4 * lane, sn), ahead = lzw_fetch_be(s, LZW_CHUNK + 4 * lane, sn);
  long base = 0;                       // the stream offset of `cur`, bytes
  int b = 0;                           // the next code's bit offset inside `cur`, < 2048
  int nxt = LZW_FIRST, width = 9, op = 0, st;
  int old_pos = 0, old_len = 0;        // where the previous code's string was emitted; length 0: no previous code
  // every round consumes `width` >= 9 bits of the stream or ends: at most sn * 8 / 9 rounds whatever the bytes are
  for (;;) {
    if (op >= dn) { st = LZW_ST_OK; break; }
    if (base * 8 + b + width > nbits) { st = LZW_ST_SRC_END; break; }
    const int wi = b >> 5;
    const unsigned w0 = __builtin_amdgcn_readlane(cur, wi);
    const unsigned w1 = wi < 63 ? __builtin_amdgcn_readlane(cur, (wi + 1) & 63) : __builtin_amdgcn_readlane(ahead, 0);
    const int code = (int)(((((unsigned long long)w0 << 32) | w1) >> (64 - (b & 31) - width)) & ((1u << width) - 1));
    b += width;
    if (b >= 8 * LZW_CHUNK) {
      b -= 8 * LZW_CHUNK;
      base += LZW_CHUNK;
      cur = ahead;
      ahead = lzw_fetch_be(s, base + LZW_CHUNK + 4 * lane, sn);
    }
    if (code == LZW_CLEAR) { nxt = LZW_FIRST; width = 9; old_len = 0; continue; }
    if (code == LZW_EOI) { st = LZW_ST_EOI; break; }
    if (old_len == 0) {   // a path of its own and one exit below: folded into the common path, or with returns, both kernels lose 3 - 9 %
      if (code >= 256) { st = LZW_ST_TABLE_CODE_FIRST; break; }
      sink.literal(op, code);
      lzw_lds_order();
      old_pos = op; old_len = 1; ++op;
      sink.after_code(op);
      continue;
    }
    // the string of `code`: [from, from + len) of the output, except that at index `wrap` it starts over (code == nxt: string(old)
    // and its own first byte again, which is where this copy's first byte lands; the source stays below `op` all the same)
    int from = 0, len = 1, wrap = 0x7fffffff;
    if (code >= 256) {
      if (code < nxt) {
        sink.entry(code - LZW_FIRST, from, len);
      } else if (code == nxt && nxt < 4096) {
        from = old_pos; len = old_len + 1; wrap = old_len;
      } else { st = LZW_ST_UNKNOWN_CODE; break; }
    }
    const int n = min(len, dn - op);
    if (code < 256) sink.literal(op, code);
    else sink.copy(op, from, n, wrap);
    if (nxt < 4096) {
      if (lane == 0) sink.set_entry(nxt - LZW_FIRST, old_pos, old_len + 1);
      ++nxt;
      if (nxt == 511 || nxt == 1023 || nxt == 2047) ++width;
    }
    lzw_lds_order();
    old_pos = op; old_len = n; op += n;
    sink.after_code(op);
  }
  produced = op;
  return st;
}

}  // namespace flair
