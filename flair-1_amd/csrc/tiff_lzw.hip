// TIFF 6.0 LZW (Compression = 5, no predictor) of uint8 prediction tiles, one independently compressed stream per strip
// (writer.py f2: the last stage of the predict flow that still ran on the host).  Strip s of tile b covers rows
// [s*R, min(H, (s+1)*R)) as one byte stream; its codes go to slot b*nstrips + s of `out`, its length to counts[].
// Stream format as libtiff writes and reads it: codes MSB first, ClearCode 256 first, EOI 257 last, first free code 258, greedy
// longest match, 9-bit codes widening to 10 / 11 / 12 when the next free code reaches 512 / 1024 / 2048 ("early change" as the
// encoder sees it), ClearCode and a fresh table when it reaches 4094.
//
// One wave per strip.  LZW is a dependent chain, one dictionary lookup of (prefix, byte) per input byte, so the lanes are not
// the resource, LDS is: the dictionary is an open-addressing table of 8192 packed u32 entries (20-bit key, 12-bit code), 32 KB,
// at load <= 3836 / 8192 = 0.47; five strips fit a CU.  All 64 lanes clear the table (at the start and at a reset) and fetch the
// input 256 bytes at a time, 4 bytes per lane, one chunk ahead of the walk; the walk itself is executed by every lane on the same
// values (a wave-uniform program: the current byte comes out of the chunk registers with v_readlane), lane 0 alone writes.
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

constexpr int LZW_TABLE = 8192;            // entries; a power of two
constexpr unsigned LZW_EMPTY = 0xffffffffu;   // key 0xfffff = (prefix 4095, byte 255): never a key, prefixes stay below 4094
constexpr int LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258, LZW_LIMIT = 4094;
constexpr int LZW_CHUNK = 256;             // input bytes per fetch: 64 lanes x 4

__device__ __forceinline__ void lzw_clear_table(unsigned* tab, int lane) {
  uint4* t4 = reinterpret_cast<uint4*>(tab);
  for (int i = lane; i < LZW_TABLE / 4; i += 64) t4[i] = make_uint4(LZW_EMPTY, LZW_EMPTY, LZW_EMPTY, LZW_EMPTY);
  __syncthreads();
}

// 4 bytes of the strip at offset `off` (any alignment).  Offsets past the strip's end are clamped to its last byte (n >= 1) rather
// than branched around: the four loads issue back to back.
__device__ __forceinline__ void lzw_fetch4(const unsigned char* __restrict__ src, int off, int n, unsigned char (&raw)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) raw[e] = src[min(off + e, n - 1)];
}

struct LzwOut {
  unsigned* dst;             // the strip's slot, as 32-bit words (slots are 16-byte aligned)
  unsigned long long acc;    // pending bits in the low `nb` bits (bits above them are stale)
  int nb, nwords;
  bool writer;
  __device__ __forceinline__ void put(unsigned code, int width) {
    acc = (acc << width) | code;
    nb += width;
    if (nb >= 32) {                      // nb <= 31 + 12
      const unsigned w = (unsigned)(acc >> (nb - 32));
      if (writer) dst[nwords] = __builtin_bswap32(w);
      ++nwords;
      nb -= 32;
    }
  }
  // the last, zero-padded word; returns the stream's length in bytes
  __device__ __forceinline__ int finish() {
    if (nb > 0 && writer) dst[nwords] = __builtin_bswap32((unsigned)(acc << (32 - nb)));
    return nwords * 4 + (nb + 7) / 8;
  }
};

__device__ __forceinline__ int lzw_widen(int nxt, int width) { return (nxt == 512 || nxt == 1024 || nxt == 2048) ? width + 1 : width; }

__global__ __launch_bounds__(64) void tiff_lzw_encode_kernel(const unsigned char* __restrict__ img, int H, int W, int R, int nstrips,
                                                             unsigned char* __restrict__ out, long slot_bytes, int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned tab[LZW_TABLE];
  const int lane = threadIdx.x;
  const long strip = blockIdx.x;
  const int b = (int)(strip / nstrips), s = (int)(strip - (long)b * nstrips);
  const int rows = min(R, H - s * R);
  const int n = rows * W;
  const unsigned char* src = img + ((long)b * H + (long)s * R) * W;

  LzwOut o;
  o.dst = reinterpret_cast<unsigned*>(out + strip * slot_bytes);
  o.acc = 0; o.nb = 0; o.nwords = 0; o.writer = lane == 0;

  lzw_clear_table(tab, lane);
  int nxt = LZW_FIRST, width = 9;
  o.put(LZW_CLEAR, width);

  // The walk, 256 bytes (one register of every lane) at a time; the next 256 are loaded meanwhile and only put together when their
  // turn comes, so nothing waits for them before.  The common step, a match at the first probe, has a loop of its own that carries
  // the prefix alone: one table read, one compare, one branch per byte.
  unsigned char raw[4];
  lzw_fetch4(src, 4 * lane, n, raw);
  unsigned prefix = 0;
  for (int base = 0; base < n; base += LZW_CHUNK) {
    const unsigned chunk = raw[0] | (raw[1] << 8) | (raw[2] << 16) | ((unsigned)raw[3] << 24);
    lzw_fetch4(src, base + LZW_CHUNK + 4 * lane, n, raw);
    const int m = min(LZW_CHUNK, n - base);
    int i = 0;
    if (base == 0) { prefix = __builtin_amdgcn_readlane(chunk, 0) & 0xff; i = 1; }   // the strip's first byte only opens a match
    while (i < m) {
      unsigned c, key, slot, e;
      bool hit;
      do {
        c = (__builtin_amdgcn_readlane(chunk, i >> 2) >> (8 * (i & 3))) & 0xff;
        key = (prefix << 8) | c;
        slot = (key * 0x9e3779b1u) >> 19;     // 13 bits
        e = tab[slot];
        hit = (e >> 12) == key;               // (LZW_EMPTY >> 12 is no key)
        if (!hit) break;
        prefix = e & 0xfff;
      } while (++i < m);
      if (hit) break;
      for (int p = 1; p < LZW_TABLE && e != LZW_EMPTY; ++p) {   // bounded by the table size whatever the bytes are
        slot = (slot + 1) & (LZW_TABLE - 1);
        e = tab[slot];
        if ((e >> 12) == key) { hit = true; break; }
      }
      ++i;
      if (hit) { prefix = e & 0xfff; continue; }
      o.put(prefix, width);
      if (e == LZW_EMPTY && lane == 0) tab[slot] = (key << 12) | (unsigned)nxt;   // a full table (unreachable: <= 3836 entries) adds nothing
      __builtin_amdgcn_wave_barrier();   // no code motion across lane 0's store: the other lanes read it in the next lookup
      ++nxt;
      width = lzw_widen(nxt, width);
      if (nxt >= LZW_LIMIT) {
        o.put(LZW_CLEAR, width);
        lzw_clear_table(tab, lane);
        nxt = LZW_FIRST; width = 9;
      }
      prefix = c;
    }
  }
  o.put(prefix, width);
  ++nxt;
  width = lzw_widen(nxt, width);
  o.put(LZW_EOI, width);
  const int count = o.finish();
  if (lane == 0) counts[strip] = count;
}

}  // namespace

// at most n + n / 3836 + 3 codes of at most 12 bits (ClearCode, one per byte, one per reset, EOI)
long tiff_lzw_slot_bytes(int R, int W) {
  if (R < 1 || W < 1) return -1;
  const long n = (long)R * W;
  const long codes = n + n / 3836 + 4;
  return round_up((3 * codes + 1) / 2, 16);
}

int tiff_lzw_encode(const unsigned char* img, int B, int H, int W, int R, unsigned char* out, long slot_bytes, int* counts, hipStream_t s) {
  if (!img || !out || !counts || B < 1 || H < 1 || W < 1 || R < 1) return -1;
  if ((long)R * W > (1L << 30)) return -1;                    // the kernel counts a strip's bytes in an int
  if (slot_bytes < tiff_lzw_slot_bytes(R, W)) return -100;
  if (((uintptr_t)out & 15) || (slot_bytes & 15) || ((uintptr_t)counts & 3)) return -2;   // slots are written as aligned 32-bit words
  const int nstrips = (int)(((long)H + R - 1) / R);
  const long nblk = (long)B * nstrips;
  if (nblk > 0x7fffffffL) return -1;
  ProfScope ps("tiff_lzw_encode", 0.0, (double)B * H * W, s);
  hipLaunchKernelGGL(tiff_lzw_encode_kernel, dim3((unsigned)nblk), dim3(64), 0, s, img, H, W, R, nstrips, out, slot_bytes, counts);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
