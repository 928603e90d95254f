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
// The walk is one device function, lzw_encode_stream, over a source that says how the 4 bytes at a stream offset reach a lane: the
// strips above are its contiguous instance, the T x T TIFF tiles of a (bands, H, W) raster resident on the device (zone_detect's output
// file, flair_amd/raster_writer.py) the other, u8 or fp32 samples, band or pixel interleave; tiff_pack_streams_kernel then moves the
// streams out of their worst-case slots back to back, so that only compressed bytes cross PCIe.
// The decoder of the same streams (and of PIL's and libtiff's), the read path of metrics(), follows the encoder below; its loop is
// lzw_decode.h's, shared with the chunk decoder of tiff_read.hip.
#include "lzw_decode.h"
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

constexpr int LZW_TABLE = 8192;            // entries; a power of two
constexpr unsigned LZW_EMPTY = 0xffffffffu;   // key 0xfffff = (prefix 4095, byte 255): never a key, prefixes stay below 4094
constexpr int LZW_LIMIT = 4094;            // the encoder's reset; the stream constants are lzw_decode.h's

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

// One stream of n >= 1 bytes, by the whole wave: the dictionary walk, once, for every source a stream is read from.  `src` says how
// the 4 bytes at stream offset `off` (a multiple of 4) reach a lane: load(off, raw) issues the loads into `raw` (src's own Raw type,
// nothing waits for them), pack(raw) puts them together as one little-endian word when their turn comes.  Offsets at and past n are
// asked for (the prefetch runs one chunk ahead of the walk); their bytes are never walked, load only has to stay inside the source.
// Returns the stream's length in bytes; lane 0 alone has written it to `dst`.
template <class Src>
__device__ __forceinline__ int lzw_encode_stream(unsigned* tab, int lane, int n, unsigned* dst, const Src& src) {
  LzwOut o;
  o.dst = dst;
  o.acc = 0; o.nb = 0; o.nwords = 0; o.writer = lane == 0;

  lzw_clear_table(tab, lane);
  int nxt = LZW_FIRST, width = 9;
  o.put(LZW_CLEAR, width);

  // The walk, 256 bytes (one register of every lane) at a time; the next 256 are loaded meanwhile and only put together when their
  // turn comes, so nothing waits for them before.  The common step, a match at the first probe, has a loop of its own that carries
  // the prefix alone: one table read, one compare, one branch per byte.
  typename Src::Raw raw;
  src.load(4 * lane, raw);
  unsigned prefix = 0;
  for (int base = 0; base < n; base += LZW_CHUNK) {
    const unsigned chunk = src.pack(raw);
    src.load(base + LZW_CHUNK + 4 * lane, raw);
    const int m = min(LZW_CHUNK, n - base);
    int i = 0;
    if (base == 0) { prefix = __builtin_amdgcn_readlane(chunk, 0) & 0xff; i = 1; }   // the stream's first byte only opens a match
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
  return o.finish();
}

__device__ __forceinline__ unsigned lzw_pack4(const unsigned char (&raw)[4]) {
  return raw[0] | (raw[1] << 8) | (raw[2] << 16) | ((unsigned)raw[3] << 24);
}

// a strip: n contiguous bytes
struct LzwStripSrc {
  typedef unsigned char Raw[4];
  const unsigned char* __restrict__ src;
  int n;
  __device__ __forceinline__ void load(int off, Raw& raw) const { lzw_fetch4(src, off, n, raw); }
  __device__ __forceinline__ unsigned pack(const Raw& raw) const { return lzw_pack4(raw); }
};

__global__ __launch_bounds__(64) void tiff_lzw_encode_kernel(const unsigned char* __restrict__ img, int H, int W, int R, int nstrips,
                                                             unsigned char* __restrict__ out, long slot_bytes, int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned tab[LZW_TABLE];
  const int lane = threadIdx.x;
  const long strip = blockIdx.x;
  const int b = (int)(strip / nstrips), s = (int)(strip - (long)b * nstrips);
  const int rows = min(R, H - s * R);
  const int n = rows * W;
  const LzwStripSrc src{img + ((long)b * H + (long)s * R) * W, n};
  const int count = lzw_encode_stream(tab, lane, n, reinterpret_cast<unsigned*>(out + strip * slot_bytes), src);
  if (lane == 0) counts[strip] = count;
}

// A TIFF tile of a (bands, H, W) raster in band planes, T x T pixels with its top left pixel at (y0, x0); pixels outside the raster
// are 0 (TIFF tiles are always full size).  PIXEL = false: one band's tile, T * T bytes row-major (PlanarConfiguration 2); a lane's 4
// bytes lie in one tile row because T is a multiple of 4.  PIXEL = true: all bands of every pixel (PlanarConfiguration 1), byte k is
// row k / (T * bands), column (k / bands) % T, band k % bands: a lane's 4 bytes span bands, pixels and tile rows.  W, and with it the
// address of a row, may be odd: every sample is loaded by itself.  A sample's index in the raster is 64-bit.
// Sample = unsigned char: the byte as stored.  Sample = float: byte = (uint8) trunc(min(max(v * scale[band], 0), 255)), NaN -> 0, one
// fp32 multiply (there is no add to contract it with), done in pack(): the loads themselves wait for nothing.
template <class Sample, bool PIXEL>
struct LzwTileSrc {
  struct Raw { Sample v[4]; float k[4]; };   // the samples and, for floats, their bands' scales (unused for bytes: no register is kept)
  const Sample* __restrict__ src;       // band 0 for PIXEL, the stream's own band plane otherwise
  const float* __restrict__ scale;      // per band for PIXEL, the stream's own band's otherwise; null for bytes
  int H, W, T, bands, y0, x0, n;

  static constexpr bool SCALED = sizeof(Sample) == 4;
  __device__ __forceinline__ Sample at(int band, int r, int c) const {
    const int y = y0 + r, x = x0 + c;
    const bool in = y < H && x < W;
    const long idx = in ? ((long)band * H + y) * W + x : 0;     // out of the raster: a load that is in bounds, a value that is dropped
    const Sample v = src[idx];
    return in ? v : Sample(0);
  }
  __device__ __forceinline__ void load(int off, Raw& raw) const {
    if (off >= n) {                     // the prefetch past the stream's end: n is a multiple of 256, the whole chunk is past it
#pragma unroll
      for (int e = 0; e < 4; ++e) { raw.v[e] = Sample(0); raw.k[e] = 0.f; }
      return;
    }
    if (!PIXEL) {
      const int r = off / T, c = off - r * T;
      const float k = SCALED ? scale[0] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { raw.v[e] = at(0, r, c + e); raw.k[e] = k; }
    } else {
      const int pix = off / bands;
      int band = off - pix * bands, r = pix / T, c = pix - r * T;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        raw.v[e] = at(band, r, c);
        raw.k[e] = SCALED ? scale[band] : 0.f;
        if (++band == bands) { band = 0; if (++c == T) { c = 0; ++r; } }
      }
    }
  }
  static __device__ __forceinline__ unsigned char byte_of(unsigned char v, float) { return v; }
  static __device__ __forceinline__ unsigned char byte_of(float v, float k) {
    float p = v * k;
    p = p > 0.f ? p : 0.f;              // NaN and -0 become 0
    p = p < 255.f ? p : 255.f;
    return (unsigned char)(unsigned)p;  // truncation
  }
  __device__ __forceinline__ unsigned pack(const Raw& raw) const {
    unsigned char b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = byte_of(raw.v[e], raw.k[e]);
    return lzw_pack4(b);
  }
};

template <class Sample, bool PIXEL>
__global__ __launch_bounds__(64) void tiff_lzw_encode_tiles_kernel(const Sample* __restrict__ raster, const float* __restrict__ scale, int bands,
                                                                   int H, int W, int T, int tiles_y, int tiles_x, long first_stream,
                                                                   unsigned char* __restrict__ out, long slot_bytes, int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned tab[LZW_TABLE];
  const int lane = threadIdx.x;
  const long stream = first_stream + blockIdx.x;                   // (band * tiles_y + y) * tiles_x + x, without the band for PIXEL
  const long row = stream / tiles_x;
  const int tx = (int)(stream - row * tiles_x);
  const int b = PIXEL ? 0 : (int)(row / tiles_y);
  const int ty = (int)(row - (long)b * tiles_y);
  LzwTileSrc<Sample, PIXEL> src;
  src.src = raster + (long)b * H * W;
  src.scale = scale ? scale + b : nullptr;
  src.H = H; src.W = W; src.T = T; src.bands = bands;
  src.y0 = ty * T; src.x0 = tx * T;
  src.n = T * T * (PIXEL ? bands : 1);
  const int count = lzw_encode_stream(tab, lane, src.n, reinterpret_cast<unsigned*>(out + (long)blockIdx.x * slot_bytes), src);
  if (lane == 0) counts[blockIdx.x] = count;
}

// Stream i, counts[i] bytes at slots + i * slot_bytes, to dst + dst_off[i], 16 bytes per lane and step; the last 16 bytes are filled
// up with zeros (a slot's bytes past its count are unspecified).  A stream whose count or offset breaks the contract (count outside
// [0, slot_bytes], an offset below 0, no multiple of 16, or with its rounded count past dst_bytes) is not copied at all.
__global__ __launch_bounds__(256) void tiff_pack_streams_kernel(const unsigned char* __restrict__ slots, long slot_bytes,
                                                                const int* __restrict__ counts, const long long* __restrict__ dst_off,
                                                                unsigned char* __restrict__ dst, long dst_bytes) {
  const long i = blockIdx.x;
  const long count = counts[i], off = dst_off[i];
  const long nvec = (count + 15) >> 4;
  if (count < 0 || count > slot_bytes || off < 0 || (off & 15) || off > dst_bytes - 16 * nvec) return;
  const uint4* __restrict__ s = reinterpret_cast<const uint4*>(slots + i * slot_bytes);
  uint4* __restrict__ d = reinterpret_cast<uint4*>(dst + off);
  for (long v = threadIdx.x; v < nvec; v += 256) {
    uint4 w = s[v];
    const int keep = (int)min(16L, count - 16 * v);      // 1 .. 16 bytes of this vector belong to the stream
    if (keep < 16) {
      unsigned* u = reinterpret_cast<unsigned*>(&w);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int kb = keep - 4 * k;                     // bytes of word k that stay
        u[k] = kb >= 4 ? u[k] : kb <= 0 ? 0u : (u[k] & (0xffffffffu >> (8 * (4 - kb))));
      }
    }
    d[v] = w;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
// The read path of metrics(): one wave per strip again, the loop is lzw_decode_stream (lzw_decode.h).  The strip is decoded into an
// LDS stage and flushed to `dst` once, so the kernel never reads its own global stores back; the stage starts at the 16-byte phase of
// the strip's global address, which makes the flush aligned 16-byte words on both sides.  A table entry is (position, length)
// packed in one u32 (16 + 16 bits: positions stay below the 65 536-byte cap, lengths below 3840).
constexpr int LZW_DEC_SMALL = 16384, LZW_DEC_CAP = 65536;   // decoded bytes of an LZW strip per size class
constexpr int lzw_dec_lds(int cap) { return cap + 16 + LZW_DEC_ENTRIES * 4; }   // stage (+ 16: the alignment phase), table

struct LzwStageSink {
  unsigned char* stage;      // LDS; stage[i] is byte i of the strip
  unsigned* tab;             // LDS; entry k
  int lane;
  __device__ __forceinline__ void literal(int op, int c) { if (lane == 0) stage[op] = (unsigned char)c; }
  __device__ __forceinline__ void copy(int op, int from, int n, int wrap) {
    for (int j = lane; j < n; j += 64) stage[op + j] = stage[from + (j < wrap ? j : 0)];
  }
  __device__ __forceinline__ void entry(int k, int& pos, int& len) const {
    const unsigned e = __builtin_amdgcn_readfirstlane(tab[k]);
    pos = (int)(e >> 16); len = (int)(e & 0xffff);
  }
  __device__ __forceinline__ void set_entry(int k, int pos, int len) { tab[k] = ((unsigned)pos << 16) | (unsigned)len; }
  __device__ __forceinline__ void after_code(int) {}
};

// Strips of one size class: LZW strips with lo < dst_len <= hi.  The launch with `first` set also serves the stored strips and
// gives the out-of-range ones their status, so that every strip is served by exactly one launch.
__global__ __launch_bounds__(64) void tiff_lzw_decode_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                             const long long* __restrict__ strip_src_off, const int* __restrict__ strip_src_len,
                                                             const long long* __restrict__ strip_dst_off, const int* __restrict__ strip_dst_len,
                                                             const int* __restrict__ strip_mode, unsigned char* __restrict__ dst, long dst_bytes,
                                                             int* __restrict__ status, int lo, int hi, int first) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lzw_dec_smem[];
  const int lane = threadIdx.x;
  const long strip = blockIdx.x;
  const long so = strip_src_off[strip], dO = strip_dst_off[strip];
  const int sn = strip_src_len[strip], dn = strip_dst_len[strip], md = strip_mode[strip];
  const bool ok = so >= 0 && sn >= 0 && dO >= 0 && dn >= 1 && so <= src_bytes - sn && dO <= dst_bytes - dn &&
                  (md == 0 || (md == 1 && dn <= LZW_DEC_CAP));
  const unsigned char* __restrict__ s = src + so;
  unsigned char* __restrict__ g = dst + dO;
  if (!ok || md == 0) {
    if (!first) return;
    if (!ok) { if (lane == 0) status[strip] = 5; return; }
    const int n = min(sn, dn);
    for (int i = lane; i < n; i += 64) g[i] = s[i];
    if (lane == 0) status[strip] = sn >= dn ? 0 : 1;
    return;
  }
  if (dn <= lo || dn > hi) return;
  if (sn == 0) { if (lane == 0) status[strip] = 1; return; }

  const int phase = (int)((uintptr_t)g & 15);
  unsigned char* stage = lzw_dec_smem + phase;                                  // stage[i] is g[i]
  LzwStageSink sink{stage, reinterpret_cast<unsigned*>(lzw_dec_smem + hi + 16), lane};

  int op;
  const int st = lzw_decode_stream(s, sn, dn, lane, sink, op);

  // the flush: what was produced (all of the strip at status 0), bytes up to the first 16-byte boundary of g, words, bytes
  const int head = min(op, (16 - phase) & 15);
  if (lane < head) g[lane] = stage[lane];
  const int nvec = (op - head) >> 4;
  for (int i = lane; i < nvec; i += 64)
    *reinterpret_cast<uint4*>(g + head + 16 * i) = *reinterpret_cast<const uint4*>(stage + head + 16 * i);
  const int t = head + 16 * nvec + lane;
  if (t < op) g[t] = stage[t];
  if (lane == 0) status[strip] = st;
}

}  // namespace

int tiff_lzw_decode_max_strip() { return LZW_DEC_CAP; }

// Both size classes are launched over all strips (the tables are on the device: the host cannot sort them without a sync); a
// workgroup whose strip belongs to the other launch leaves at once.
int tiff_lzw_decode(const unsigned char* src, long src_bytes, const long long* strip_src_off, const int* strip_src_len,
                    const long long* strip_dst_off, const int* strip_dst_len, const int* strip_mode, long nstrips, unsigned char* dst,
                    long dst_bytes, int* status, hipStream_t s) {
  if (!src || !strip_src_off || !strip_src_len || !strip_dst_off || !strip_dst_len || !strip_mode || !dst || !status) return -1;
  if (nstrips < 1 || nstrips > 0x7fffffffL || src_bytes < 0 || dst_bytes < 0) return -1;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tiff_lzw_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       lzw_dec_lds(LZW_DEC_CAP));
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  {
    ProfScope ps("tiff_lzw_decode_small", 0.0, 0.0, s);
    hipLaunchKernelGGL(tiff_lzw_decode_kernel, dim3((unsigned)nstrips), dim3(64), lzw_dec_lds(LZW_DEC_SMALL), s, src, src_bytes, strip_src_off,
                       strip_src_len, strip_dst_off, strip_dst_len, strip_mode, dst, dst_bytes, status, 0, LZW_DEC_SMALL, 1);
    FLAIR_CHECK_LAUNCH();
  }
  {
    ProfScope ps("tiff_lzw_decode_large", 0.0, 0.0, s);
    hipLaunchKernelGGL(tiff_lzw_decode_kernel, dim3((unsigned)nstrips), dim3(64), lzw_dec_lds(LZW_DEC_CAP), s, src, src_bytes, strip_src_off,
                       strip_src_len, strip_dst_off, strip_dst_len, strip_mode, dst, dst_bytes, status, LZW_DEC_SMALL, LZW_DEC_CAP, 0);
    FLAIR_CHECK_LAUNCH();
  }
  return 0;
}

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

long tiff_lzw_tile_slot_bytes(int T, int samples) {
  if (T < 1 || samples < 1 || (long)T * T * samples > (1L << 30)) return -1;
  return tiff_lzw_slot_bytes(1, T * T * samples);
}

template <class Sample>
static int launch_encode_tiles(const Sample* raster, const float* scale, int bands, int H, int W, int T, int interleave, long first_stream,
                               long n_streams, unsigned char* out, long slot_bytes, int* counts, hipStream_t s) {
  const int ty = (H + T - 1) / T, tx = (W + T - 1) / T;
  const dim3 grid((unsigned)n_streams), block(64);
  if (interleave)
    hipLaunchKernelGGL((tiff_lzw_encode_tiles_kernel<Sample, true>), grid, block, 0, s, raster, scale, bands, H, W, T, ty, tx, first_stream, out,
                       slot_bytes, counts);
  else
    hipLaunchKernelGGL((tiff_lzw_encode_tiles_kernel<Sample, false>), grid, block, 0, s, raster, scale, bands, H, W, T, ty, tx, first_stream, out,
                       slot_bytes, counts);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int tiff_lzw_encode_tiles(const void* raster, int src_f32, const float* scale, int bands, int H, int W, int T, int interleave,
                          long first_stream, long n_streams, unsigned char* out, long slot_bytes, int* counts, hipStream_t s) {
  if (!raster || !out || !counts || bands < 1 || H < 1 || W < 1 || T < 1 || (T % 16)) return -1;
  if ((src_f32 != 0 && src_f32 != 1) || (interleave != 0 && interleave != 1) || (src_f32 && !scale)) return -1;
  const int samples = interleave ? bands : 1;
  const long slot = tiff_lzw_tile_slot_bytes(T, samples);            // -1: the kernel counts a stream's bytes in an int
  if (slot < 0 || (long)H + T > 0x7fffffffL || (long)W + T > 0x7fffffffL) return -1;
  const long ty = ((long)H + T - 1) / T, tx = ((long)W + T - 1) / T;
  const long total = (interleave ? 1 : (long)bands) * ty * tx;
  if (first_stream < 0 || n_streams < 1 || n_streams > 0x7fffffffL || first_stream > total - n_streams) return -1;
  if (slot_bytes < slot) return -100;
  if (((uintptr_t)out & 15) || (slot_bytes & 15) || ((uintptr_t)counts & 3) || ((uintptr_t)raster & (src_f32 ? 3 : 0)) ||
      ((uintptr_t)scale & 3))
    return -2;
  ProfScope ps(src_f32 ? "tiff_lzw_encode_tiles_f32" : "tiff_lzw_encode_tiles_u8", 0.0, (double)n_streams * T * T * samples * (src_f32 ? 4 : 1), s);
  if (src_f32)
    return launch_encode_tiles(static_cast<const float*>(raster), scale, bands, H, W, T, interleave, first_stream, n_streams, out, slot_bytes,
                               counts, s);
  return launch_encode_tiles(static_cast<const unsigned char*>(raster), scale, bands, H, W, T, interleave, first_stream, n_streams, out,
                             slot_bytes, counts, s);
}

int tiff_pack_streams(const unsigned char* slots, long slot_bytes, const int* counts, const long long* dst_off, long n_streams,
                      unsigned char* dst, long dst_bytes, hipStream_t s) {
  if (!slots || !counts || !dst_off || !dst || n_streams < 1 || n_streams > 0x7fffffffL || slot_bytes < 16 || dst_bytes < 0) return -1;
  if (((uintptr_t)slots & 15) || (slot_bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)counts & 3) || ((uintptr_t)dst_off & 7)) return -2;
  ProfScope ps("tiff_pack_streams", 0.0, 0.0, s);
  hipLaunchKernelGGL(tiff_pack_streams_kernel, dim3((unsigned)n_streams), dim3(256), 0, s, slots, slot_bytes, counts, dst_off, dst, dst_bytes);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
