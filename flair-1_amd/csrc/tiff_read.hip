// The read path of zone_detect's input raster (flair_amd/raster_reader.py): the chunks of a TIFF (tiles or strips, stored or LZW) are
// decoded into slots of a scratch buffer, one wave per chunk, and a second kernel scatters the slots into the (bands, H, W) band-plane
// raster, undoing the horizontal predictor on the way.  The stream rules, the loop and the status codes are lzw_decode_stream's
// (csrc/lzw_decode.h), shared with tiff_lzw_decode_kernel (csrc/tiff_lzw.hip); what differs is the size: a 512 x 512 tile of 5
// interleaved bands is 1.3 MB, so the decoded output lives in the slot, in global memory, and not in LDS.  Positions are 32 bits
// (RD_CAP = 16 MiB), lengths stay below RD_MAXSTR: an entry is one byte longer than the string before it, so the longest of the 3838
// entries between two clears has 3839 bytes.
//
// Where the copy reads from.  The most recent output lies in an LDS ring of RD_RING bytes, position p at ring[p % RD_RING].  After
// every code the completed 128-byte blocks of the output (the slot is 128-byte aligned, so these are whole cache lines) are flushed
// from the ring to the slot, 16 bytes per lane: flushed = op & ~127 at the start of every round, op the bytes produced so far.  A
// code's source byte at position s is read from the ring if s >= op - RD_WINDOW and from the slot otherwise (only a Clear bounds how
// far back a source lies: a run of equal bytes fills the table very slowly).  RD_WINDOW = RD_RING - RD_MAXSTR, because the copy
// itself, at most RD_MAXSTR - 1 bytes at [op, op + n), overwrites the ring places of [op - RD_RING, op + n - RD_RING): all of them
// older than the window, whatever step of the copy reads.  A source always lies below op and a destination at or above it, so no
// step of a copy reads what another step of it wrote.
//
// The read-back is a cross-lane read of the wave's own global stores: lane a's flush store is lane b's load.  Its argument:
//  (1) only positions below op - RD_WINDOW <= flushed are read from the slot, and flushed is a multiple of 128 on a 128-byte aligned
//      slot: a cache line is read only after its last byte was stored, never while unflushed bytes of it are still to come, and it is
//      never stored to again.  So no copy of a line that any cache can hold is ever older than the line's final content, provided
//      the stores have left the wave and the L1's copy, if it has one, is dropped:
//  (2) before a read-back whose source ends above `fenced` (the positions the last fence covered) the wave waits for its stores
//      (vmcnt(0)), releases at agent scope (the flush stores reach L2), waits again, acquires at agent scope (this CU's L1 drops its
//      lines) and sets fenced = flushed.  Sources are at least RD_WINDOW behind op and the fence covers all but the last < 128
//      bytes, so the next fence is due after another RD_WINDOW - 128 bytes of output at the earliest: one fence pair per 12 KB of
//      output in the worst case, none at all in a chunk whose references stay inside the window.  fenced starts at 0, so the first
//      read-back of a chunk is always behind an acquire.
//  (3) the read-back loads are per-lane byte loads through a pointer that is neither const nor __restrict__: vector loads, never
//      the scalar cache.
#include "lzw_decode.h"
#include "ops.h"
#include "prof.h"

namespace flair {

namespace {

constexpr int RD_RING = 16384;                       // a power of two
constexpr int RD_MAXSTR = 4096;                      // above the longest string, LZW_DEC_ENTRIES + 1
constexpr int RD_WINDOW = RD_RING - RD_MAXSTR;
constexpr int RD_BLOCK = 128;                        // the flush unit: one cache line
constexpr int RD_CAP = 1 << 24;                      // decoded bytes of an LZW chunk
static_assert((RD_RING & (RD_RING - 1)) == 0 && LZW_DEC_ENTRIES + 1 < RD_MAXSTR && RD_WINDOW > RD_BLOCK, "ring geometry");

// (2) of the argument above; every lane of the wave executes it
__device__ __forceinline__ void rd_publish_flushed() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct LzwRingSink {
  static constexpr int M = RD_RING - 1;
  unsigned char* ring;       // LDS
  unsigned* tpos;            // LDS; entry k: its string is [tpos, tpos + tlen) of the output
  unsigned short* tlen;
  unsigned char* g;          // the slot, 128-byte aligned; read back below: no __restrict__
  int lane;
  int flushed, fenced;       // multiples of RD_BLOCK: [0, flushed) is in the slot, [0, fenced) may be read back
  __device__ __forceinline__ void literal(int op, int c) { if (lane == 0) ring[op & M] = (unsigned char)c; }
  __device__ __forceinline__ void copy(int op, int from, int n, int wrap) {
    const int lo = op - RD_WINDOW;              // sources below it come from the slot; lo <= flushed
    if (from < lo && min(from + min(n, wrap), lo) > fenced) {
      rd_publish_flushed();
      fenced = flushed;
    }
    for (int j = lane; j < n; j += 64) {
      const int sp = from + (j < wrap ? j : 0);
      ring[(op + j) & M] = sp >= lo ? ring[sp & M] : g[sp];
    }
  }
  __device__ __forceinline__ void entry(int k, int& pos, int& len) const {
    pos = (int)__builtin_amdgcn_readfirstlane(tpos[k]);
    len = (int)__builtin_amdgcn_readfirstlane((unsigned)tlen[k]);
  }
  __device__ __forceinline__ void set_entry(int k, int pos, int len) { tpos[k] = (unsigned)pos; tlen[k] = (unsigned short)len; }
  __device__ __forceinline__ void after_code(int op) {
    const int upto = op & ~(RD_BLOCK - 1);
    if (upto > flushed) {                        // whole blocks: at most RD_MAXSTR bytes, all of them still in the ring
      for (int i = flushed + 16 * lane; i < upto; i += 1024)
        *reinterpret_cast<uint4*>(g + i) = *reinterpret_cast<const uint4*>(ring + (i & M));
      flushed = upto;
    }
  }
};

__global__ __launch_bounds__(64) void tiff_lzw_decode_chunks_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                                    const long long* __restrict__ src_off, const int* __restrict__ src_len,
                                                                    const int* __restrict__ dst_len, const int* __restrict__ mode,
                                                                    unsigned char* scratch, long slot_bytes, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) unsigned char ring[RD_RING];
  __shared__ unsigned tpos[LZW_DEC_ENTRIES];
  __shared__ unsigned short tlen[LZW_DEC_ENTRIES];
  const int lane = threadIdx.x;
  const long chunk = blockIdx.x;
  const long so = src_off[chunk];
  const int sn = src_len[chunk], dn = dst_len[chunk], md = mode[chunk];
  const bool ok = so >= 0 && sn >= 0 && dn >= 1 && so <= src_bytes - sn && dn <= slot_bytes && (md == 0 || (md == 1 && dn <= RD_CAP));
  if (!ok) { if (lane == 0) status[chunk] = 5; return; }
  const unsigned char* __restrict__ s = src + so;
  unsigned char* g = scratch + chunk * slot_bytes;
  if (md == 0) {
    // stored: the slot is aligned, the source is not; 4 bytes per lane, put together as one word
    const int n = min(sn, dn), n4 = n & ~3;
    for (int i = 4 * lane; i < n4; i += 256)
      *reinterpret_cast<unsigned*>(g + i) = s[i] | (s[i + 1] << 8) | (s[i + 2] << 16) | ((unsigned)s[i + 3] << 24);
    if (n4 + lane < n) g[n4 + lane] = s[n4 + lane];
    if (lane == 0) status[chunk] = sn >= dn ? 0 : 1;
    return;
  }
  if (sn == 0) { if (lane == 0) status[chunk] = 1; return; }

  LzwRingSink sink{ring, tpos, tlen, g, lane, 0, 0};
  int op;
  const int st = lzw_decode_stream(s, sn, dn, lane, sink, op);
  // what was produced past the last whole block (all of the chunk's rest at status 0): fewer than RD_BLOCK bytes
  for (int i = sink.flushed + lane; i < op; i += 64) g[i] = ring[i & LzwRingSink::M];
  if (lane == 0) status[chunk] = st;
}

// The row walk of both scatter kernels.  A chunk's decoded bytes, rows x width pixels of `samples` bytes each, row-major, to planes
// of H x W bytes: sample k of the pixel at (r, x) goes to first[k][y0 + r][x0 + x] (`first` the plane of sample 0) when that lies
// inside H x W.  The block's four waves take the rows blockIdx.y * 4 + wave, + gridDim.y * 4, ...: one wave per chunk row, a lane per
// pixel, 64 pixels a trip, so the stores of a trip are 64 consecutive bytes of one plane row.  PRED: TIFF predictor 2, per sample
// the running sum modulo 256 along the chunk row, as an inclusive wave scan per trip plus the carry of the trips before (lane 63's
// sum).  The caller has checked the chunk: x0, y0 >= 0, width, rows, samples >= 1, the slot holds the chunk, the planes exist.
template <bool PRED>
__device__ __forceinline__ void chunk_rows_to_planes(const unsigned char* __restrict__ slot, int x0, int y0, int width, int rows, int samples,
                                                     unsigned char* __restrict__ first, int H, int W) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long plane = (long)H * W;
  for (int r = blockIdx.y * 4 + wave; r < rows; r += gridDim.y * 4) {
    const int y = y0 + r;
    if (y >= H) return;                                     // rows of an edge tile below the raster, and every row after
    const unsigned char* __restrict__ row = slot + (long)r * width * samples;
    unsigned char* __restrict__ out = first + (long)y * W + x0;
    for (int k = 0; k < samples; ++k) {
      unsigned carry = 0;
      for (int xb = 0; xb < width; xb += 64) {
        const int x = xb + lane;
        unsigned v = x < width ? row[(long)x * samples + k] : 0u;
        if (PRED) {
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(v, d, 64);
            if (lane >= d) v += t;
          }
          v = (v + carry) & 0xffu;
          carry = __shfl(v, 63, 64);
        }
        if (x < width && x0 + x < W) out[(long)k * plane + x] = (unsigned char)v;
        if (x0 + xb + 64 >= W) break;                      // the rest of the row lies right of the raster
      }
    }
  }
}

// One raster: every chunk has the launch's `samples` and predictor; chunks (n, 5) {x0, y0, width, rows, band0}.
template <bool PRED>
__global__ __launch_bounds__(256) void tiff_chunks_to_planes_kernel(const unsigned char* __restrict__ scratch, long slot_bytes,
                                                                    const int* __restrict__ chunks, const int* __restrict__ status,
                                                                    int samples, unsigned char* __restrict__ planes, int bands, int H, int W) {
  const long c = blockIdx.x;
  if (status[c] != 0) return;
  const int x0 = chunks[5 * c], y0 = chunks[5 * c + 1], width = chunks[5 * c + 2], rows = chunks[5 * c + 3], band0 = chunks[5 * c + 4];
  if (x0 < 0 || y0 < 0 || width < 1 || rows < 1 || band0 < 0 || band0 > bands - samples) return;
  if ((long)width * rows * samples > slot_bytes) return;
  chunk_rows_to_planes<PRED>(scratch + c * slot_bytes, x0, y0, width, rows, samples, planes + (long)band0 * H * W, H, W);
}

// A batch of files: chunks (n, 8) {x0, y0, width, rows, plane0, samples, predictor, 0}, every chunk with the samples and the
// predictor of its own file; planes (n_planes, H, W), the planes of all files one behind the other.  What decides a chunk's path is
// its table row, the same for the whole block: the branch on the predictor does not diverge.
__global__ __launch_bounds__(256) void tiff_chunks_to_batch_kernel(const unsigned char* __restrict__ scratch, long slot_bytes,
                                                                   const int* __restrict__ chunks, const int* __restrict__ status,
                                                                   unsigned char* __restrict__ planes, int n_planes, int H, int W) {
  const long c = blockIdx.x;
  if (status[c] != 0) return;
  const int* __restrict__ t = chunks + 8 * c;
  const int x0 = t[0], y0 = t[1], width = t[2], rows = t[3], plane0 = t[4], samples = t[5], predictor = t[6];
  if (x0 < 0 || y0 < 0 || width < 1 || rows < 1 || samples < 1 || plane0 < 0 || plane0 > n_planes - samples) return;
  if (predictor != 1 && predictor != 2) return;
  if ((long)width * rows > slot_bytes / samples) return;   // width * rows * samples > slot_bytes, without the product of three
  const unsigned char* __restrict__ slot = scratch + c * slot_bytes;
  unsigned char* __restrict__ first = planes + (long)plane0 * H * W;
  if (predictor == 2)
    chunk_rows_to_planes<true>(slot, x0, y0, width, rows, samples, first, H, W);
  else
    chunk_rows_to_planes<false>(slot, x0, y0, width, rows, samples, first, H, W);
}

}  // namespace

int tiff_lzw_decode_chunks_cap() { return RD_CAP; }
int tiff_lzw_decode_chunks_window() { return RD_WINDOW; }

int tiff_lzw_decode_chunks(const unsigned char* src, long src_bytes, const long long* src_off, const int* src_len, const int* dst_len,
                           const int* mode, long nchunks, unsigned char* scratch, long slot_bytes, int* status, hipStream_t s) {
  if (!src || !src_off || !src_len || !dst_len || !mode || !scratch || !status) return -1;
  if (nchunks < 1 || nchunks > 0x7fffffffL || src_bytes < 0 || slot_bytes < 1) return -1;
  if (((uintptr_t)scratch & (RD_BLOCK - 1)) || (slot_bytes & (RD_BLOCK - 1)) || ((uintptr_t)src_off & 7) || ((uintptr_t)src_len & 3) ||
      ((uintptr_t)dst_len & 3) || ((uintptr_t)mode & 3) || ((uintptr_t)status & 3))
    return -2;   // blocks of the slot are flushed as aligned cache lines
  ProfScope ps("tiff_lzw_decode_chunks", 0.0, 0.0, s);
  hipLaunchKernelGGL(tiff_lzw_decode_chunks_kernel, dim3((unsigned)nchunks), dim3(64), 0, s, src, src_bytes, src_off, src_len, dst_len, mode,
                     scratch, slot_bytes, status);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int tiff_chunks_to_planes(const unsigned char* scratch, long slot_bytes, const int* chunks, const int* status, long nchunks, int max_rows,
                          int samples, int predictor, unsigned char* planes, int bands, int H, int W, hipStream_t s) {
  if (!scratch || !chunks || !status || !planes) return -1;
  if (nchunks < 1 || nchunks > 0x7fffffffL || slot_bytes < 1 || max_rows < 1 || bands < 1 || H < 1 || W < 1) return -1;
  if ((samples != 1 && samples != bands) || (predictor != 1 && predictor != 2)) return -1;
  if (((uintptr_t)chunks & 3) || ((uintptr_t)status & 3)) return -2;
  const dim3 grid((unsigned)nchunks, (unsigned)min((max_rows + 3) / 4, 65535)), block(256);
  ProfScope ps("tiff_chunks_to_planes", 0.0, 0.0, s);
  if (predictor == 2)
    hipLaunchKernelGGL((tiff_chunks_to_planes_kernel<true>), grid, block, 0, s, scratch, slot_bytes, chunks, status, samples, planes, bands, H, W);
  else
    hipLaunchKernelGGL((tiff_chunks_to_planes_kernel<false>), grid, block, 0, s, scratch, slot_bytes, chunks, status, samples, planes, bands, H, W);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

int tiff_chunks_to_batch(const unsigned char* scratch, long slot_bytes, const int* chunks, const int* status, long nchunks, int max_rows,
                         unsigned char* planes, int n_planes, int H, int W, hipStream_t s) {
  if (!scratch || !chunks || !status || !planes) return -1;
  if (nchunks < 1 || nchunks > 0x7fffffffL || slot_bytes < 1 || max_rows < 1 || n_planes < 1 || H < 1 || W < 1) return -1;
  if (((uintptr_t)chunks & 3) || ((uintptr_t)status & 3)) return -2;
  const dim3 grid((unsigned)nchunks, (unsigned)min((max_rows + 3) / 4, 65535)), block(256);
  ProfScope ps("tiff_chunks_to_batch", 0.0, 0.0, s);
  hipLaunchKernelGGL(tiff_chunks_to_batch_kernel, grid, block, 0, s, scratch, slot_bytes, chunks, status, planes, n_planes, H, W);
  FLAIR_CHECK_LAUNCH();
  return 0;
}

}  // namespace flair
