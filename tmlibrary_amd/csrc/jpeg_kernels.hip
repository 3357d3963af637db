// JPEG coding of pyramid tiles (tmlib/image.py:1073-1094 PyramidTile.jpeg_encode,
// reached once per tile from tmlib/models/tile.py:107-122): every tile of one
// tile-major level [rows][cols][256][256] uint8 as the baseline JPEG file
// libjpeg writes for it, byte for byte.  The per-block arithmetic is
// jpeg_core.h (shared with the host build the CPU suite checks); this file is
// the workgroup around it and the scan of the files' sizes into offsets.
//
// A file's size is only known once it is coded (0xFF bytes are stuffed), so a
// level is coded twice by the same kernel: once counting bytes, the sizes
// scanned into offsets, then once writing each file at its offset.  No
// scratch proportional to the level; every output byte has one writer.
#include "common.h"
#include "jpeg_core.h"

namespace tmh {

namespace {

constexpr int kTile = 256;
constexpr int64_t kTileBytes = (int64_t)kTile * kTile;
constexpr int kJT = 128;  // threads per workgroup = blocks per strip
// The bit buffer holds a quarter of a strip at the largest size of every
// block, behind 7 carried bits, and one word of slack for the sinks' last
// partial word.
constexpr int kBatchBits = (kJT / 4) * kJpegMaxBlockBits + 7;
constexpr int kBitWords = (kBatchBits + 31) / 32 + 1;

typedef unsigned int jpg_u32x4 __attribute__((ext_vector_type(4)));

struct OrLds {
  static __device__ __forceinline__ void apply(uint32_t* p, uint32_t v) { atomicOr(p, v); }
};

struct JpegShared {
  JpegTables t;
  uint32_t coef[kJT * kJpegCoefPitch];
  uint32_t bits[kBitWords];
  int part[4];
  int ff[2];
};

// One workgroup per tile; thread i of a strip owns block s0 + i of the tile's
// blocks in raster order (the order of the entropy-coded segment).  Per strip:
//   1. samples -> DCT -> quantised coefficients, zigzag order, in LDS;
//   2. the block's bit length (a dry run of the coder), scanned over the
//      workgroup into the block's bit offset in the strip;
//   3. the block's bits merged into the bit buffer in LDS, behind the 0..7
//      bits left over before it;
//   4. the buffer's whole bytes: each wave takes half of them, 64 per round,
//      counts the 0xFF among them (ballot) and, when WRITE, stores every byte
//      at its stuffed position -- consecutive lanes, consecutive addresses.
// (3 and 4 once per strip, or per quarter of it when the strip's bits exceed
// the buffer.)  The DC predictor and the partial byte carry on.  A tile of
// one value (spacer tiles, background) skips the samples and the DCT after
// its first strip: every block has the first block's coefficients.
// !WRITE: sizes[t] = the file's size.  WRITE: the file at out + offsets[t].
template <bool WRITE>
__global__ __launch_bounds__(kJT, 3) void k_jpeg_tiles(const uint8_t* __restrict__ level, int rows,
                                                    int cols, int last_h, int last_w,
                                                    const JpegTables* __restrict__ tables,
                                                    const int64_t* __restrict__ offsets,
                                                    int64_t* __restrict__ sizes,
                                                    uint8_t* __restrict__ out) {
  __shared__ JpegShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t t = blockIdx.x;
  const int ty = (int)(t / cols), tx = (int)(t - (int64_t)ty * cols);
  const int H = ty == rows - 1 ? last_h : kTile, W = tx == cols - 1 ? last_w : kTile;
  const int bw = (W + 7) >> 3, nblk = ((H + 7) >> 3) * bw;
  const uint8_t* tile = level + t * kTileBytes;
  uint8_t* file = WRITE ? out + offsets[t] : nullptr;

  for (int i = tid; i < (int)(sizeof(JpegTables) / 4); i += kJT)
    reinterpret_cast<uint32_t*>(&S.t)[i] = reinterpret_cast<const uint32_t*>(tables)[i];

  // is the tile one value?  16 bytes per load, columns past W masked out
  const uint32_t v0 = tile[0];
  uint32_t differs = 0;
  for (int i = tid; i < H * 16; i += kJT) {
    const int c = (i & 15) * 16;
    if (c >= W) continue;
    const jpg_u32x4 v = *reinterpret_cast<const jpg_u32x4*>(tile + (i >> 4) * kTile + c);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int keep = W - c - 4 * j;  // bytes of word j inside the tile
      const uint32_t m = keep >= 4 ? 0xFFFFFFFFu : keep <= 0 ? 0u : 0xFFFFFFFFu >> (8 * (4 - keep));
      differs |= (w[j] ^ (v0 * 0x01010101u)) & m;
    }
  }
  const bool uniform = !__syncthreads_or(differs != 0);  // (also: S.t is complete)

  if (WRITE)
    for (int i = tid; i < kJpegHeaderBytes; i += kJT)
      file[i] = jpeg_header_byte(S.t.header, i, H, W);

  int cursor = kJpegHeaderBytes;  // bytes of the file so far
  int carry_bits = 0;             // 0..7 bits of the last strip not yet a byte ...
  uint32_t carry_word = 0;        // ... at the top of this word
  int carry_dc = 0;               // DC of the block before this strip
  uint32_t* zz = S.coef + tid * kJpegCoefPitch;

  for (int s0 = 0; s0 < nblk; s0 += kJT) {
    const int b = s0 + tid;
    const bool active = b < nblk;
    // 1. coefficients
    if (active && (!uniform || s0 == 0)) {
      int d[64];
      if (uniform) {
#pragma unroll
        for (int i = 0; i < 64; ++i) d[i] = (int)v0 - 128;
      } else {
        const int by = b / bw;
        jpeg_load_block(tile, kTile, H, W, by, b - by * bw, d);
      }
      jpeg_fdct_quantise(d, S.t, zz);
    }
    __syncthreads();
    // 2. lengths and offsets
    const int prev_dc = tid ? jpeg_coef(zz - kJpegCoefPitch, 0) : carry_dc;
    int len = 0;
    if (active) {
      JpegCountSink c;
      jpeg_encode_block(zz, prev_dc, S.t, c);
      len = c.bits;
    }
    int incl = len;  // inclusive scan over the wave
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
      const int up = __shfl_up(incl, step);
      if (lane >= step) incl += up;
    }
    if ((lane & 31) == 31) S.part[tid >> 5] = incl;  // at the end of each quarter of the strip
    __syncthreads();
    const int q1 = S.part[0], q2 = S.part[1], q3 = q2 + S.part[2], strip_bits = q2 + S.part[3];
    const int at_strip = (wave ? q2 : 0) + incl - len;  // the block's bit offset in the strip
    carry_dc = jpeg_coef(S.coef + (kJT - 1) * kJpegCoefPitch, 0);
    // Steps 3 and 4 over the whole strip when its bits fit the buffer (they do
    // unless blocks average more than a quarter of the largest size), else over
    // its quarters one after another: 32 blocks always fit.
    const int nbatch = carry_bits + strip_bits <= kBatchBits ? 1 : 4;
    for (int q = 0; q < nbatch; ++q) {
      const int lo = nbatch == 1 || q == 0 ? 0 : q == 1 ? q1 : q == 2 ? q2 : q3;
      const int hi = nbatch == 1 || q == 3 ? strip_bits : q == 0 ? q1 : q == 1 ? q2 : q3;
      const int total_bits = carry_bits + hi - lo;
      // 3. the batch's bits
      const int nwords = (total_bits + 31) / 32 + 1;  // <= kBitWords
      for (int i = tid; i < nwords; i += kJT) S.bits[i] = i ? 0u : carry_word;
      __syncthreads();
      if (active && (nbatch == 1 || (tid >> 5) == q)) {
        JpegBitSink<OrLds> sink(S.bits, carry_bits + at_strip - lo);
        jpeg_encode_block(zz, prev_dc, S.t, sink);
        sink.finish();
      }
      __syncthreads();
      // 4. whole bytes; the tile's last partial byte is filled with 1 bits
      const bool last = s0 + kJT >= nblk && q == nbatch - 1;
      const int nbytes = last ? (total_bits + 7) >> 3 : total_bits >> 3;
      const uint32_t fill = last ? (1u << ((8 - (total_bits & 7)) & 7)) - 1u : 0u;
      const int seg = (((nbytes + 1) >> 1) + 63) & ~63;
      const int beg = min(wave * seg, nbytes), end = min(beg + seg, nbytes);
      int ff = 0;
      for (int r = beg; r < end; r += 64) {
        const int i = r + lane;
        const bool is_ff =
            i < end && (jpeg_stream_byte(S.bits, i) | (i == nbytes - 1 ? fill : 0u)) == 255u;
        ff += __popcll(__ballot(is_ff));
      }
      if (lane == 0) S.ff[wave] = ff;
      __syncthreads();
      if (WRITE) {
        int shift = wave ? S.ff[0] : 0;  // stuffed bytes before this round
        for (int r = beg; r < end; r += 64) {
          const int i = r + lane;
          const uint32_t v =
              i < end ? jpeg_stream_byte(S.bits, i) | (i == nbytes - 1 ? fill : 0u) : 0u;
          const unsigned long long m = __ballot(v == 255u);
          if (i < end) {
            uint8_t* p = file + cursor + i + shift + __popcll(m & ((1ull << lane) - 1ull));
            p[0] = (uint8_t)v;
            if (v == 255u) p[1] = 0;
          }
          shift += __popcll(m);
        }
      }
      cursor += nbytes + S.ff[0] + S.ff[1];
      carry_bits = last ? 0 : total_bits & 7;
      carry_word = (jpeg_stream_byte(S.bits, nbytes) & ~(0xFFu >> carry_bits)) << 24;
      __syncthreads();  // before bits, ff and (next strip) coef and part are rewritten
    }
  }
  if (tid == 0) {
    if (WRITE) {
      file[cursor] = 0xFF;
      file[cursor + 1] = 0xD9;
    } else {
      sizes[t] = cursor + 2;
    }
  }
}

// offsets[0] = 0 and, in place, offsets[1 + i] = the sum of the sizes held in
// offsets[1 .. 1 + i]: one workgroup, a contiguous run of entries per thread
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_jpeg_offsets(int64_t* __restrict__ offsets,
                                                               int64_t n) {
  __shared__ int64_t part[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t b = min((int64_t)tid * per, n), e = min(b + per, n);
  int64_t sum = 0;
  for (int64_t i = b; i < e; ++i) sum += offsets[1 + i];
  part[tid] = sum;
  __syncthreads();
  for (int step = 1; step < kScanThreads; step <<= 1) {
    const int64_t add = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int64_t run = part[tid] - sum;
  for (int64_t i = b; i < e; ++i) {
    run += offsets[1 + i];
    offsets[1 + i] = run;
  }
  if (tid == 0) offsets[0] = 0;
}

}  // namespace

void jpeg_tables_host(int quality, void* tables) {
  jpeg_build_tables(quality, static_cast<JpegTables*>(tables));
}
size_t jpeg_tables_bytes() { return sizeof(JpegTables); }

void launch_jpeg_measure(const uint8_t* level, int rows, int cols, int last_h, int last_w,
                         const void* d_tables, int64_t* offsets, hipStream_t s) {
  ProfScope prof("jpeg_measure", s);
  const int64_t n = (int64_t)rows * cols;
  hipLaunchKernelGGL(k_jpeg_tiles<false>, dim3((unsigned)n), dim3(kJT), 0, s, level, rows, cols,
                     last_h, last_w, static_cast<const JpegTables*>(d_tables),
                     (const int64_t*)nullptr, offsets + 1, (uint8_t*)nullptr);
  TMH_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_jpeg_offsets, dim3(1), dim3(kScanThreads), 0, s, offsets, n);
  TMH_HIP(hipGetLastError());
}

void launch_jpeg_write(const uint8_t* level, int rows, int cols, int last_h, int last_w,
                       const void* d_tables, const int64_t* offsets, uint8_t* out, hipStream_t s) {
  ProfScope prof("jpeg_write", s);
  hipLaunchKernelGGL(k_jpeg_tiles<true>, dim3((unsigned)((int64_t)rows * cols)), dim3(kJT), 0, s,
                     level, rows, cols, last_h, last_w, static_cast<const JpegTables*>(d_tables),
                     offsets, (int64_t*)nullptr, out);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
