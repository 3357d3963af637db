// JPEG decoding of pyramid tiles, two kernels over
// jpeg_core.h's arithmetic (shared with the host build the CPU suite checks):
//
// k_jpeg_roundtrip: every tile of a tile-major level [rows][cols][256][256]
//   uint8 as libjpeg decodes it from the file k_jpeg_tiles writes for it --
//   tmlib/models/tile.py:97-105, the getter through which
//   _create_lower_zoom_level_tiles (tmlib/workflow/illuminati/api.py:503-573)
//   reads the level above.  Huffman coding is lossless, so no file is made:
//   per 8 x 8 block the forward DCT, the quantiser, its inverse and the
//   inverse DCT, a block per thread in registers.
//
// k_jpeg_decode_tiles: stored files (tmlib/image.py:993-1037
//   PyramidTile.create_from_binary) back into tile storage.  Entropy decoding
//   of a file is sequential; a workgroup takes a file, one lane decodes a
//   strip of blocks into LDS, then a block per thread runs the inverse DCT.
#include "common.h"
#include "jpeg_core.h"

namespace tmh {

namespace {

constexpr int kTile = 256;
constexpr int64_t kTileBytes = (int64_t)kTile * kTile;
constexpr int kDT = 128;  // threads per workgroup = blocks per strip

// the quantisers of a call, passed by value: every index is a constant after
// unrolling, so they are scalar operands
struct JpegQuant {
  uint32_t recip[64];
  uint16_t qv[64];
};

// rows y0 .. y0 + 7 of a tile's columns 8 bx .. 8 bx + 7: the block's samples
// inside the tile's H x W, 0 outside
__device__ __forceinline__ void store_block(uint8_t* tile, const int (&d)[64], int by, int bx,
                                            int H, int W) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint64_t v = 8 * by + r < H ? jpeg_pack_row(d, r, W - 8 * bx) : 0ull;
    *reinterpret_cast<uint64_t*>(tile + (8 * by + r) * kTile + 8 * bx) = v;
  }
}

__device__ __forceinline__ void store_zero_block(uint8_t* tile, int by, int bx) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    *reinterpret_cast<uint64_t*>(tile + (8 * by + r) * kTile + 8 * bx) = 0ull;
}

// One workgroup per tile; thread i of a strip owns block slot s0 + i of the
// tile's 32 x 32: 32 neighbouring lanes read and write 256 contiguous bytes
// of a row.  Every byte of the output tile is written once: the samples
// inside the tile's extent, 0 outside it.
__global__ __launch_bounds__(kDT) void k_jpeg_roundtrip(const uint8_t* __restrict__ level, int rows,
                                                        int cols, int last_h, int last_w,
                                                        const JpegQuant q,
                                                        uint8_t* __restrict__ out) {
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int ty = (int)(t / cols), tx = (int)(t - (int64_t)ty * cols);
  const int H = ty == rows - 1 ? last_h : kTile, W = tx == cols - 1 ? last_w : kTile;
  const int bh = (H + 7) >> 3, bw = (W + 7) >> 3;
  const uint8_t* src = level + t * kTileBytes;
  uint8_t* dst = out + t * kTileBytes;
  for (int s0 = 0; s0 < 1024; s0 += kDT) {
    const int by = (s0 + tid) >> 5, bx = tid & 31;
    if (by < bh && bx < bw) {
      int d[64];
      jpeg_load_block(src, kTile, H, W, by, bx, d);
      jpeg_roundtrip_block(d, q);
      store_block(dst, d, by, bx, H, W);
    } else {
      store_zero_block(dst, by, bx);
    }
  }
}

struct JpegDecodeShared {
  JpegDecodeTables t;
  uint32_t coef[kDT * kJpegCoefPitch];  // per block 64 int16, natural order, two to a word
  JpegFileInfo info;
  int status;
};

struct PutLds {
  int16_t* c;
  __device__ __forceinline__ void operator()(int i, int v) { c[i] = (int16_t)v; }
};

// One workgroup per file.  Thread 0 walks the header; then per strip of 128
// blocks (raster order, the order of the coded segment): the strip's
// coefficients are zeroed, thread 0 decodes the strip's symbols into them
// (the bit reader and the DC predictor carry on in its registers), and every
// thread dequantises, inverts and stores one block.  Reads stay inside the
// file (jpeg_parse_header and JpegBitReader are bounded by its size), writes
// inside the tile's 64 KB (block slots are below 32 x 32 by SOF0's check).
// A file that fails leaves a tile of zeros.
__global__ __launch_bounds__(kDT) void k_jpeg_decode_tiles(
    const uint8_t* __restrict__ blob, const int64_t* __restrict__ offsets,
    const JpegDecodeTables* __restrict__ tables, uint8_t* __restrict__ tiles,
    int32_t* __restrict__ dims, int32_t* __restrict__ status) {
  __shared__ JpegDecodeShared S;
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const uint8_t* f = blob + offsets[t];
  const int64_t n = offsets[t + 1] - offsets[t];
  uint8_t* tile = tiles + t * kTileBytes;

  for (int i = tid; i < (int)(sizeof(JpegDecodeTables) / 4); i += kDT)
    reinterpret_cast<uint32_t*>(&S.t)[i] = reinterpret_cast<const uint32_t*>(tables)[i];
  __syncthreads();
  if (tid == 0) S.status = jpeg_parse_header(f, n, S.t, &S.info);
  __syncthreads();

  int H = 0, W = 0, bh = 0, bw = 0;
  if (S.status == kJpegOk) {
    H = S.info.height;
    W = S.info.width;
    bh = (H + 7) >> 3;
    bw = (W + 7) >> 3;
    const int nblk = bh * bw;
    JpegBitReader reader(f, S.info.scan, n);
    int dc = 0;
    for (int s0 = 0; s0 < nblk; s0 += kDT) {
      for (int i = tid; i < kDT * kJpegCoefPitch; i += kDT) S.coef[i] = 0u;
      __syncthreads();
      if (tid == 0) {
        const int count = min(kDT, nblk - s0);
        int st = kJpegOk;
        for (int b = 0; b < count && st == kJpegOk; ++b) {
          PutLds put{reinterpret_cast<int16_t*>(S.coef + b * kJpegCoefPitch)};
          st = jpeg_decode_block(reader, S.t, &dc, put);
        }
        if (st == kJpegOk && s0 + kDT >= nblk && !reader.at_eoi()) st = kJpegCorrupt;
        if (st != kJpegOk) S.status = st;
      }
      __syncthreads();
      if (S.status != kJpegOk) break;  // the same for every thread
      const int b = s0 + tid;
      if (b < nblk) {
        const uint32_t* w = S.coef + tid * kJpegCoefPitch;
        int c[64];
#pragma unroll
        for (int i = 0; i < 64; ++i)
          c[i] = (int)(int16_t)(w[i >> 1] >> (16 * (i & 1))) * (int)S.info.q[i];
        jpeg_idct_block(c);
        const int by = b / bw;
        store_block(tile, c, by, b - by * bw, H, W);
      }
      __syncthreads();  // before the coefficients are zeroed again
    }
  }
  const bool ok = S.status == kJpegOk;
  // what no block covers (everything, after a failure): 8 bytes at a time
  for (int i = tid; i < kTile * 32; i += kDT) {
    const int row = i >> 5, cx = i & 31;
    if (!ok || row >= 8 * bh || cx >= bw)
      *reinterpret_cast<uint64_t*>(tile + row * kTile + 8 * cx) = 0ull;
  }
  if (tid == 0) {
    dims[2 * t] = ok ? H : 0;
    dims[2 * t + 1] = ok ? W : 0;
    status[t] = S.status;
  }
}

}  // namespace

void launch_jpeg_roundtrip(const uint8_t* level, int rows, int cols, int last_h, int last_w,
                           int quality, uint8_t* out, hipStream_t s) {
  ProfScope prof("jpeg_roundtrip", s);
  JpegTables t;
  jpeg_build_tables(quality, &t);
  JpegQuant q;
  memcpy(q.recip, t.recip, sizeof(q.recip));
  memcpy(q.qv, t.qv, sizeof(q.qv));
  hipLaunchKernelGGL(k_jpeg_roundtrip, dim3((unsigned)((int64_t)rows * cols)), dim3(kDT), 0, s,
                     level, rows, cols, last_h, last_w, q, out);
  TMH_HIP(hipGetLastError());
}

size_t jpeg_decode_tables_bytes() { return sizeof(JpegDecodeTables); }
void jpeg_decode_tables_host(void* tables) {
  jpeg_build_decode_tables(static_cast<JpegDecodeTables*>(tables));
}

void launch_jpeg_decode_tiles(const uint8_t* blob, const int64_t* offsets, int64_t n,
                              const void* d_tables, uint8_t* tiles, int32_t* dims,
                              int32_t* status, hipStream_t s) {
  ProfScope prof("jpeg_decode_tiles", s);
  hipLaunchKernelGGL(k_jpeg_decode_tiles, dim3((unsigned)n), dim3(kDT), 0, s, blob, offsets,
                     static_cast<const JpegDecodeTables*>(d_tables), tiles, dims, status);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
