// illuminati tile pyramid (tmlib/workflow/illuminati/api.py:356-573): the base
// tiles gathered from the chain's [n][H][W] uint8 sites, and the halving of
// one level of tiles into the next.  Tile-major storage: a level is
// [tile_rows][tile_cols][256][256] uint8, every tile 64 KB contiguous; a
// ragged tile (last row / column of a level) sits in its tile's top left
// corner at the same 256-byte row pitch, zeros around it.
#include "common.h"

namespace tmh {

namespace {

typedef unsigned int pyr_u32x4 __attribute__((ext_vector_type(4)));
constexpr int kTile = 256;
constexpr int64_t kTileBytes = (int64_t)kTile * kTile;

// 16 bytes at any byte address, as one unaligned vector load (global memory
// takes unaligned dwordx4 addresses on gfx950)
__device__ __forceinline__ pyr_u32x4 load16_any(const uint8_t* p) {
  pyr_u32x4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// One workgroup per tile; a thread owns the 16-byte column group (tid & 15)
// of the 16 rows (tid >> 4) + 16 j and writes each of them once: the bytes of
// the tile's rectangle that covers them, else 0.
// Fast path, per rectangle that spans the thread's 16 columns: its rows in
// batches of kBatch loads issued back to back, then their stores (one load in
// flight per thread left the pass latency bound: 0.62 of the box's flat copy,
// DESIGN.md section 12).  A row outside the rectangle loads the nearest row
// inside it (in bounds, not stored).  Rows no such rectangle covers -- tile
// borders, background, spacer tiles -- take the general path: every rectangle
// against the row, byte loads where one covers part of the group.  The
// rectangles of a tile are disjoint, so the order does not matter.
// (site_bytes_total, the sites' extent, is not read: the unaligned loads stay
// inside their rectangle.)
constexpr int kBatch = 8;
constexpr int kXcds = 8;

__global__ __launch_bounds__(256) void k_tiles_base(const uint8_t* __restrict__ sites,
                                                    int64_t site_bytes_total, int H, int W,
                                                    const tmh_tile_rect* __restrict__ rects,
                                                    const int* __restrict__ tbeg,
                                                    uint8_t* __restrict__ tiles, int64_t n_tiles,
                                                    int64_t per_xcd) {
  // Workgroups go round the 8 XCDs in launch order: XCD x takes tiles
  // [x per_xcd, (x + 1) per_xcd) in order, so tiles that are neighbours in a
  // tile row -- they share the cache lines at their common edge and the DRAM
  // pages of their source rows -- run at about the same time behind one L2.
  const int64_t t = (int64_t)(blockIdx.x % kXcds) * per_xcd + blockIdx.x / kXcds;
  if (t >= n_tiles) return;
  const int b = tbeg[t], e = tbeg[t + 1];
  const int cx = (threadIdx.x & 15) * 16;
  const int r0 = threadIdx.x >> 4;
  uint8_t* dst = tiles + t * kTileBytes + cx;
  unsigned done = 0;  // bit j: row r0 + 16 j is written
  for (int k = b; k < e; ++k) {
    const tmh_tile_rect q = rects[k];
    if (cx < q.dst_x || cx + 16 > q.dst_x + q.width) continue;
    const uint8_t* src = sites + ((int64_t)q.site * H + q.src_y) * (int64_t)W + q.src_x + (cx - q.dst_x);
#pragma unroll
    for (int j0 = 0; j0 < 16; j0 += kBatch) {
      const int first = r0 + 16 * j0 - q.dst_y;  // rectangle row of the batch's first row
      if (first + 16 * (kBatch - 1) < 0 || first >= q.height) continue;
      pyr_u32x4 v[kBatch];
#pragma unroll
      for (int i = 0; i < kBatch; ++i) {
        const int dy = min(max(first + 16 * i, 0), q.height - 1);
        v[i] = load16_any(src + (int64_t)dy * W);
      }
#pragma unroll
      for (int i = 0; i < kBatch; ++i) {
        const int dy = first + 16 * i;
        if (dy >= 0 && dy < q.height) {
          *reinterpret_cast<pyr_u32x4*>(dst + (int64_t)(r0 + 16 * (j0 + i)) * kTile) = v[i];
          done |= 1u << (j0 + i);
        }
      }
    }
  }
  if (done == 0xFFFFu) return;
  for (int j = 0; j < 16; ++j) {
    if (done >> j & 1u) continue;
    const int r = r0 + 16 * j;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int k = b; k < e; ++k) {
      const tmh_tile_rect q = rects[k];
      const int dy = r - q.dst_y;
      if (dy < 0 || dy >= q.height) continue;
      const int c0 = max(cx, q.dst_x), c1 = min(cx + 16, q.dst_x + q.width);
      if (c0 >= c1) continue;
      // the source byte of column cx (outside the rectangle when c0 > cx:
      // only columns [c0, c1) are read)
      const uint8_t* src =
          sites + ((int64_t)q.site * H + q.src_y + dy) * (int64_t)W + q.src_x + (cx - q.dst_x);
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (cx + i >= c0 && cx + i < c1) w[i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
    }
    pyr_u32x4 v;
    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    *reinterpret_cast<pyr_u32x4*>(dst + (int64_t)r * kTile) = v;
  }
}

// four output bytes from eight source bytes of two rows: per pixel
// (a + b + c + d + 2) >> 2, two pixels to a word in 16-bit lanes
__device__ __forceinline__ uint32_t shrink4(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  const uint32_t m = 0x00FF00FFu;
  const uint32_t p0 = (((a0 & m) + ((a0 >> 8) & m) + (b0 & m) + ((b0 >> 8) & m) + 0x00020002u) >> 2) & m;
  const uint32_t p1 = (((a1 & m) + ((a1 >> 8) & m) + (b1 & m) + ((b1 >> 8) & m) + 0x00020002u) >> 2) & m;
  return ((p0 | (p0 >> 8)) & 0xFFFFu) | ((p1 | (p1 >> 8)) << 16);
}

// One workgroup per output tile (y, x): the mosaic of source tiles
// (2y..2y+1, 2x..2x+1) that exist, halved.  A thread's 16 output bytes of a
// row come from 32 source bytes of two rows of one source tile.  A mosaic
// with an odd side is left to the host: its output tile is not written.
__global__ __launch_bounds__(256) void k_pyramid_shrink2(const uint8_t* __restrict__ src, int R,
                                                         int C, int last_h, int last_w,
                                                         uint8_t* __restrict__ dst, int OC) {
  const int y = blockIdx.x / OC, x = blockIdx.x - y * OC;
  const int ty = 2 * y, tx = 2 * x;
  const int mh = (ty == R - 1 ? last_h : kTile) + (ty + 1 < R ? (ty + 1 == R - 1 ? last_h : kTile) : 0);
  const int mw = (tx == C - 1 ? last_w : kTile) + (tx + 1 < C ? (tx + 1 == C - 1 ? last_w : kTile) : 0);
  if ((mh | mw) & 1) return;
  const int oh = mh >> 1, ow = mw >> 1;
  const int cx = (threadIdx.x & 15) * 16;
  uint8_t* out = dst + (int64_t)blockIdx.x * kTileBytes + cx;
  const int sc = tx + (cx >> 7);  // source tile column of this thread's bytes
  const int lc = (2 * cx) & (kTile - 1);
  for (int r = threadIdx.x >> 4; r < kTile; r += 16) {
    pyr_u32x4 v = {0u, 0u, 0u, 0u};
    const int sr = ty + (r >> 7);
    if (r < oh && cx < ow && sr < R && sc < C) {
      const uint8_t* p = src + ((int64_t)sr * C + sc) * kTileBytes +
                         (int64_t)((2 * r) & (kTile - 1)) * kTile + lc;
      const pyr_u32x4 a0 = *reinterpret_cast<const pyr_u32x4*>(p);
      const pyr_u32x4 a1 = *reinterpret_cast<const pyr_u32x4*>(p + 16);
      const pyr_u32x4 b0 = *reinterpret_cast<const pyr_u32x4*>(p + kTile);
      const pyr_u32x4 b1 = *reinterpret_cast<const pyr_u32x4*>(p + kTile + 16);
      uint32_t w[4] = {shrink4(a0.x, a0.y, b0.x, b0.y), shrink4(a0.z, a0.w, b0.z, b0.w),
                       shrink4(a1.x, a1.y, b1.x, b1.y), shrink4(a1.z, a1.w, b1.z, b1.w)};
      const int nb = ow - cx;  // output bytes of this group inside the tile
      if (nb < 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int keep = nb - 4 * j;  // bytes of word j to keep
          w[j] = keep >= 4 ? w[j] : keep <= 0 ? 0u : (w[j] & (0xFFFFFFFFu >> (8 * (4 - keep))));
        }
      }
      v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    }
    *reinterpret_cast<pyr_u32x4*>(out + (int64_t)r * kTile) = v;
  }
}

}  // namespace

void launch_tiles_base(const uint8_t* sites, int64_t n_sites, int H, int W,
                       const tmh_tile_rect* d_rects, const int* d_tbeg, uint8_t* tiles,
                       int64_t n_tiles, hipStream_t s) {
  ProfScope prof("tiles_base", s);
  const int64_t total = n_sites * H * W;
  const int64_t per_xcd = cdiv(n_tiles, kXcds);
  const dim3 grid((unsigned)(per_xcd * kXcds));
  hipLaunchKernelGGL(k_tiles_base, grid, dim3(256), 0, s, sites, total, H, W, d_rects, d_tbeg,
                     tiles, n_tiles, per_xcd);
  TMH_HIP(hipGetLastError());
}

void launch_pyramid_shrink2(const uint8_t* src, int R, int C, int last_h, int last_w, uint8_t* dst,
                            hipStream_t s) {
  ProfScope prof("pyramid_shrink2", s);
  const int OR = (R + 1) / 2, OC = (C + 1) / 2;
  hipLaunchKernelGGL(k_pyramid_shrink2, dim3((unsigned)((int64_t)OR * OC)), dim3(256), 0, s, src, R,
                     C, last_h, last_w, dst, OC);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
