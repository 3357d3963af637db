// jterator object tables (gfx950 / MI355X): what SegmentedObjects computes from
// an int32 label plane around the modules.
//
// Reference: tmlib/workflow/jterator/handles.py:399-551 and tmlib/image.py:796
//   labels     np.unique(value[value > 0])
//   bbox       mh.labeled.bbox(plane): per label [min_y, max_y + 1, min_x, max_x + 1]
//   centroids  mh.center_of_mass(plane, labels=plane): sum_y / n, sum_x / n
//   is_border  the label occurs in the first / last row or column
// One tmh_object_row per label 0..max_label of a plane holds the integer sums
// these are made of; every field is accumulated with integer atomics, so the
// table is exact and independent of scheduling.
//
// The table kernel walks the plane as label_tile.h describes: tiles, runs, an
// LDS table per tile, memory for what the table cannot hold.  Its own part: the
// columns of a run are consecutive, so its pixel count is the distance to the
// next head bit and its column sum an arithmetic series -- no segmented scan is
// needed, the run's HEAD lane has both in closed form; sum_y is y * n.  An entry
// is flushed once: 8 global atomics per (label, tile) instead of per run.
#include <algorithm>
#include <climits>

#include "common.h"
#include "label_tile.h"

namespace tmh {

constexpr int kObjSlots = TMH_OBJECT_SLOTS;   // LDS table entries (22.5 KB)
constexpr int kObjProbe = TMH_OBJECT_PROBE;
constexpr int kObjBatch = 4;                  // row segments loaded ahead per wave

__global__ void k_label_minmax_init(int32_t* __restrict__ mx, int32_t* __restrict__ mn, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  mx[i] = INT_MIN;
  mn[i] = INT_MAX;
}

// per plane (blockIdx.y) the largest and smallest label: grid-stride loads,
// wave reduction, one atomic pair per wave
__global__ __launch_bounds__(256) void k_label_minmax(const int32_t* __restrict__ planes,
                                                      int64_t npx, int32_t* __restrict__ mx,
                                                      int32_t* __restrict__ mn) {
  const int32_t* p = planes + (int64_t)blockIdx.y * npx;
  int hi = INT_MIN, lo = INT_MAX;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (int64_t)gridDim.x * 256) {
    const int v = p[i];
    hi = v > hi ? v : hi;
    lo = v < lo ? v : lo;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int h2 = __shfl_xor(hi, o, 64), l2 = __shfl_xor(lo, o, 64);
    hi = h2 > hi ? h2 : hi;
    lo = l2 < lo ? l2 : lo;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(mx + blockIdx.y, hi);
    atomicMin(mn + blockIdx.y, lo);
  }
}

// rows while they accumulate: y1 / x1 hold the inclusive maximum (-1: none),
// y0 / x0 the minimum (INT_MAX: none); k_object_finalize gives them their
// documented form
__global__ void k_object_init(tmh_object_row* __restrict__ rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tmh_object_row r;
  r.n = r.sum_y = r.sum_x = 0;
  r.y0 = r.x0 = INT_MAX;
  r.y1 = r.x1 = -1;
  r.border = r.pad = 0;
  rows[i] = r;
}

__global__ void k_object_finalize(tmh_object_row* __restrict__ rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tmh_object_row r = rows[i];
  if (r.n == 0) {
    r.y0 = r.y1 = r.x0 = r.x1 = 0;
  } else {
    r.y1 += 1;
    r.x1 += 1;
  }
  rows[i] = r;
}

// one run (label L, row y, columns [xs, xs + len)) into a row in memory
__device__ __forceinline__ void object_add_global(tmh_object_row* row, unsigned int n,
                                                  unsigned long long sy, unsigned long long sx,
                                                  int y0, int y1, int x0, int x1,
                                                  unsigned int border) {
  atomicAdd(reinterpret_cast<unsigned long long*>(&row->n), (unsigned long long)n);
  atomicAdd(reinterpret_cast<unsigned long long*>(&row->sum_y), sy);
  atomicAdd(reinterpret_cast<unsigned long long*>(&row->sum_x), sx);
  atomicMin(&row->y0, y0);
  atomicMax(&row->y1, y1);
  atomicMin(&row->x0, x0);
  atomicMax(&row->x1, x1);
  if (border) atomicOr(reinterpret_cast<unsigned int*>(&row->border), 1u);
}

__global__ __launch_bounds__(256) void k_object_table(const int32_t* __restrict__ planes, int H,
                                                      int W, int tiles_x, int32_t max_label,
                                                      tmh_object_row* __restrict__ rows) {
  __shared__ int key[kObjSlots];
  __shared__ unsigned int cnt[kObjSlots], brd[kObjSlots];
  __shared__ unsigned long long sy[kObjSlots], sx[kObjSlots];
  __shared__ int y0[kObjSlots], y1[kObjSlots], x0[kObjSlots], x1[kObjSlots];
  for (int i = threadIdx.x; i < kObjSlots; i += 256) {
    key[i] = -1;
    cnt[i] = brd[i] = 0u;
    sy[i] = sx[i] = 0ull;
    y0[i] = x0[i] = INT_MAX;
    y1[i] = x1[i] = -1;
  }
  __syncthreads();
  const int64_t plane = blockIdx.y;
  const int32_t* img = planes + plane * (int64_t)H * W;
  tmh_object_row* prow = rows + plane * ((int64_t)max_label + 1);
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int r0 = ty * kTileRows, c0 = tx * kTileCols;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // kObjBatch of a wave's items are loaded before any is used
  for (int i0 = wv; i0 < kTileItems; i0 += kTileWaves * kObjBatch) {
    int lab[kObjBatch];
#pragma unroll
    for (int b = 0; b < kObjBatch; ++b) {
      const TileItem it = tile_item(i0 + b * kTileWaves, r0, c0, lane, H, W);
      lab[b] = it.valid ? img[(int64_t)it.y * W + it.x] : -1;
    }
#pragma unroll
    for (int b = 0; b < kObjBatch; ++b) {
      const TileItem it = tile_item(i0 + b * kTileWaves, r0, c0, lane, H, W);
      const int y = it.y, x = it.x, L = lab[b];
      const LabelRuns runs = label_runs(L, it.valid, lane);
      if (!runs.head || (unsigned)L > (unsigned)max_label) continue;
      const unsigned long long above = lane == 63 ? 0ull : runs.heads & (~0ull << (lane + 1));
      const int next = above ? __ffsll((long long)above) - 1 : runs.nv;
      const unsigned int len = (unsigned int)(next - lane);
      const int xe = x + (int)len - 1;
      const unsigned long long rsy = (unsigned long long)y * len;
      const unsigned long long rsx =
          (unsigned long long)x * len + (unsigned long long)len * (len - 1) / 2;
      const unsigned int border = (y == 0 || y == H - 1 || x == 0 || xe == W - 1) ? 1u : 0u;
      int h = label_slot(L);
      bool found = false;
      for (int t = 0; t < kObjProbe; ++t) {
        const int old = atomicCAS(&key[h], -1, L);
        if (old == -1 || old == L) {
          found = true;
          break;
        }
        h = (h + 1) & (kObjSlots - 1);
      }
      if (found) {
        atomicAdd(&cnt[h], len);
        atomicAdd(&sy[h], rsy);
        atomicAdd(&sx[h], rsx);
        atomicMin(&y0[h], y);
        atomicMax(&y1[h], y);
        atomicMin(&x0[h], x);
        atomicMax(&x1[h], xe);
        if (border) atomicOr(&brd[h], 1u);
      } else {
        object_add_global(prow + L, len, rsy, rsx, y, y, x, xe, border);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kObjSlots; i += 256) {
    const int L = key[i];
    if (L < 0) continue;
    object_add_global(prow + L, cnt[i], sy[i], sx[i], y0[i], y1[i], x0[i], x1[i], brd[i]);
  }
}

static_assert(sizeof(tmh_object_row) == 48, "tmh_object_row layout (include/tmhip.h)");

void launch_label_minmax(const int32_t* planes, int64_t n_planes, int64_t npx, int32_t* d_max,
                         int32_t* d_min, hipStream_t s) {
  if (n_planes <= 0) return;
  hipLaunchKernelGGL(k_label_minmax_init, dim3((unsigned)cdiv(n_planes, 256)), dim3(256), 0, s,
                     d_max, d_min, n_planes);
  // each thread reads at least 8 pixels where the plane has them
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(npx, 256 * 8), 2048));
  hipLaunchKernelGGL(k_label_minmax, dim3(blocks, (unsigned)n_planes), dim3(256), 0, s, planes, npx,
                     d_max, d_min);
  TMH_HIP(hipGetLastError());
}

void launch_object_table(const int32_t* planes, int64_t n_planes, int H, int W, int32_t max_label,
                         tmh_object_row* rows, hipStream_t s) {
  if (n_planes <= 0) return;
  ProfScope prof("objects", s);
  const int64_t n_rows = n_planes * ((int64_t)max_label + 1);
  const dim3 rg((unsigned)cdiv(n_rows, 256));
  hipLaunchKernelGGL(k_object_init, rg, dim3(256), 0, s, rows, n_rows);
  const int tiles_x = (int)cdiv(W, kTileCols), tiles_y = (int)cdiv(H, kTileRows);
  hipLaunchKernelGGL(k_object_table, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_planes),
                     dim3(256), 0, s, planes, H, W, tiles_x, max_label, rows);
  hipLaunchKernelGGL(k_object_finalize, rg, dim3(256), 0, s, rows, n_rows);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
