// jterator intensity measurements (gfx950 / MI355X): per label of an int32
// label plane and per channel the integer row (n, sum, sum of squares, min,
// max) of the intensity values under the label, and the five features taken
// from the rows (intensity_core.h).  DESIGN.md section 27.
//
// The table kernel walks the plane as label_tile.h describes: tiles, runs, an
// LDS table per tile, memory for what the table cannot hold.  Its own part: a
// run's sums have no closed form here, so the wave does a segmented inclusive
// scan (sum, sum of squares, min, max per channel, through DPP moves; steps no
// lane needs are skipped) and the LAST lane of each run, which then holds the
// run's totals, updates the table: one entry per label with n and, per channel
// of the pass, sum, sum_sq, min, max.
//
// Within a tile n <= 8,192, so a tile's sum (< 2^29) is kept in 32 bits and
// only sum_sq (< 2^45) in 64.  A pass holds up to kIntPass channels (44 KB of
// LDS at four); more channels are more passes, each reading the labels again.
#include <algorithm>
#include <climits>

#include "common.h"
#include "intensity_core.h"
#include "label_tile.h"

namespace tmh {

constexpr int kIntSlots = TMH_INTENSITY_SLOTS;
constexpr int kIntProbe = TMH_INTENSITY_PROBE;
constexpr int kIntPass = TMH_INTENSITY_PASS_CHANNELS;
constexpr int kIntBatch = 2;  // row segments loaded ahead per wave

struct IntensityJob {
  const int32_t* labels;
  const void* pixels;
  int H, W, tiles_x;
  int32_t max_label;
  int n_channels, c0, nc;  // channels of a row, first channel of the pass, channels in the pass
  int64_t cs, ps, rs, xs;
  tmh_intensity_row* rows;
};

// rows while they accumulate: min holds UINT_MAX until a pixel arrives
__global__ void k_intensity_init(tmh_intensity_row* __restrict__ rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tmh_intensity_row r;
  r.sum = r.sum_sq = 0ull;
  r.n = 0;
  r.min = UINT_MAX;
  r.max = 0u;
  rows[i] = r;
}

__global__ void k_intensity_fix(tmh_intensity_row* __restrict__ rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (rows[i].n == 0) rows[i].min = 0u;
}

__device__ __forceinline__ void intensity_add_global(tmh_intensity_row* row, unsigned int n,
                                                     unsigned long long sum,
                                                     unsigned long long sum_sq, unsigned int lo,
                                                     unsigned int hi) {
  atomicAdd(reinterpret_cast<unsigned long long*>(&row->sum), sum);
  atomicAdd(reinterpret_cast<unsigned long long*>(&row->sum_sq), sum_sq);
  atomicAdd(reinterpret_cast<unsigned long long*>(&row->n), (unsigned long long)n);
  atomicMin(&row->min, lo);
  atomicMax(&row->max, hi);
}

// Another lane's register through the DPP path (VALU, no LDS traffic): CTRL
// 0x110 + n is row_shr:n (lane - n of the same row of 16), 0x142 row_bcast:15
// (lane 15 of a row to every lane of the next row), 0x143 row_bcast:31 (lane 31
// to lanes 32..63).  A lane without a source keeps its own value.  All 64 lanes
// must be active.
template <int CTRL>
__device__ __forceinline__ unsigned int dpp32(unsigned int v) {
  return (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}

// one step of the segmented inclusive scan of C channels
template <int CTRL, int C>
__device__ __forceinline__ void scan_step(bool take, unsigned int (&s)[C],
                                          unsigned long long (&q)[C], unsigned int (&lo)[C],
                                          unsigned int (&hi)[C]) {
  if (__ballot(take) == 0ull) return;  // the whole wave
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const unsigned int s2 = dpp32<CTRL>(s[j]), lo2 = dpp32<CTRL>(lo[j]), hi2 = dpp32<CTRL>(hi[j]);
    const unsigned long long q2 = ((unsigned long long)dpp32<CTRL>((unsigned int)(q[j] >> 32)) << 32) |
                                  dpp32<CTRL>((unsigned int)q[j]);
    if (take) {
      s[j] += s2;
      q[j] += q2;
      lo[j] = lo2 < lo[j] ? lo2 : lo[j];
      hi[j] = hi2 > hi[j] ? hi2 : hi[j];
    }
  }
}

template <typename T, int C>
__global__ __launch_bounds__(256) void k_intensity_table(const IntensityJob a) {
  __shared__ int key[kIntSlots];
  __shared__ unsigned int cnt[kIntSlots];
  __shared__ unsigned int sm[C][kIntSlots], mn[C][kIntSlots], mx[C][kIntSlots];
  __shared__ unsigned long long sq[C][kIntSlots];
  for (int i = threadIdx.x; i < kIntSlots; i += 256) {
    key[i] = -1;
    cnt[i] = 0u;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      sm[j][i] = mx[j][i] = 0u;
      mn[j][i] = UINT_MAX;
      sq[j][i] = 0ull;
    }
  }
  __syncthreads();
  const int H = a.H, W = a.W, nc = a.nc;
  const int64_t plane = blockIdx.y;
  const int32_t* img = a.labels + plane * (int64_t)H * W;
  const T* pix = static_cast<const T*>(a.pixels) + a.c0 * a.cs + plane * a.ps;
  tmh_intensity_row* prow =
      a.rows + plane * ((int64_t)a.max_label + 1) * a.n_channels + a.c0;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int r0 = ty * kTileRows, c0 = tx * kTileCols;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // kIntBatch of a wave's items are loaded before any is used
  for (int i0 = wv; i0 < kTileItems; i0 += kTileWaves * kIntBatch) {
    int lab[kIntBatch];
    unsigned int val[kIntBatch][C];
#pragma unroll
    for (int b = 0; b < kIntBatch; ++b) {
      const TileItem it = tile_item(i0 + b * kTileWaves, r0, c0, lane, H, W);
      const bool valid = it.valid;
      lab[b] = valid ? img[(int64_t)it.y * W + it.x] : -1;
      const int64_t at = (int64_t)it.y * a.rs + (int64_t)it.x * a.xs;
#pragma unroll
      for (int j = 0; j < C; ++j)
        val[b][j] = (valid && j < nc) ? (unsigned int)pix[at + j * a.cs] : 0u;
    }
#pragma unroll
    for (int b = 0; b < kIntBatch; ++b) {
      const bool valid = tile_item(i0 + b * kTileWaves, r0, c0, lane, H, W).valid;
      const int L = lab[b];
      const LabelRuns runs = label_runs(L, valid, lane);
      if (runs.nv == 0) continue;  // the whole wave
      // the run of a lane starts at the highest head at or below it (lane 0 is one)
      const unsigned long long upto = runs.heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
      const int start = 63 - __clzll((long long)(upto | 1ull));
      const bool tail = valid && (lane + 1 == runs.nv || ((runs.heads >> (lane + 1)) & 1ull));
      unsigned int s[C], lo[C], hi[C];
      unsigned long long q[C];
#pragma unroll
      for (int j = 0; j < C; ++j) {
        s[j] = lo[j] = hi[j] = val[b][j];
        q[j] = (unsigned long long)val[b][j] * val[b][j];
      }
      // in-row steps (lanes 16 r .. 16 r + 15), then lane 15 of a row to the next
      // row and lane 31 to the upper half; a lane takes what arrives only when
      // the sending lane belongs to its run, and a step no lane takes is skipped
      const int rl = lane & 15, since = lane - start;
      scan_step<0x111, C>(valid && rl >= 1 && since >= 1, s, q, lo, hi);
      scan_step<0x112, C>(valid && rl >= 2 && since >= 2, s, q, lo, hi);
      scan_step<0x114, C>(valid && rl >= 4 && since >= 4, s, q, lo, hi);
      scan_step<0x118, C>(valid && rl >= 8 && since >= 8, s, q, lo, hi);
      scan_step<0x142, C>(valid && (lane & 16) && start < (lane & ~15), s, q, lo, hi);
      scan_step<0x143, C>(valid && lane >= 32 && start < 32, s, q, lo, hi);
      if (!tail || (unsigned)L > (unsigned)a.max_label) continue;
      const unsigned int len = (unsigned int)(lane - start + 1);
      int h = label_slot(L);
      bool found = false;
      for (int t = 0; t < kIntProbe; ++t) {
        const int old = atomicCAS(&key[h], -1, L);
        if (old == -1 || old == L) {
          found = true;
          break;
        }
        h = (h + 1) & (kIntSlots - 1);
      }
      if (found) {
        atomicAdd(&cnt[h], len);
#pragma unroll
        for (int j = 0; j < C; ++j) {
          if (j >= nc) break;
          atomicAdd(&sm[j][h], s[j]);
          atomicAdd(&sq[j][h], q[j]);
          atomicMin(&mn[j][h], lo[j]);
          atomicMax(&mx[j][h], hi[j]);
        }
      } else {
        tmh_intensity_row* row = prow + (int64_t)L * a.n_channels;
#pragma unroll
        for (int j = 0; j < C; ++j) {
          if (j >= nc) break;
          intensity_add_global(row + j, len, s[j], q[j], lo[j], hi[j]);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kIntSlots; i += 256) {
    const int L = key[i];
    if (L < 0) continue;
    tmh_intensity_row* row = prow + (int64_t)L * a.n_channels;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      if (j >= nc) break;
      intensity_add_global(row + j, cnt[i], sm[j][i], sq[j][i], mn[j][i], mx[j][i]);
    }
  }
}

// one thread per (group, label, channel): the group's planes merged, then the features
__global__ void k_intensity_features(const tmh_intensity_row* __restrict__ rows, int64_t per_group,
                                     int64_t plane_rows, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t g = i / plane_rows, k = i - g * plane_rows;  // k = label * n_channels + channel
  const tmh_intensity_row* p = rows + g * per_group * plane_rows + k;
  tmh_intensity_row r = p[0];
  for (int64_t z = 1; z < per_group; ++z) ic_merge(&r, p[z * plane_rows]);
  double f[5];
  ic_features(r, f);
#pragma unroll
  for (int j = 0; j < 5; ++j) out[i * 5 + j] = f[j];
}

static_assert(kIntPass == 4, "k_intensity_table is instantiated for 1, 2 and 4 channels");
static_assert(kTileRows * kTileCols <= 65536, "a tile's sum of 16-bit values is kept in 32 bits");
static_assert(sizeof(tmh_intensity_row) == 32, "tmh_intensity_row layout (include/tmhip.h)");

template <typename T>
static void launch_pass(const IntensityJob& job, dim3 grid, hipStream_t s) {
  if (job.nc == 1)
    hipLaunchKernelGGL((k_intensity_table<T, 1>), grid, dim3(256), 0, s, job);
  else if (job.nc == 2)
    hipLaunchKernelGGL((k_intensity_table<T, 2>), grid, dim3(256), 0, s, job);
  else
    hipLaunchKernelGGL((k_intensity_table<T, 4>), grid, dim3(256), 0, s, job);
}

void launch_intensity_table(const int32_t* labels, const void* pixels, int elem_bytes,
                            int64_t n_planes, int H, int W, int n_channels, int64_t cs, int64_t ps,
                            int64_t rs, int64_t xs, int32_t max_label, tmh_intensity_row* rows,
                            hipStream_t s) {
  if (n_planes <= 0) return;
  ProfScope prof("intensity", s);
  const int64_t n_rows = n_planes * ((int64_t)max_label + 1) * n_channels;
  const dim3 rg((unsigned)cdiv(n_rows, 256));
  hipLaunchKernelGGL(k_intensity_init, rg, dim3(256), 0, s, rows, n_rows);
  IntensityJob job{labels, pixels, H, W, (int)cdiv(W, kTileCols), max_label, n_channels, 0, 0,
                   cs, ps, rs, xs, rows};
  const dim3 grid((unsigned)(job.tiles_x * (int)cdiv(H, kTileRows)), (unsigned)n_planes);
  for (int c0 = 0; c0 < n_channels; c0 += kIntPass) {
    job.c0 = c0;
    job.nc = std::min(kIntPass, n_channels - c0);
    if (elem_bytes == 2)
      launch_pass<uint16_t>(job, grid, s);
    else
      launch_pass<uint8_t>(job, grid, s);
  }
  hipLaunchKernelGGL(k_intensity_fix, rg, dim3(256), 0, s, rows, n_rows);
  TMH_HIP(hipGetLastError());
}

void launch_intensity_features(const tmh_intensity_row* rows, int64_t n_planes, int64_t n_groups,
                               int32_t max_label, int n_channels, double* out, hipStream_t s) {
  if (n_groups <= 0) return;
  ProfScope prof("intensity_features", s);
  const int64_t plane_rows = ((int64_t)max_label + 1) * n_channels, n = n_groups * plane_rows;
  hipLaunchKernelGGL(k_intensity_features, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, rows,
                     n_planes / n_groups, plane_rows, n, out);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
