// The clustering tool (gfx950 / MI355X): RobustScaler's column statistics and
// k-means (k-means++ seeding, Lloyd) on row-major f64 feature tables.
//
// Reference: tmlib/tools/base.py:586-645 (Classifier.train_unsupervised /
// predict) through scikit-learn's RobustScaler and KMeans; the rules every
// kernel follows are restated in tests/clustering_literal.py.
//
// All arithmetic is f64.  X is [n][d], 1 <= d <= 256, 1 <= k <= 64,
// k * d <= 8,192 (the centres fit in 64 KB of LDS), n < 2^31.
//
// Determinism.  Nothing here adds floating-point values with atomics.  Every
// sum is taken over a partition of the rows that depends on (n, d, k) alone
// -- a launch has exactly one grid for a given shape -- in a fixed order:
//   * k_kmeans_assign owns one chunk of rows per workgroup; inside it a
//     thread owns (slice, feature) and adds its rows in ascending order, the
//     slices are added in ascending order, k_reduce_partials adds the chunks
//     in 32 fixed runs, each in ascending order, then the runs;
//   * k_sum_chunks / k_sum_final (potentials, inertia) and k_colsum (column
//     means and variances) do the same with their own fixed partitions;
//   * the seeding's prefix sum is defined once (prefix_of_block) and used by
//     both the block sums and the search, so it is monotone by construction.
// Counts and flags use integer atomics, which are exact in any order.
//
// Scaling on load.  Kernels that read X take optional center[d] / scale[d]
// and apply (x - c) / s -- one subtract, one divide, nothing to contract --
// as they load, so a scaled copy of X is never needed and the values are
// those k_robust_scale would have stored.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "table_load.h"

namespace tmh {

constexpr int kClThreads = 256;
constexpr int kClTileDoubles = 2048;   // a staged tile of rows (16 KB of LDS)
constexpr int kSeedBlock = 1024;       // rows per block of the seeding's prefix sum
constexpr int kSeedLane = kSeedBlock / 64;
constexpr int kSumChunk = 8192;        // elements per partial of k_sum_chunks
constexpr int kColChunk = 4096;        // rows per partial of k_colsum

__device__ __forceinline__ unsigned long long f64_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_f64(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// rows [r0, r0 + rows) of X, scaled, into tile[rows][d]: 16-byte loads where
// the tile starts on a 16-byte boundary (block-uniform), 8-byte loads otherwise
__device__ __forceinline__ void stage_tile(const double* __restrict__ X, int64_t r0, int rows, int d,
                                           const double* sc, bool has_sc, double* tile) {
  const double* src = X + r0 * d;
  const int cnt = rows * d;
  const double* c = has_sc ? sc : nullptr;
  const double* s = sc + 256;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const int pairs = cnt >> 1;
    for (int i = threadIdx.x; i < pairs; i += blockDim.x) {
      const double2 v = reinterpret_cast<const double2*>(src)[i];
      const int f0 = (2 * i) % d, f1 = f0 + 1 == d ? 0 : f0 + 1;
      tile[2 * i] = scaled(v.x, c, s, f0);
      tile[2 * i + 1] = scaled(v.y, c, s, f1);
    }
    if ((cnt & 1) && threadIdx.x == 0) tile[cnt - 1] = scaled(src[cnt - 1], c, s, (cnt - 1) % d);
  } else {
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) tile[i] = scaled(src[i], c, s, i % d);
  }
}

// ---- census ------------------------------------------------------------------
// cnt[f] = values of column f that are not NaN, cnt[d + f] = those that are +-inf
__global__ __launch_bounds__(kClThreads) void k_census(const double* __restrict__ X, int64_t total,
                                                       int d, unsigned long long* __restrict__ cnt) {
  __shared__ unsigned int c[512];
  for (int i = threadIdx.x; i < 512; i += kClThreads) c[i] = 0u;
  __syncthreads();
  // a block owns a run of whole elements; 2^20 of them at the most, so the
  // 32-bit LDS counters cannot wrap
  const int64_t per = 4096;
  const int64_t b0 = (int64_t)blockIdx.x * per;
  const int64_t b1 = b0 + per < total ? b0 + per : total;
  const unsigned int f0 = (unsigned int)(b0 % d);
  for (int64_t i = b0 + threadIdx.x; i < b1; i += kClThreads) {
    const double v = X[i];
    const int f = (int)((f0 + (unsigned int)(i - b0)) % (unsigned int)d);
    if (v == v) atomicAdd(&c[f], 1u);
    if (isinf(v)) atomicAdd(&c[256 + f], 1u);
  }
  __syncthreads();
  for (int f = threadIdx.x; f < d; f += kClThreads) {
    if (c[f]) atomicAdd(&cnt[f], (unsigned long long)c[f]);
    if (c[256 + f]) atomicAdd(&cnt[d + f], (unsigned long long)c[256 + f]);
  }
}

// ---- column sums in a fixed order ----------------------------------------------
// part[chunk][f] = sum over the chunk's rows of g(x_rf), NaN skipped:
// g = x (mean == nullptr) or (x - mean[f])^2.  Thread (s, f) of S = 256 / d
// slices adds rows s, s + S, ... in ascending order; the slices are added in
// ascending order.
__global__ __launch_bounds__(kClThreads) void k_colsum(const double* __restrict__ X, int64_t n,
                                                       int d, const double* __restrict__ cen,
                                                       const double* __restrict__ scl,
                                                       const double* __restrict__ mean,
                                                       double* __restrict__ part) {
  __shared__ double acc[kClThreads];
  const int S = kClThreads / d;
  const int s = threadIdx.x / d, f = threadIdx.x - s * d;
  const int64_t r0 = (int64_t)blockIdx.x * kColChunk;
  const int64_t r1 = r0 + kColChunk < n ? r0 + kColChunk : n;
  double a = 0.0;
  if (s < S) {
    const double c = cen ? cen[f] : 0.0, sc = cen ? scl[f] : 1.0, m = mean ? mean[f] : 0.0;
    for (int64_t r = r0 + s; r < r1; r += S) {
      double v = X[r * d + f];
      if (cen) v = (v - c) / sc;
      if (v != v) continue;
      if (mean) {
        const double t = v - m;
        a += t * t;
      } else {
        a += v;
      }
    }
  }
  acc[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < d) {
    double t = acc[threadIdx.x];
    for (int q = 1; q < S; ++q) t += acc[q * d + threadIdx.x];
    part[(int64_t)blockIdx.x * d + threadIdx.x] = t;
  }
}

// out[f] = (sum over chunks, ascending, of part[chunk][f]) / cnt[f]
__global__ void k_colsum_final(const double* __restrict__ part, int64_t chunks, int d,
                               const unsigned long long* __restrict__ cnt,
                               double* __restrict__ out) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= d) return;
  double t = 0.0;
  for (int64_t c = 0; c < chunks; ++c) t += part[c * d + f];
  out[f] = t / (double)cnt[f];
}

// ---- sums of a vector in a fixed order -------------------------------------------
// part[v][chunk] = sum of vec[v][chunk * kSumChunk ..): a thread adds its
// strided elements in ascending order, then a fixed LDS tree
__device__ __forceinline__ double block_tree_sum(double a, double* red) {
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = kClThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kClThreads) void k_sum_chunks(const double* __restrict__ vec, int64_t n,
                                                           int64_t chunks,
                                                           double* __restrict__ part) {
  __shared__ double red[kClThreads];
  const double* v = vec + (int64_t)blockIdx.y * n;
  const int64_t i0 = (int64_t)blockIdx.x * kSumChunk;
  const int64_t i1 = i0 + kSumChunk < n ? i0 + kSumChunk : n;
  double a = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kClThreads) a += v[i];
  const double r = block_tree_sum(a, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * chunks + blockIdx.x] = r;
}

__global__ __launch_bounds__(kClThreads) void k_sum_final(const double* __restrict__ part,
                                                          int64_t chunks,
                                                          double* __restrict__ out) {
  __shared__ double red[kClThreads];
  const double* p = part + (int64_t)blockIdx.x * chunks;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < chunks; i += kClThreads) a += p[i];
  const double r = block_tree_sum(a, red);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// ---- robust scale --------------------------------------------------------------
__global__ __launch_bounds__(kClThreads) void k_robust_scale(const double* __restrict__ X,
                                                             int64_t total, int d,
                                                             const double* __restrict__ cen,
                                                             const double* __restrict__ scl,
                                                             double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x;
  if (i >= total) return;
  const int f = (int)(i % d);
  out[i] = (X[i] - cen[f]) / scl[f];
}

// ---- order statistics: radix select ------------------------------------------------
// Per (column, rank) a prefix of the key's high bytes is followed; one pass
// counts, per (column, rank), the next byte of the keys under that prefix.
// A workgroup owns a run of rows and a group of G columns, G * r <= 128, so
// its tables are G * r * 256 counters = 128 KB of LDS at the most.
// state[(c * r + q) * 2] = prefix (high `pass` bytes), [.. + 1] = rank left
__global__ __launch_bounds__(kClThreads) void k_select_hist(
    const double* __restrict__ X, int64_t n, int d, int r, int G, int pass, int64_t rows_per_block,
    const unsigned long long* __restrict__ state, unsigned int* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned int h[];
  __shared__ unsigned long long pre[128];
  const int c0 = blockIdx.y * G;
  const int g_n = d - c0 < G ? d - c0 : G;
  const int tabs = g_n * r;
  for (int i = threadIdx.x; i < tabs * 256; i += kClThreads) h[i] = 0u;
  for (int i = threadIdx.x; i < tabs; i += kClThreads) pre[i] = state[((int64_t)c0 * r + i) * 2];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  const int shift = 56 - 8 * pass;
  // at most 2^20 rows x 128 columns: 32-bit item arithmetic
  const unsigned int items = (unsigned int)(r1 - r0) * (unsigned int)g_n;
  for (unsigned int it = threadIdx.x; it < items; it += kClThreads) {
    const unsigned int lr = it / (unsigned int)g_n;
    const int64_t row = r0 + lr;
    const int g = (int)(it - lr * (unsigned int)g_n);
    const double v = X[row * d + c0 + g];
    if (v != v) continue;
    const unsigned long long key = f64_key(v);
    const unsigned long long hi = pass == 0 ? 0ull : key >> (shift + 8);
    const unsigned int digit = (unsigned int)(key >> shift) & 255u;
    for (int q = 0; q < r; ++q)
      if (pass == 0 || pre[g * r + q] == hi) atomicAdd(&h[(g * r + q) * 256 + digit], 1u);
  }
  __syncthreads();
  unsigned int* out = hist + (int64_t)c0 * r * 256;
  for (int i = threadIdx.x; i < tabs * 256; i += kClThreads)
    if (h[i]) atomicAdd(&out[i], h[i]);
}

// one thread per (column, rank): the digit whose cumulative count passes the
// rank left; the table is zeroed for the next pass
__global__ void k_select_pick(unsigned long long* __restrict__ state,
                              unsigned int* __restrict__ hist, int tabs, int pass,
                              double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tabs) return;
  unsigned long long rank = state[2 * t + 1];
  unsigned int* h = hist + (int64_t)t * 256;
  int digit = 255;
  unsigned long long before = 0ull;
  for (int b = 0; b < 256; ++b) {
    const unsigned long long c = h[b];
    if (before + c > rank) {
      digit = b;
      break;
    }
    before += c;
  }
  for (int b = 0; b < 256; ++b) h[b] = 0u;
  const unsigned long long prefix = (pass == 0 ? 0ull : state[2 * t] << 8) | (unsigned long long)digit;
  state[2 * t] = prefix;
  state[2 * t + 1] = rank - before;
  if (pass == 7) out[t] = key_f64(prefix);
}

// ---- k-means: assign + per-chunk sums ----------------------------------------------
struct AssignGeom {
  int d, k, cs;      // features, clusters, stride of a centre row in LDS
  int R, T, S;       // tile rows, lanes per row, accumulation slices
  int64_t chunk;     // rows per workgroup
};

// LDS: centres[k][cs] | tile[R][d] | sums[S][k][d] (when psums) | lab[R] | cnt[k]
__global__ __launch_bounds__(kClThreads) void k_kmeans_assign(
    const double* __restrict__ X, int64_t n, AssignGeom g, const double* __restrict__ cen,
    const double* __restrict__ scl, const double* __restrict__ centres,
    const int32_t* __restrict__ prev, int32_t* __restrict__ labels, double* __restrict__ mind,
    int* __restrict__ changed, double* __restrict__ psums, unsigned int* __restrict__ pcounts) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double sc[512];
  const int d = g.d, k = g.k, cs = g.cs, R = g.R, T = g.T, S = g.S;
  double* cent = lds;
  double* tile = cent + k * cs;
  double* sums = tile + R * d;
  int* lab = reinterpret_cast<int*>(sums + (psums ? S * k * d : 0));
  unsigned int* cnt = reinterpret_cast<unsigned int*>(lab + R);
  const int tid = threadIdx.x;
  for (int i = tid; i < k * d; i += kClThreads) cent[(i / d) * cs + (i % d)] = centres[i];
  if (psums) {
    for (int i = tid; i < S * k * d; i += kClThreads) sums[i] = 0.0;
    for (int i = tid; i < k; i += kClThreads) cnt[i] = 0u;
  }
  stage_scaler(cen, scl, d, sc);
  __syncthreads();
  const int64_t c0 = (int64_t)blockIdx.x * g.chunk;
  const int64_t c1 = c0 + g.chunk < n ? c0 + g.chunk : n;
  const int RP = kClThreads / T;
  const int rr = tid / T, gg = tid - rr * T;
  int any_changed = 0;
  for (int64_t t0 = c0; t0 < c1; t0 += R) {
    const int rows = (int)(c1 - t0 < R ? c1 - t0 : R);
    stage_tile(X, t0, rows, d, sc, cen != nullptr, tile);
    __syncthreads();
    for (int rb = 0; rb < rows; rb += RP) {
      const int r = rb + rr;
      double best = INFINITY;
      int bj = 0x7fffffff;
      if (r < rows) {
        const double* x = tile + r * d;
        for (int j = gg; j < k; j += T) {
          const double* c = cent + j * cs;
          double a = 0.0;
          for (int f = 0; f < d; ++f) {
            const double t = x[f] - c[f];
            a += t * t;
          }
          if (a < best) {
            best = a;
            bj = j;
          }
        }
      }
      for (int o = T >> 1; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ob < best || (ob == best && oj < bj)) {
          best = ob;
          bj = oj;
        }
      }
      if (r < rows && gg == 0) {
        if (bj == 0x7fffffff) bj = 0;  // every distance overflowed
        lab[r] = bj;
        labels[t0 + r] = bj;
        if (mind) mind[t0 + r] = best;
        if (prev && prev[t0 + r] != bj) any_changed = 1;
      }
    }
    __syncthreads();
    if (psums) {
      if (tid < S * d) {
        const int s = tid / d, f = tid - s * d;
        double* mine = sums + (int64_t)s * k * d + f;
        for (int r = s; r < rows; r += S) mine[lab[r] * d] += tile[r * d + f];
      }
      for (int r = tid; r < rows; r += kClThreads) atomicAdd(&cnt[lab[r]], 1u);
    }
    __syncthreads();
  }
  if (any_changed) atomicOr(changed, 1);
  if (psums) {
    for (int i = tid; i < k * d; i += kClThreads) {
      double a = sums[i];
      for (int s = 1; s < S; ++s) a += sums[(int64_t)s * k * d + i];
      psums[(int64_t)blockIdx.x * k * d + i] = a;
    }
    for (int i = tid; i < k; i += kClThreads) pcounts[(int64_t)blockIdx.x * k + i] = cnt[i];
  }
}

// sums[i] = the sum over chunks of psums[chunk][i] in a fixed order: the chunks
// are cut into 32 runs of cdiv(chunks, 32), lane g adds run g in ascending
// order, lane 0 adds the 32 runs in ascending order.  8 values per workgroup;
// values kd .. kd + k - 1 are the member counts, added the same way in integers.
__global__ __launch_bounds__(kClThreads) void k_reduce_partials(
    const double* __restrict__ psums, const unsigned int* __restrict__ pcounts, int64_t chunks,
    int kd, int k, double* __restrict__ sums, long long* __restrict__ counts) {
  __shared__ double run[kClThreads];
  __shared__ long long irun[kClThreads];
  const int e = threadIdx.x >> 5, g = threadIdx.x & 31;
  const int i = blockIdx.x * 8 + e;
  const int64_t len = cdiv(chunks, 32);
  const int64_t c0 = g * len, c1 = c0 + len < chunks ? c0 + len : chunks;
  double a = 0.0;
  long long m = 0;
  if (i < kd) {
    for (int64_t c = c0; c < c1; ++c) a += psums[c * kd + i];
  } else if (i < kd + k) {
    for (int64_t c = c0; c < c1; ++c) m += pcounts[c * k + (i - kd)];
  }
  run[threadIdx.x] = a;
  irun[threadIdx.x] = m;
  __syncthreads();
  if (g != 0) return;
  if (i < kd) {
    double t = run[threadIdx.x];
    for (int q = 1; q < 32; ++q) t += run[threadIdx.x + q];
    sums[i] = t;
  } else if (i < kd + k) {
    long long t = 0;
    for (int q = 0; q < 32; ++q) t += irun[threadIdx.x + q];
    counts[i - kd] = t;
  }
}

// Empty clusters, the division and the centre shift; one workgroup.
// For each empty cluster in ascending index: the row with the largest mind
// not taken yet (ties: the lowest row) leaves its cluster and becomes the
// empty cluster's centre (scikit-learn's _relocate_empty_clusters_dense).
// A cluster left without members keeps its old centre.
__global__ __launch_bounds__(1024) void k_kmeans_finalize(
    const double* __restrict__ X, int64_t n, int d, int k, const double* __restrict__ cen,
    const double* __restrict__ scl, const int32_t* __restrict__ labels,
    const double* __restrict__ mind, double* __restrict__ sums, long long* __restrict__ counts,
    const double* __restrict__ old, double* __restrict__ centres_new, double* __restrict__ shift,
    int64_t* __restrict__ taken) {
  __shared__ double bv[1024];
  __shared__ long long bi[1024];
  __shared__ double red[1024];
  __shared__ int empty[64];
  const int tid = threadIdx.x;
  if (tid < k) empty[tid] = counts[tid] == 0;  // the empty set is fixed before any row moves
  __syncthreads();
  int n_taken = 0;
  for (int e = 0; e < k; ++e) {
    if (!empty[e]) continue;
    double best = -1.0;
    long long brow = -1;
    for (int64_t i = tid; i < n; i += 1024) {
      bool used = false;
      for (int q = 0; q < n_taken; ++q) used |= taken[q] == i;
      if (used) continue;
      const double v = mind[i];
      if (v > best) {
        best = v;
        brow = i;
      }
    }
    bv[tid] = best;
    bi[tid] = brow;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if (tid < o) {
        const double ov = bv[tid + o];
        const long long oi = bi[tid + o];
        if (oi >= 0 && (bi[tid] < 0 || ov > bv[tid] || (ov == bv[tid] && oi < bi[tid]))) {
          bv[tid] = ov;
          bi[tid] = oi;
        }
      }
      __syncthreads();
    }
    const long long row = bi[0];
    __syncthreads();
    if (row < 0) break;  // fewer rows than clusters: refused by the host before any launch
    const int from = labels[row];
    for (int f = tid; f < d; f += 1024) {
      const double x = scaled(X[row * d + f], cen, scl, f);
      sums[from * d + f] -= x;
      sums[e * d + f] = x;
    }
    if (tid == 0) {
      counts[from] -= 1;
      counts[e] = 1;
      taken[n_taken] = row;
    }
    n_taken += 1;
    __threadfence_block();
    __syncthreads();
  }
  double a = 0.0;
  for (int i = tid; i < k * d; i += 1024) {
    const long long c = counts[i / d];
    const double v = c > 0 ? sums[i] / (double)c : old[i];
    centres_new[i] = v;
    const double t = v - old[i];
    a += t * t;
  }
  red[tid] = a;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) *shift = red[0];
}

// ---- k-means++ seeding ---------------------------------------------------------------
// The inclusive prefix sum of closest[] at row i is DEFINED as
//   block_excl[b] + (lane_excl[l] + s)
// with b = i / 1024, l = (i % 1024) / 16, s the sum of the lane's values up to
// i added in ascending order, lane_excl the running sum of the lanes' totals
// in ascending order, block_excl the running sum of the blocks' totals.  Every
// term is a running sum of non-negative values and each level ends on the
// value the next begins with, so the prefix never decreases.
// lane_tot[64] in LDS -> lane_excl[65] (lane_excl[64] = the block's total)
__device__ __forceinline__ void prefix_of_block(const double* __restrict__ closest, int64_t n,
                                                int64_t b, double* vals, double* lane_excl) {
  const int l = threadIdx.x;  // 64 threads
  const int64_t i0 = b * kSeedBlock + (int64_t)l * kSeedLane;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < kSeedLane; ++e) {
    const int64_t i = i0 + e;
    const double v = i < n ? closest[i] : 0.0;
    vals[e] = v;
    s += v;
  }
  __shared__ double tot[64];
  tot[l] = s;
  __syncthreads();
  if (l == 0) {
    double run = 0.0;
    for (int q = 0; q < 64; ++q) {
      lane_excl[q] = run;
      run += tot[q];
    }
    lane_excl[64] = run;
  }
  __syncthreads();
}

__global__ __launch_bounds__(64) void k_seed_blocksums(const double* __restrict__ closest, int64_t n,
                                                       double* __restrict__ block_tot) {
  __shared__ double lane_excl[65];
  double vals[kSeedLane];
  prefix_of_block(closest, n, blockIdx.x, vals, lane_excl);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = lane_excl[64];
}

// block_excl[0..nb]: running sum (one thread; nb <= 2^21)
__global__ void k_seed_blockscan(const double* __restrict__ block_tot, int64_t nb,
                                 double* __restrict__ block_excl) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double run = 0.0;
  for (int64_t b = 0; b < nb; ++b) {
    block_excl[b] = run;
    run += block_tot[b];
  }
  block_excl[nb] = run;
}

// one wave per trial: target = draw * pot; candidate = the first row whose
// prefix reaches the target, n - 1 when none does
__global__ __launch_bounds__(64) void k_seed_search(const double* __restrict__ closest, int64_t n,
                                                    int64_t nb, const double* __restrict__ block_excl,
                                                    const double* __restrict__ draws,
                                                    const double* __restrict__ pot,
                                                    double* __restrict__ targets,
                                                    int64_t* __restrict__ cand) {
  __shared__ double lane_excl[65];
  __shared__ long long first[64];
  const int l = threadIdx.x, t = blockIdx.x;
  const double target = draws[t] * pot[0];
  long long fb = nb;
  for (int64_t b = l; b < nb; b += 64)
    if (block_excl[b + 1] >= target) {
      fb = b;
      break;
    }
  first[l] = fb;
  __syncthreads();
  if (l == 0) {
    long long m = nb;
    for (int q = 0; q < 64; ++q) m = first[q] < m ? first[q] : m;
    first[0] = m;
  }
  __syncthreads();
  const long long b = first[0];
  __syncthreads();
  if (b >= nb) {  // block-uniform
    if (l == 0) {
      targets[t] = target;
      cand[t] = n - 1;
    }
    return;
  }
  double vals[kSeedLane];
  prefix_of_block(closest, n, b, vals, lane_excl);
  const double base = block_excl[b];
  long long mine = n;  // none
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < kSeedLane; ++e) {
    s += vals[e];
    const long long i = b * kSeedBlock + (long long)l * kSeedLane + e;
    if (mine == n && i < n && base + (lane_excl[l] + s) >= target) mine = i;
  }
  first[l] = mine;
  __syncthreads();
  if (l == 0) {
    long long m = n;
    for (int q = 0; q < 64; ++q) m = first[q] < m ? first[q] : m;
    targets[t] = target;
    cand[t] = m < n ? m : n - 1;
  }
}

// out[t][i] = min(closest[i], |x_i - x_cand[t]|^2); closest == nullptr: the distance alone
__global__ __launch_bounds__(kClThreads) void k_seed_trials(
    const double* __restrict__ X, int64_t n, int d, int R, int trials, const double* __restrict__ cen,
    const double* __restrict__ scl, const int64_t* __restrict__ cand,
    const double* __restrict__ closest, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double sc[512];
  double* cx = lds;              // [trials][d]
  double* tile = lds + trials * d;
  stage_scaler(cen, scl, d, sc);
  __syncthreads();
  for (int i = threadIdx.x; i < trials * d; i += kClThreads) {
    const int t = i / d, f = i - t * d;
    cx[i] = scaled(X[cand[t] * d + f], cen ? sc : nullptr, sc + 256, f);
  }
  const int64_t t0 = (int64_t)blockIdx.x * R;
  const int rows = (int)(n - t0 < R ? n - t0 : R);
  stage_tile(X, t0, rows, d, sc, cen != nullptr, tile);
  __syncthreads();
  for (int it = threadIdx.x; it < rows * trials; it += kClThreads) {
    const int t = it / rows, r = it - t * rows;
    const double* x = tile + r * d;
    const double* c = cx + t * d;
    double a = 0.0;
    for (int f = 0; f < d; ++f) {
      const double u = x[f] - c[f];
      a += u * u;
    }
    if (closest) {
      const double o = closest[t0 + r];
      a = o < a ? o : a;
    }
    out[(int64_t)t * n + t0 + r] = a;
  }
}

// the trial with the smallest potential (the first of equals)
__global__ void k_seed_pick(const double* __restrict__ pots, int trials,
                            const int64_t* __restrict__ cand, const double* __restrict__ targets,
                            int step, double* __restrict__ pot, int* __restrict__ best_out,
                            int32_t* __restrict__ indices, double* __restrict__ trace, int tmax) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int best = 0;
  for (int t = 1; t < trials; ++t)
    if (pots[t] < pots[best]) best = t;
  pot[0] = pots[best];
  *best_out = best;
  indices[step] = (int32_t)cand[best];
  if (trace) {
    // per step: targets[tmax] | candidate rows[tmax] | potentials[tmax] | kept trial
    double* tr = trace + (int64_t)(step - 1) * (3 * tmax + 1);
    for (int t = 0; t < trials; ++t) {
      tr[t] = targets ? targets[t] : 0.0;
      tr[tmax + t] = (double)cand[t];
      tr[2 * tmax + t] = pots[t];
    }
    tr[3 * tmax] = (double)best;
  }
}

__global__ __launch_bounds__(kClThreads) void k_seed_keep(const double* __restrict__ trial_closest,
                                                          int64_t n, const int* __restrict__ best,
                                                          double* __restrict__ closest) {
  const int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x;
  if (i < n) closest[i] = trial_closest[(int64_t)best[0] * n + i];
}

// centres[j][f] = the scaled row indices[j]
__global__ void k_gather_rows(const double* __restrict__ X, int d, int k,
                              const double* __restrict__ cen, const double* __restrict__ scl,
                              const int32_t* __restrict__ indices, double* __restrict__ centres) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k * d) return;
  const int j = i / d, f = i - j * d;
  centres[i] = scaled(X[(int64_t)indices[j] * d + f], cen, scl, f);
}

// ---- launchers ---------------------------------------------------------------------

void cluster_census(const double* X, int64_t n, int d, unsigned long long* cnt, hipStream_t s) {
  TMH_HIP(hipMemsetAsync(cnt, 0, 2 * (size_t)d * sizeof(unsigned long long), s));
  const int64_t total = n * d;
  hipLaunchKernelGGL(k_census, dim3((unsigned)cdiv(total, 4096)), dim3(kClThreads), 0, s, X, total, d,
                     cnt);
  TMH_HIP(hipGetLastError());
}

int64_t cluster_colsum_chunks(int64_t n) { return cdiv(n, kColChunk); }

void cluster_colstat(const double* X, int64_t n, int d, const double* cen, const double* scl,
                     const unsigned long long* cnt, const double* mean, double* part, double* out,
                     hipStream_t s) {
  const int64_t chunks = cluster_colsum_chunks(n);
  hipLaunchKernelGGL(k_colsum, dim3((unsigned)chunks), dim3(kClThreads), 0, s, X, n, d, cen, scl, mean,
                     part);
  hipLaunchKernelGGL(k_colsum_final, dim3((unsigned)cdiv(d, 64)), dim3(64), 0, s, part, chunks, d, cnt,
                     out);
  TMH_HIP(hipGetLastError());
}

int64_t cluster_sum_chunks(int64_t n) { return cdiv(n, kSumChunk); }

void cluster_sum(const double* vec, int64_t n, int n_vec, double* part, double* out, hipStream_t s) {
  const int64_t chunks = cluster_sum_chunks(n);
  hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)chunks, (unsigned)n_vec), dim3(kClThreads), 0, s, vec,
                     n, chunks, part);
  hipLaunchKernelGGL(k_sum_final, dim3((unsigned)n_vec), dim3(kClThreads), 0, s, part, chunks, out);
  TMH_HIP(hipGetLastError());
}

void cluster_robust_scale(const double* X, int64_t n, int d, const double* cen, const double* scl,
                          double* out, hipStream_t s) {
  ProfScope prof("robust_scale", s);
  const int64_t total = n * d;
  hipLaunchKernelGGL(k_robust_scale, dim3((unsigned)cdiv(total, kClThreads)), dim3(kClThreads), 0, s, X,
                     total, d, cen, scl, out);
  TMH_HIP(hipGetLastError());
}

void cluster_select(const double* X, int64_t n, int d, int r, unsigned long long* state,
                    unsigned int* hist, double* out, hipStream_t s) {
  ProfScope prof("column_select", s);
  const int G = std::max(1, std::min(d, 128 / r));
  const int groups = (int)cdiv(d, G);
  const size_t lds = (size_t)G * r * 256 * sizeof(unsigned int);
  TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_select_hist),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // about 2,048 workgroups over rows x column groups; 2^20 rows per workgroup
  // at the most, so a 32-bit LDS counter cannot wrap
  int64_t rows_per_block = std::max<int64_t>(256, cdiv(n, std::max(1, 2048 / groups)));
  rows_per_block = std::min<int64_t>(rows_per_block, 1 << 20);
  const unsigned row_blocks = (unsigned)cdiv(n, rows_per_block);
  const int tabs = d * r;
  TMH_HIP(hipMemsetAsync(hist, 0, (size_t)tabs * 256 * sizeof(unsigned int), s));
  for (int pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(k_select_hist, dim3(row_blocks, (unsigned)groups), dim3(kClThreads), lds, s, X, n,
                       d, r, G, pass, rows_per_block, state, hist);
    hipLaunchKernelGGL(k_select_pick, dim3((unsigned)cdiv(tabs, 64)), dim3(64), 0, s, state, hist, tabs,
                       pass, out);
  }
  TMH_HIP(hipGetLastError());
}

static AssignGeom assign_geom(int64_t n, int d, int k, bool with_sums) {
  AssignGeom g;
  g.d = d;
  g.k = k;
  g.cs = (d & 1) ? d : d + 1;
  int R = std::min(256, std::max(1, kClTileDoubles / d));
  if (R > 1) R &= ~1;
  g.R = R;
  int T = 1;
  while (T < k && T < 64) T <<= 1;
  g.T = T;
  // what 160 KB of LDS leave for the slices' sums after the centres, the tile
  // and the small arrays
  const size_t fixed = ((size_t)k * g.cs + (size_t)R * d) * 8 + (size_t)R * 4 + (size_t)k * 4 + 4096 + 256;
  const size_t room = 160 * 1024 - fixed;
  int S = std::max(1, kClThreads / d);
  S = std::min<int64_t>(S, std::max<int64_t>(1, (int64_t)(room / ((size_t)k * d * 8))));
  g.S = with_sums ? S : 1;
  int64_t chunk = 1024;
  while (cdiv(n, chunk) > 2048) chunk *= 2;
  g.chunk = chunk;
  return g;
}

int64_t cluster_assign_chunks(int64_t n, int d, int k) { return cdiv(n, assign_geom(n, d, k, true).chunk); }

void cluster_assign(const double* X, int64_t n, int d, int k, const double* cen, const double* scl,
                    const double* centres, const int32_t* prev, int32_t* labels, double* mind,
                    int* changed, double* psums, unsigned int* pcounts, hipStream_t s) {
  ProfScope prof("kmeans_assign", s);
  const AssignGeom g = assign_geom(n, d, k, psums != nullptr);
  const size_t lds = ((size_t)k * g.cs + (size_t)g.R * d + (psums ? (size_t)g.S * k * d : 0)) * 8 +
                     (size_t)g.R * 4 + (size_t)k * 4;
  TMH_CHECK(lds + 4096 <= 160 * 1024, TMH_EINVAL, "k * d is over the limit of 8,192");
  TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_kmeans_assign),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (changed) TMH_HIP(hipMemsetAsync(changed, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_kmeans_assign, dim3((unsigned)cdiv(n, g.chunk)), dim3(kClThreads), lds, s, X, n,
                     g, cen, scl, centres, prev, labels, mind, changed, psums, pcounts);
  TMH_HIP(hipGetLastError());
}

void cluster_update(const double* X, int64_t n, int d, int k, const double* cen, const double* scl,
                    const int32_t* labels, const double* mind, const double* psums,
                    const unsigned int* pcounts, double* sums, long long* counts, const double* old,
                    double* centres_new, double* shift, int64_t* taken, hipStream_t s) {
  ProfScope prof("kmeans_update", s);
  const int64_t chunks = cluster_assign_chunks(n, d, k);
  hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)cdiv(k * d + k, 8)), dim3(kClThreads), 0, s,
                     psums, pcounts, chunks, k * d, k, sums, counts);
  hipLaunchKernelGGL(k_kmeans_finalize, dim3(1), dim3(1024), 0, s, X, n, d, k, cen, scl, labels, mind,
                     sums, counts, old, centres_new, shift, taken);
  TMH_HIP(hipGetLastError());
}

int64_t cluster_seed_blocks(int64_t n) { return cdiv(n, kSeedBlock); }

static int seed_tile_rows(int d) {
  int R = std::min(256, std::max(1, kClTileDoubles / d));
  if (R > 1) R &= ~1;
  return R;
}

void cluster_seed_trials(const double* X, int64_t n, int d, int trials, const double* cen,
                         const double* scl, const int64_t* cand, const double* closest, double* out,
                         hipStream_t s) {
  const int R = seed_tile_rows(d);
  const size_t lds = ((size_t)trials * d + (size_t)R * d) * 8;
  hipLaunchKernelGGL(k_seed_trials, dim3((unsigned)cdiv(n, R)), dim3(kClThreads), lds, s, X, n, d, R,
                     trials, cen, scl, cand, closest, out);
  TMH_HIP(hipGetLastError());
}

void cluster_seed_search(const double* closest, int64_t n, int trials, const double* draws,
                         const double* pot, double* block_tot, double* block_excl, double* targets,
                         int64_t* cand, hipStream_t s) {
  const int64_t nb = cluster_seed_blocks(n);
  hipLaunchKernelGGL(k_seed_blocksums, dim3((unsigned)nb), dim3(64), 0, s, closest, n, block_tot);
  hipLaunchKernelGGL(k_seed_blockscan, dim3(1), dim3(1), 0, s, block_tot, nb, block_excl);
  hipLaunchKernelGGL(k_seed_search, dim3((unsigned)trials), dim3(64), 0, s, closest, n, nb, block_excl,
                     draws, pot, targets, cand);
  TMH_HIP(hipGetLastError());
}

void cluster_seed_pick(const double* pots, int trials, const int64_t* cand, const double* targets,
                       int step, double* pot, int* best, int32_t* indices, double* trace, int tmax,
                       const double* trial_closest, int64_t n, double* closest, hipStream_t s) {
  hipLaunchKernelGGL(k_seed_pick, dim3(1), dim3(1), 0, s, pots, trials, cand, targets, step, pot, best,
                     indices, trace, tmax);
  hipLaunchKernelGGL(k_seed_keep, dim3((unsigned)cdiv(n, kClThreads)), dim3(kClThreads), 0, s,
                     trial_closest, n, best, closest);
  TMH_HIP(hipGetLastError());
}

void cluster_gather_rows(const double* X, int d, int k, const double* cen, const double* scl,
                         const int32_t* indices, double* centres, hipStream_t s) {
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)cdiv(k * d, 256)), dim3(256), 0, s, X, d, k, cen, scl,
                     indices, centres);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
