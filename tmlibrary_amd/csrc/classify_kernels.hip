// The supervised classification tool (gfx950 / MI355X): random-forest and SVC
// prediction on row-major f64 feature tables from flat models.
//
// Reference: tmlib/tools/classification.py:45-116 through Classifier.predict
// (tmlib/tools/base.py:621-645), where scikit-learn's
// RandomForestClassifier.predict and SVC.predict label every object on the
// host.  The row rules are in classify_core.h, which tests/classify_host.cpp
// compiles for the host, and are restated in tests/classification_literal.py.
//
// Forest.  A workgroup owns a chunk of rows and walks it in tiles: the tile is
// read with coalesced loads and lands in LDS as f32; thread (row, tree) walks
// one tree and leaves the leaf row in LDS; thread (row, class) adds the trees'
// fractions in tree order and divides; thread (row) takes the first maximum.
// The packed nodes (16 bytes each) are staged into LDS once per workgroup when
// they fit kForestLdsBytes, and read from memory otherwise; the two routes run
// the same code on the same values.
//
// SVC.  A workgroup owns a chunk of rows and walks it in tiles of R rows; the
// support vectors stream through LDS in tiles of Ms.  Both tiles are stored
// feature-major, so a thread that owns (one SV, four rows) reads its SV's
// value without a bank conflict and the four rows' values as two broadcast
// 16-byte reads.  Per SV tile: K[row][sv] into LDS, then thread (row, pair)
// continues its decision value over the tile's SVs in ascending order.  The
// sums are the same sequence of fused multiply-adds whatever the tile size, so
// every tile size gives the same bytes.  A linear model arrives collapsed to
// one weight vector per pair and runs the same kernel with dec = x . w.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "table_load.h"

#include "classify_core.h"

namespace tmh {

constexpr int kCfThreads = 256;
// The forest's LDS route: one staged copy of the nodes serves 16 waves, and a
// workgroup keeps it for four times the rows.  (At 256 threads the staged
// forest left a CU four waves, and the memory route beat it: DESIGN 23.4.)
constexpr int kForestLdsThreads = 1024;
constexpr int kForestLdsChunks = 4;

// ---- refused input ---------------------------------------------------------------
// cnt[0] += finite values whose f32 cast is infinite; a grid-stride loop, so
// the grid does not grow with the table
__global__ __launch_bounds__(kCfThreads) void k_count_f32_overflow(
    const double* __restrict__ X, int64_t total, unsigned long long* __restrict__ cnt) {
  const int64_t step = (int64_t)gridDim.x * kCfThreads;
  unsigned int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * kCfThreads + threadIdx.x; i < total; i += step)
    mine += f32_cast_overflows(X[i]) ? 1u : 0u;
  if (mine) atomicAdd(cnt, (unsigned long long)mine);
}

// ---- forest ----------------------------------------------------------------------
struct ForestGeom {
  int d, ds;          // features, stride of a tile row in floats (odd)
  int C, T, nodes;    // classes, trees, packed nodes
  int R;              // tile rows
  int tile_bytes;     // the tile: f32 [R][ds], then reused as f64 [R][C]
  int64_t chunk;      // rows per workgroup
};

// LDS: nodes[nodes] (the LDS route) | tile | leaf[R][T] | root[T]
template <bool kLdsNodes>
__global__ __launch_bounds__(kLdsNodes ? kForestLdsThreads : kCfThreads) void k_forest_predict(
    const double* __restrict__ X, int64_t n, ForestGeom g, const ForestNode* __restrict__ nodes,
    const int32_t* __restrict__ roots, const double* __restrict__ leaf_value,
    int32_t* __restrict__ labels, double* __restrict__ proba) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int d = g.d, ds = g.ds, C = g.C, T = g.T, R = g.R;
  const int tid = threadIdx.x;
  constexpr int kThreads = kLdsNodes ? kForestLdsThreads : kCfThreads;
  ForestNode* lnodes = reinterpret_cast<ForestNode*>(lds_raw);
  unsigned char* after = lds_raw + (kLdsNodes ? (size_t)g.nodes * sizeof(ForestNode) : 0);
  float* tile = reinterpret_cast<float*>(after);
  double* prob = reinterpret_cast<double*>(after);
  int32_t* leaf = reinterpret_cast<int32_t*>(after + g.tile_bytes);
  int32_t* root = leaf + R * T;
  if (kLdsNodes) {
    // 16-byte copies of the 16-byte nodes
    const double2* src = reinterpret_cast<const double2*>(nodes);
    double2* dst = reinterpret_cast<double2*>(lnodes);
    for (int i = tid; i < g.nodes; i += kThreads) dst[i] = src[i];
  }
  for (int t = tid; t < T; t += kThreads) root[t] = roots[t];
  const int64_t c0 = (int64_t)blockIdx.x * g.chunk;
  const int64_t c1 = c0 + g.chunk < n ? c0 + g.chunk : n;
  for (int64_t t0 = c0; t0 < c1; t0 += R) {
    const int rows = (int)(c1 - t0 < R ? c1 - t0 : R);
    __syncthreads();  // the nodes and roots are staged; the last tile's prob is read
    {
      const double* src = X + t0 * d;
      const int cnt = rows * d;
      if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        for (int i = tid; i < (cnt >> 1); i += kThreads) {
          const double2 v = reinterpret_cast<const double2*>(src)[i];
          const int r0 = (2 * i) / d, f0 = 2 * i - r0 * d;
          const int r1 = f0 + 1 == d ? r0 + 1 : r0, f1 = f0 + 1 == d ? 0 : f0 + 1;
          tile[r0 * ds + f0] = (float)v.x;
          tile[r1 * ds + f1] = (float)v.y;
        }
        if ((cnt & 1) && tid == 0) tile[(rows - 1) * ds + d - 1] = (float)src[cnt - 1];
      } else {
        for (int i = tid; i < cnt; i += kThreads) tile[(i / d) * ds + i % d] = (float)src[i];
      }
    }
    __syncthreads();
    for (int it = tid; it < rows * T; it += kThreads) {
      const int t = it / rows, r = it - t * rows;
      leaf[r * T + t] = forest_leaf(kLdsNodes ? lnodes : nodes, root[t], tile + r * ds);
    }
    __syncthreads();  // the tile is read; prob takes its place
    for (int it = tid; it < rows * C; it += kThreads) {
      const int r = it / C, c = it - r * C;
      const double p = forest_class_proba(leaf_value, leaf + r * T, T, C, c);
      prob[it] = p;
      if (proba) proba[t0 * C + it] = p;
    }
    __syncthreads();
    for (int r = tid; r < rows; r += kThreads) labels[t0 + r] = first_max(prob + r * C, C);
  }
}

// ---- SVC ---------------------------------------------------------------------------
struct SvcGeom {
  int d, k, P, kernel;
  int m;            // rows of `sv`: support vectors (rbf) or the pairs' weight vectors (linear)
  int R, xs;        // tile rows (a multiple of 4), stride of a feature's row values (even)
  int Ms, cs;       // SVs per tile, stride of a coefficient row in the tile (odd)
  int64_t chunk;    // rows per workgroup
  double gamma;
};

// LDS: xt[d][xs] | svt[d][Ms] | Kb[R][Ms] | dec[R][P] | ct[k - 1][cs] | rho[P] | start[k + 1]
template <int kKernel>
__global__ __launch_bounds__(kCfThreads) void k_svc_predict(
    const double* __restrict__ X, int64_t n, SvcGeom g, const double* __restrict__ cen,
    const double* __restrict__ scl, const double* __restrict__ sv, const double* __restrict__ coef,
    const int32_t* __restrict__ start_g, const double* __restrict__ rho_g,
    int32_t* __restrict__ labels, double* __restrict__ dec_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double sc[512];
  const int d = g.d, k = g.k, P = g.P, m = g.m, R = g.R, xs = g.xs, Ms = g.Ms, cs = g.cs;
  const int tid = threadIdx.x;
  double* xt = lds;
  double* svt = xt + d * xs;
  double* Kb = svt + d * Ms;
  double* dec = Kb + R * Ms;
  double* ct = dec + R * P;
  double* rho = ct + (k - 1) * cs;
  int32_t* start = reinterpret_cast<int32_t*>(rho + P);
  stage_scaler(cen, scl, d, sc);
  for (int p = tid; p < P; p += kCfThreads) rho[p] = rho_g[p];
  if (kKernel == kSvcRbf)
    for (int c = tid; c <= k; c += kCfThreads) start[c] = start_g[c];
  const double* c_sc = cen ? sc : nullptr;
  const int64_t c0 = (int64_t)blockIdx.x * g.chunk;
  const int64_t c1 = c0 + g.chunk < n ? c0 + g.chunk : n;
  const int RB = R >> 2;  // blocks of four rows
  for (int64_t t0 = c0; t0 < c1; t0 += R) {
    const int rows = (int)(c1 - t0 < R ? c1 - t0 : R);
    __syncthreads();  // the scaler is staged; the last tile's dec is read
    {
      const double* src = X + t0 * d;
      const int cnt = rows * d;
      for (int i = tid; i < cnt; i += kCfThreads) {
        const int r = i / d, f = i - r * d;
        xt[f * xs + r] = scaled(src[i], c_sc, sc + 256, f);
      }
      // rows past the table's end: zeros, computed and never written out
      for (int i = cnt + tid; i < R * d; i += kCfThreads) {
        const int r = i / d, f = i - r * d;
        xt[f * xs + r] = 0.0;
      }
      for (int i = tid; i < R * P; i += kCfThreads) dec[i] = 0.0;
    }
    for (int s0 = 0; s0 < m; s0 += Ms) {
      const int ns = m - s0 < Ms ? m - s0 : Ms;
      __syncthreads();  // xt and dec are written; the last SV tile is read
      for (int i = tid; i < ns * d; i += kCfThreads) {
        const int s = i / d, f = i - s * d;
        svt[f * Ms + s] = sv[(int64_t)s0 * d + i];
      }
      if (kKernel == kSvcRbf)
        for (int i = tid; i < (k - 1) * ns; i += kCfThreads) {
          const int row = i / ns, s = i - row * ns;
          ct[row * cs + s] = coef[(int64_t)row * m + s0 + s];
        }
      __syncthreads();
      for (int it = tid; it < ns * RB; it += kCfThreads) {
        const int rb = it / ns, s = it - rb * ns;
        const double* xp = xt + 4 * rb;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int f = 0; f < d; ++f) {
          const double v = svt[f * Ms + s];
          const double2 x01 = *reinterpret_cast<const double2*>(xp + f * xs);
          const double2 x23 = *reinterpret_cast<const double2*>(xp + f * xs + 2);
          if (kKernel == kSvcRbf) {
            const double u0 = x01.x - v, u1 = x01.y - v, u2 = x23.x - v, u3 = x23.y - v;
            a0 = fma(u0, u0, a0);
            a1 = fma(u1, u1, a1);
            a2 = fma(u2, u2, a2);
            a3 = fma(u3, u3, a3);
          } else {
            a0 = fma(x01.x, v, a0);
            a1 = fma(x01.y, v, a1);
            a2 = fma(x23.x, v, a2);
            a3 = fma(x23.y, v, a3);
          }
        }
        if (kKernel == kSvcRbf) {
          a0 = exp(-g.gamma * a0);
          a1 = exp(-g.gamma * a1);
          a2 = exp(-g.gamma * a2);
          a3 = exp(-g.gamma * a3);
        }
        double* kp = Kb + (4 * rb) * Ms + s;
        kp[0] = a0;
        kp[Ms] = a1;
        kp[2 * Ms] = a2;
        kp[3 * Ms] = a3;
      }
      __syncthreads();
      if (kKernel == kSvcRbf) {
        for (int it = tid; it < rows * P; it += kCfThreads) {
          const int r = it / P, p = it - r * P;
          // the pair (i, j) of index p
          int i = 0, left = p;
          while (left >= k - 1 - i) {
            left -= k - 1 - i;
            ++i;
          }
          const int j = i + 1 + left;
          dec[it] = svc_pair_accumulate(dec[it], ct, cs, Kb + r * Ms, s0, s0 + ns, start, i, j);
        }
      } else {
        for (int it = tid; it < rows * ns; it += kCfThreads) {
          const int r = it / ns, s = it - r * ns;
          dec[r * P + s0 + s] = Kb[r * Ms + s];
        }
      }
    }
    __syncthreads();
    for (int it = tid; it < rows * P; it += kCfThreads) {
      const double v = dec[it] - rho[it % P];
      dec[it] = v;
      if (dec_out) dec_out[t0 * P + it] = v;
    }
    __syncthreads();
    for (int r = tid; r < rows; r += kCfThreads) labels[t0 + r] = svc_vote(dec + r * P, 1, k);
  }
}

// ---- launchers -----------------------------------------------------------------------

void classify_count_f32_overflow(const double* X, int64_t n, int d, unsigned long long* cnt,
                                 hipStream_t s) {
  TMH_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
  const int64_t total = n * d;
  const int64_t blocks = std::min<int64_t>(cdiv(total, kCfThreads), 8192);
  hipLaunchKernelGGL(k_count_f32_overflow, dim3((unsigned)blocks), dim3(kCfThreads), 0, s, X, total,
                     cnt);
  TMH_HIP(hipGetLastError());
}

static int64_t row_chunk(int64_t n) {
  int64_t chunk = 1024;
  while (cdiv(n, chunk) > 2048) chunk *= 2;
  return chunk;
}

bool forest_fits_lds(int64_t nodes) { return nodes * (int64_t)sizeof(ForestNode) <= kForestLdsBytes; }

int forest_tile_rows(int d, int n_classes, int n_trees) {
  const int ds = d | 1;
  // f32 tile and f64 probabilities within 32 KB, leaf rows within 16 KB
  return std::max(1, std::min({256, 8192 / ds, 4096 / n_classes, 4096 / n_trees}));
}

void forest_predict(const double* X, int64_t n, int d, int n_classes, int n_trees, int nodes,
                    bool lds_route, const ForestNode* dev_nodes, const int32_t* dev_roots,
                    const double* dev_leaf_value, int32_t* labels, double* proba, hipStream_t s) {
  ProfScope prof(lds_route ? "forest_predict_lds" : "forest_predict_mem", s);
  ForestGeom g;
  g.d = d;
  g.ds = d | 1;
  g.C = n_classes;
  g.T = n_trees;
  g.nodes = nodes;
  g.R = forest_tile_rows(d, n_classes, n_trees);
  g.tile_bytes = (std::max(g.R * g.ds * 4, g.R * g.C * 8) + 15) & ~15;
  g.chunk = row_chunk(n) * (lds_route ? kForestLdsChunks : 1);
  const size_t lds = (lds_route ? (size_t)nodes * sizeof(ForestNode) : 0) + (size_t)g.tile_bytes +
                     ((size_t)g.R * g.T + (size_t)g.T) * 4;
  TMH_CHECK(lds + 1024 <= 160 * 1024, TMH_EINVAL, "the forest does not fit the LDS route");
  const dim3 grid((unsigned)cdiv(n, g.chunk));
  if (lds_route) {
    TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_forest_predict<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_forest_predict<true>, grid, dim3(kForestLdsThreads), lds, s, X, n, g, dev_nodes,
                       dev_roots, dev_leaf_value, labels, proba);
  } else {
    TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_forest_predict<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_forest_predict<false>, grid, dim3(kCfThreads), lds, s, X, n, g, dev_nodes,
                       dev_roots, dev_leaf_value, labels, proba);
  }
  TMH_HIP(hipGetLastError());
}

// the SV tile of a model: what LDS holds beside the row tile, capped by `cap` (0: none)
static SvcGeom svc_geom(int64_t n, int d, int k, int kernel, int m, double gamma, int cap) {
  SvcGeom g;
  g.d = d;
  g.k = k;
  g.P = k * (k - 1) / 2;
  g.kernel = kernel;
  g.m = m;
  g.gamma = gamma;
  int R = std::min({256, 4096 / d, 2048 / g.P});
  R = std::max(4, R & ~3);
  g.R = R;
  g.xs = R + 2;
  int Ms = std::min({m, 256, 4096 / d, 4096 / R});
  if (cap > 0) Ms = std::min(Ms, cap);
  g.Ms = std::max(1, Ms);
  g.cs = g.Ms | 1;
  g.chunk = row_chunk(n);
  return g;
}

int svc_tile_svs(int d, int k, int kernel, int m, int cap) {
  return svc_geom(1, d, k, kernel, m, 0.0, cap).Ms;
}

void svc_predict(const double* X, int64_t n, int d, int k, int kernel, double gamma, int m,
                 int tile_cap, const double* cen, const double* scl, const double* dev_sv,
                 const double* dev_coef, const int32_t* dev_start, const double* dev_rho,
                 int32_t* labels, double* dec, hipStream_t s) {
  ProfScope prof("svc_predict", s);
  const SvcGeom g = svc_geom(n, d, k, kernel, m, gamma, tile_cap);
  const size_t lds = ((size_t)d * g.xs + (size_t)d * g.Ms + (size_t)g.R * g.Ms + (size_t)g.R * g.P +
                      (size_t)(k - 1) * g.cs + (size_t)g.P) * 8 + ((size_t)k + 1) * 4;
  TMH_CHECK(lds + 4096 + 1024 <= 160 * 1024, TMH_EINVAL, "the SVC tiles do not fit LDS");
  const dim3 grid((unsigned)cdiv(n, g.chunk));
  if (kernel == kSvcRbf) {
    TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_svc_predict<kSvcRbf>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_svc_predict<kSvcRbf>, grid, dim3(kCfThreads), lds, s, X, n, g, cen, scl,
                       dev_sv, dev_coef, dev_start, dev_rho, labels, dec);
  } else {
    TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_svc_predict<kSvcLinear>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_svc_predict<kSvcLinear>, grid, dim3(kCfThreads), lds, s, X, n, g, cen, scl,
                       dev_sv, dev_coef, dev_start, dev_rho, labels, dec);
  }
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
