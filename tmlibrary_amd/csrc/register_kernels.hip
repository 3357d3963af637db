// Cross-cycle registration (the align step's chi2_shift): the circular
// cross-correlation of a target and a reference site by 2-D FFT, and its argmax.
//
//   C[dy, dx] = sum_{r,c} T[r, c] R[(r + dy) mod H, (c + dx) mod W]
//
// One pair costs two complex 2-D transforms: z = (T - mean T) + i (R - mean R)
// is transformed once, F(T) and F(R) are split from Z by Hermitian symmetry
// where conj(F(T)) F(R) is formed, and that product is transformed back.
// Three line passes over one complex plane Z[H][Mw] per pair (fft_core.h holds
// the line arithmetic; Mh, Mw = fft_line_length of H, W):
//   k_reg_rows_fwd  one row per workgroup: loads the u8/u16 rows of T and R,
//                   subtracts the means (exact integer sums, k_reg_sums), pads
//                   to Mw with zeros, transforms, writes Z[r][0..Mw).  Rows
//                   H..Mh of the padded plane are zero and never stored.
//   k_reg_cols      columns kx and Mw - kx together (the split needs Z[-ky][-kx]),
//                   c of each per workgroup: forward column transforms, the
//                   product, inverse column transforms, the fold of the y axis
//                   back to period H, all in LDS; rewrites the columns in place.
//   k_reg_rows_inv  one row per workgroup: inverse transform, real part, fold of
//                   the x axis, optional store of the f32 plane, and the row's
//                   argmax candidate.
// k_reg_argmax then reduces a pair's H candidates.  Ties go to the lowest flat
// lag dy W + dx in both reductions, so the result does not depend on the
// launch geometry.
#include <algorithm>
#include <vector>

#include "common.h"
#include "fft_core.h"

namespace tmh {
namespace {

constexpr int kRowThreads = 256;
// 16 waves on the one workgroup a CU holds: 7.9 ms for 64 full-size pairs against 9.7 with 512
constexpr int kColThreads = 1024;
constexpr int kSumParts = 64;
constexpr size_t kLdsBytes = 160 * 1024;           // per CU
constexpr size_t kChunkBytes = size_t(128) << 20;  // Z planes in flight: within the Infinity Cache

struct RegGeom {
  int H, W, Mh, Mw;
  FftPlan ph, pw;
};

struct RegResult {
  int32_t y, x;
  float peak;
  int32_t pad;
};

struct Cand {
  float v;
  int32_t idx;
};

__device__ inline bool cand_better(float v, int idx, float bv, int bi) {
  return v > bv || (v == bv && idx < bi);
}

// workgroup argmax with the tie rule; the result is valid in thread 0
template <int THREADS>
__device__ inline Cand block_argmax(float v, int idx, Cand* smem) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_down(v, o, 64);
    const int oi = __shfl_down(idx, o, 64);
    if (cand_better(ov, oi, v, idx)) {
      v = ov;
      idx = oi;
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) smem[wave] = Cand{v, idx};
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < THREADS / 64; ++w)
      if (cand_better(smem[w].v, smem[w].idx, v, idx)) {
        v = smem[w].v;
        idx = smem[w].idx;
      }
  }
  return Cand{v, idx};
}

// integer sum and sum of squares of every image: grid (kSumParts, images)
template <typename T>
__global__ __launch_bounds__(256) void k_reg_sums(const T* __restrict__ imgs, int64_t px,
                                                  unsigned long long* __restrict__ sums,
                                                  unsigned long long* __restrict__ squares) {
  const T* img = imgs + (int64_t)blockIdx.y * px;
  constexpr int kPer = 16 / sizeof(T);
  unsigned long long acc = 0, acc2 = 0;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  int64_t head = 0;
  if ((reinterpret_cast<uintptr_t>(img) & 15) == 0) {
    const int64_t nvec = px / kPer;
    const uint4* v = reinterpret_cast<const uint4*>(img);
    for (int64_t i = tid; i < nvec; i += nthr) {
      const uint4 q = v[i];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
      uint32_t s = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (sizeof(T) == 2) {
          const uint32_t lo = w[k] & 0xffffu, hi = w[k] >> 16;
          s += lo + hi;
          acc2 += (unsigned long long)(lo * lo) + (hi * hi);  // each below 2^32, their sum not
        } else {
          const uint32_t b0 = w[k] & 0xffu, b1 = (w[k] >> 8) & 0xffu, b2 = (w[k] >> 16) & 0xffu,
                         b3 = w[k] >> 24;
          s += b0 + b1 + b2 + b3;
          acc2 += b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3;
        }
      }
      acc += s;
    }
    head = nvec * kPer;
  }
  for (int64_t i = head + tid; i < px; i += nthr) {
    const uint32_t v = img[i];
    acc += v;
    acc2 += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_down(acc, o, 64);
    acc2 += __shfl_down(acc2, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && acc) {
    atomicAdd(&sums[blockIdx.y], acc);
    atomicAdd(&squares[blockIdx.y], acc2);
  }
}

// every pixel equals the mean: px * sum(v^2) == sum(v)^2, in 128 bits
__device__ inline bool reg_is_flat(unsigned long long sum, unsigned long long squares,
                                   unsigned long long px) {
  return squares * px == sum * sum && __umul64hi(squares, px) == __umul64hi(sum, sum);
}

// grid (H, pairs of the chunk); LDS 2 * Mw values
template <typename T>
__global__ __launch_bounds__(kRowThreads) void k_reg_rows_fwd(
    const T* __restrict__ targets, const T* __restrict__ refs, const int32_t* __restrict__ ref_of,
    int64_t first_pair, int64_t n_targets, RegGeom g, const unsigned long long* __restrict__ sums,
    const unsigned long long* __restrict__ squares, const cf* __restrict__ tw_w,
    cf* __restrict__ Z) {
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  cf* src = lds;
  cf* dst = lds + g.Mw;
  const int tid = threadIdx.x, r = blockIdx.x;
  const int64_t pair = first_pair + blockIdx.y;
  const int64_t ri = ref_of[pair];
  const double px = (double)g.H * (double)g.W;
  const double mt = (double)sums[pair] / px, mr = (double)sums[n_targets + ri] / px;
  const T* trow = targets + (pair * g.H + r) * g.W;
  const T* rrow = refs + (ri * g.H + r) * g.W;
  // A constant image correlates to exactly zero with anything, but the split of
  // F(T) and F(R) from one transform is exact only up to rounding: the other
  // image would leak into the flat one's spectrum and the argmax would be noise.
  const unsigned long long npx = (unsigned long long)g.H * (unsigned long long)g.W;
  const bool flat = reg_is_flat(sums[pair], squares[pair], npx) ||
                    reg_is_flat(sums[n_targets + ri], squares[n_targets + ri], npx);
  for (int c = tid; c < g.Mw; c += kRowThreads)
    src[c] = c < g.W && !flat ? cf{(float)((double)trow[c] - mt), (float)((double)rrow[c] - mr)}
                              : cf{0.f, 0.f};
  __syncthreads();
  int Ns = 1;
  for (int p = 0; p < g.pw.npass; ++p) {
    fft_pass(src, dst, g.Mw, Ns, g.pw.radix[p], 1, g.Mw, tw_w, false, tid, kRowThreads);
    __syncthreads();
    Ns *= g.pw.radix[p];
    cf* t = src;
    src = dst;
    dst = t;
  }
  cf* out = Z + ((int64_t)blockIdx.y * g.H + r) * g.Mw;
  for (int c = tid; c < g.Mw; c += kRowThreads) out[c] = src[c];
}

// grid (column groups, pairs of the chunk); LDS 2 buffers of 2 c lines of
// `stride` values (stride is odd, so the lines start on different banks)
__global__ __launch_bounds__(kColThreads) void k_reg_cols(RegGeom g, int c, int stride,
                                                          const cf* __restrict__ tw_h,
                                                          cf* __restrict__ Z) {
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  const int ncol = 2 * c, tid = threadIdx.x;
  cf* src = lds;
  cf* dst = lds + ncol * stride;
  // consecutive workgroups go to different XCDs: give each XCD a contiguous
  // run of column groups, so that neighbours share their 128-byte lines in one L2
  const int nb = gridDim.x, bid = blockIdx.x, q = nb / 8, rem = nb % 8, xcd = bid % 8;
  const int grp = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + bid / 8;
  const int k0 = grp * c, half = g.Mw / 2;
  cf* Zp = Z + (int64_t)blockIdx.y * g.H * g.Mw;

  // slot s < c: column k0 + s; slot c + s: its mirror (Mw - column) mod Mw
  for (int i = tid; i < g.Mh * ncol; i += kColThreads) {
    const int row = i / ncol, s = i - row * ncol;
    const int kx = k0 + (s < c ? s : s - c);
    const int col = s < c ? kx : (g.Mw - kx) % g.Mw;
    src[s * stride + row] =
        (row < g.H && kx <= half) ? Zp[(int64_t)row * g.Mw + col] : cf{0.f, 0.f};
  }
  __syncthreads();
  int Ns = 1;
  for (int p = 0; p < g.ph.npass; ++p) {
    fft_pass(src, dst, g.Mh, Ns, g.ph.radix[p], ncol, stride, tw_h, false, tid, kColThreads);
    __syncthreads();
    Ns *= g.ph.radix[p];
    cf* t = src;
    src = dst;
    dst = t;
  }
  // with a = Z[ky][kx] and b = conj(Z[-ky][-kx]): a + b = 2 F(T), -i (a - b) = 2 F(R)
  const float scale = 0.25f / ((float)g.Mh * (float)g.Mw);
  for (int i = tid; i < g.Mh * ncol; i += kColThreads) {
    const int s = i / g.Mh, ky = i - s * g.Mh;
    const int sp = s < c ? s + c : s - c;
    const cf a = src[s * stride + ky];
    const cf b = cf_conj(src[sp * stride + (ky ? g.Mh - ky : 0)]);
    const cf prod = cf_mul(cf_conj(cf_add(a, b)), cf_rot(cf_sub(a, b), false));
    dst[s * stride + ky] = cf{prod.x * scale, prod.y * scale};
  }
  __syncthreads();
  {
    cf* t = src;
    src = dst;
    dst = t;
  }
  Ns = 1;
  for (int p = 0; p < g.ph.npass; ++p) {
    fft_pass(src, dst, g.Mh, Ns, g.ph.radix[p], ncol, stride, tw_h, true, tid, kColThreads);
    __syncthreads();
    Ns *= g.ph.radix[p];
    cf* t = src;
    src = dst;
    dst = t;
  }
  for (int i = tid; i < g.H * ncol; i += kColThreads) {
    const int row = i / ncol, s = i - row * ncol;
    const int kx = k0 + (s < c ? s : s - c);
    const int col = s < c ? kx : (g.Mw - kx) % g.Mw;
    if (kx > half || (s >= c && col == kx)) continue;  // no such column / the column of slot s - c
    cf v = src[s * stride + row];
    const int f = fft_fold_index(row, g.H, g.Mh);
    if (f >= 0) v = cf_add(v, src[s * stride + f]);
    Zp[(int64_t)row * g.Mw + col] = v;
  }
}

// grid (H, pairs of the chunk); LDS 2 * Mw values
__global__ __launch_bounds__(kRowThreads) void k_reg_rows_inv(RegGeom g, const cf* __restrict__ tw_w,
                                                              const cf* __restrict__ Z,
                                                              float* __restrict__ plane,
                                                              Cand* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) cf lds[];
  __shared__ Cand red[kRowThreads / 64];
  cf* src = lds;
  cf* dst = lds + g.Mw;
  const int tid = threadIdx.x, dy = blockIdx.x;
  const int64_t line = (int64_t)blockIdx.y * g.H + dy;
  const cf* in = Z + line * g.Mw;
  for (int c = tid; c < g.Mw; c += kRowThreads) src[c] = in[c];
  __syncthreads();
  int Ns = 1;
  for (int p = 0; p < g.pw.npass; ++p) {
    fft_pass(src, dst, g.Mw, Ns, g.pw.radix[p], 1, g.Mw, tw_w, true, tid, kRowThreads);
    __syncthreads();
    Ns *= g.pw.radix[p];
    cf* t = src;
    src = dst;
    dst = t;
  }
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int dx = tid; dx < g.W; dx += kRowThreads) {
    float v = src[dx].x;
    const int f = fft_fold_index(dx, g.W, g.Mw);
    if (f >= 0) v += src[f].x;
    if (plane) plane[line * g.W + dx] = v;
    if (cand_better(v, dx, bv, bi)) {
      bv = v;
      bi = dx;
    }
  }
  const Cand best = block_argmax<kRowThreads>(bv, bi, red);
  if (tid == 0) cand[line] = best;
}

// grid (pairs of the chunk)
__global__ __launch_bounds__(256) void k_reg_argmax(RegGeom g, const Cand* __restrict__ cand,
                                                    RegResult* __restrict__ res) {
  __shared__ Cand red[256 / 64];
  const Cand* cp = cand + (int64_t)blockIdx.x * g.H;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int dy = threadIdx.x; dy < g.H; dy += 256) {
    const Cand q = cp[dy];
    const int idx = dy * g.W + q.idx;
    if (cand_better(q.v, idx, bv, bi)) {
      bv = q.v;
      bi = idx;
    }
  }
  const Cand best = block_argmax<256>(bv, bi, red);
  if (threadIdx.x == 0) {
    const int dy = best.idx / g.W, dx = best.idx - dy * g.W;
    res[blockIdx.x] = RegResult{dy <= g.H / 2 ? dy : dy - g.H, dx <= g.W / 2 ? dx : dx - g.W,
                                best.v, 0};
  }
}

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// the caller's scratch, carved up
struct RegScratch {
  size_t tw_h, tw_w, sums, ref_of, cand, res, z, total;
  int64_t chunk;  // pairs per launch
};

RegGeom reg_geom(int H, int W) {
  TMH_CHECK(H >= 1 && W >= 1, TMH_EINVAL, "height and width must be at least 1");
  TMH_CHECK(H <= kFftMaxLine && W <= kFftMaxLine, TMH_EINVAL,
            "an image side is over the limit of 4096 values");
  RegGeom g;
  g.H = H;
  g.W = W;
  g.Mh = fft_line_length(H);
  g.Mw = fft_line_length(W);
  TMH_CHECK(g.Mh <= kFftMaxLine && g.Mw <= kFftMaxLine, TMH_EINVAL,
            "a transformed line is over the limit of 4096 values: an axis must be 5-smooth "
            "and <= 4096, or <= 2048 when it is padded to 2 L - 1");
  fft_make_plan(g.Mh, &g.ph);
  fft_make_plan(g.Mw, &g.pw);
  return g;
}

RegScratch reg_scratch(const RegGeom& g, int64_t n, int64_t m) {
  RegScratch L;
  const size_t pair_bytes = (size_t)g.H * g.Mw * sizeof(cf);
  L.chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n, 32768),
                                                   (int64_t)(kChunkBytes / pair_bytes)));
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += align256(bytes);
    return o;
  };
  L.tw_h = take((size_t)g.Mh * sizeof(cf));
  L.tw_w = take((size_t)g.Mw * sizeof(cf));
  L.sums = take(2 * (size_t)(n + m) * sizeof(unsigned long long));  // sums, then sums of squares
  L.ref_of = take((size_t)n * sizeof(int32_t));
  L.cand = take((size_t)L.chunk * g.H * sizeof(Cand));
  L.res = take((size_t)n * sizeof(RegResult));
  L.z = take((size_t)L.chunk * pair_bytes);
  L.total = at;
  return L;
}

template <typename T>
void reg_run(const T* targets, int64_t n, const T* refs, int64_t m, const RegGeom& g,
             const RegScratch& L, uint8_t* scratch, float* dev_plane, hipStream_t s) {
  const cf* tw_h = reinterpret_cast<const cf*>(scratch + L.tw_h);
  const cf* tw_w = reinterpret_cast<const cf*>(scratch + L.tw_w);
  auto* sums = reinterpret_cast<unsigned long long*>(scratch + L.sums);
  unsigned long long* squares = sums + n + m;
  const int32_t* ref_of = reinterpret_cast<const int32_t*>(scratch + L.ref_of);
  Cand* cand = reinterpret_cast<Cand*>(scratch + L.cand);
  RegResult* res = reinterpret_cast<RegResult*>(scratch + L.res);
  cf* Z = reinterpret_cast<cf*>(scratch + L.z);
  const int64_t px = (int64_t)g.H * g.W;

  TMH_HIP(hipMemsetAsync(sums, 0, 2 * (size_t)(n + m) * sizeof(unsigned long long), s));
  {
    ProfScope prof("reg_sums", s);
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(kSumParts, px / 4096));
    for (int64_t at = 0; at < n; at += 32768)
      hipLaunchKernelGGL(k_reg_sums<T>, dim3(parts, (unsigned)std::min<int64_t>(32768, n - at)),
                         dim3(256), 0, s, targets + at * px, px, sums + at, squares + at);
    for (int64_t at = 0; at < m; at += 32768)
      hipLaunchKernelGGL(k_reg_sums<T>, dim3(parts, (unsigned)std::min<int64_t>(32768, m - at)),
                         dim3(256), 0, s, refs + at * px, px, sums + n + at, squares + n + at);
    TMH_HIP(hipGetLastError());
  }
  const size_t row_lds = 2 * (size_t)g.Mw * sizeof(cf);
  const int stride = g.Mh | 1;
  const int half_cols = g.Mw / 2 + 1;
  int c = (int)(kLdsBytes / (4 * (size_t)stride * sizeof(cf)));
  c = std::max(1, std::min(std::min(c, 8), half_cols));
  const size_t col_lds = 4 * (size_t)c * stride * sizeof(cf);
  TMH_CHECK(col_lds <= kLdsBytes, TMH_EINVAL, "a transformed line is over the limit of 4096 values");
  const int groups = (half_cols + c - 1) / c;
  TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_reg_cols),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)col_lds));
  TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_reg_rows_fwd<T>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)row_lds));
  TMH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_reg_rows_inv),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)row_lds));
  for (int64_t first = 0; first < n; first += L.chunk) {
    const unsigned pairs = (unsigned)std::min<int64_t>(L.chunk, n - first);
    {
      ProfScope prof("reg_rows_fwd", s);
      hipLaunchKernelGGL(k_reg_rows_fwd<T>, dim3(g.H, pairs), dim3(kRowThreads), row_lds, s,
                         targets, refs, ref_of, first, n, g, sums, squares, tw_w, Z);
      TMH_HIP(hipGetLastError());
    }
    {
      ProfScope prof("reg_cols", s);
      hipLaunchKernelGGL(k_reg_cols, dim3(groups, pairs), dim3(kColThreads), col_lds, s, g, c,
                         stride, tw_h, Z);
      TMH_HIP(hipGetLastError());
    }
    {
      ProfScope prof("reg_rows_inv", s);
      hipLaunchKernelGGL(k_reg_rows_inv, dim3(g.H, pairs), dim3(kRowThreads), row_lds, s, g, tw_w,
                         Z, dev_plane ? dev_plane + first * px : nullptr, cand);
      TMH_HIP(hipGetLastError());
    }
    {
      ProfScope prof("reg_argmax", s);
      hipLaunchKernelGGL(k_reg_argmax, dim3(pairs), dim3(256), 0, s, g, cand, res + first);
      TMH_HIP(hipGetLastError());
    }
  }
}

}  // namespace

int64_t register_scratch_bytes(int64_t n, int64_t m, int H, int W) {
  const RegGeom g = reg_geom(H, W);
  return (int64_t)reg_scratch(g, n, m).total;
}

void launch_register(const void* dev_targets, int64_t n, const void* dev_refs, int64_t m, int H,
                     int W, int elem_bytes, const int32_t* host_ref_of, void* dev_scratch,
                     int64_t scratch_bytes, int32_t* host_y, int32_t* host_x, float* host_peak,
                     float* dev_plane, hipStream_t s) {
  const RegGeom g = reg_geom(H, W);
  const RegScratch L = reg_scratch(g, n, m);
  TMH_CHECK(scratch_bytes >= (int64_t)L.total, TMH_EINVAL,
            "scratch is smaller than tmh_register_scratch_bytes");
  for (int64_t i = 0; i < n; ++i)
    TMH_CHECK(host_ref_of[i] >= 0 && host_ref_of[i] < m, TMH_EINVAL,
              "ref_of_target holds an index outside the references");
  uint8_t* scratch = static_cast<uint8_t*>(dev_scratch);
  std::vector<cf> tw_h(g.Mh), tw_w(g.Mw);
  fft_twiddles_host(g.Mh, tw_h.data());
  fft_twiddles_host(g.Mw, tw_w.data());
  TMH_HIP(hipMemcpyAsync(scratch + L.tw_h, tw_h.data(), tw_h.size() * sizeof(cf),
                         hipMemcpyHostToDevice, s));
  TMH_HIP(hipMemcpyAsync(scratch + L.tw_w, tw_w.data(), tw_w.size() * sizeof(cf),
                         hipMemcpyHostToDevice, s));
  TMH_HIP(hipMemcpyAsync(scratch + L.ref_of, host_ref_of, (size_t)n * sizeof(int32_t),
                         hipMemcpyHostToDevice, s));
  if (elem_bytes == 2)
    reg_run(static_cast<const uint16_t*>(dev_targets), n, static_cast<const uint16_t*>(dev_refs),
            m, g, L, scratch, dev_plane, s);
  else
    reg_run(static_cast<const uint8_t*>(dev_targets), n, static_cast<const uint8_t*>(dev_refs), m,
            g, L, scratch, dev_plane, s);
  std::vector<RegResult> res((size_t)n);
  TMH_HIP(hipMemcpyAsync(res.data(), scratch + L.res, res.size() * sizeof(RegResult),
                         hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));  // the results are on the host; the tables may go
  for (int64_t i = 0; i < n; ++i) {
    if (host_y) host_y[i] = res[i].y;
    if (host_x) host_x[i] = res[i].x;
    if (host_peak) host_peak[i] = res[i].peak;
  }
}

}  // namespace tmh
