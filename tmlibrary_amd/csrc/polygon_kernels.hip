// jterator object input (gfx950 / MI355X): label planes from stored outlines,
// what SegmentationImage.create_from_polygons (tmlib/image.py:740-776) draws
// with skimage.draw.polygon per (label, ring) of a plane's list, later rings
// over earlier ones.  The per-ring rule is in polygon_core.h, which
// tests/polygon_host.cpp also compiles for the host; DESIGN.md section 25.
//
// One wave owns one ring.  Its lanes take an edge each; an edge toggles one bit
// per row it spans in the bit rows of the ring's clipped bounding box (an edge
// spanning more than kPolygonShortRows rows is shared out over all 64 lanes),
// a lane per row turns the toggles into the inside mask by a suffix XOR, and
// the wave writes the set bits -- O(vertices + box area / 64) where the
// reference tests every pixel against every vertex.  The bit rows sit in LDS
// when they take at most kPolygonLdsWords words: k_polygons_lds, 4 KB a wave,
// which leaves the 32 wave slots of a CU unbounded by its 160 KB of LDS.  A
// larger box goes on a list and takes the memory route after it: the same
// toggles into a zeroed workspace by k_polygons_big_edges, then
// k_polygons_big_fill a wave per row, both spread over the whole chip, since
// such a ring is one of few.
//
// Overlaps do not depend on scheduling: the inside pixels get the ring's list
// index + 1 by atomicMax, so the later ring of a list wins wherever two meet,
// and k_polygon_labels then maps index -> label in place.  No other atomic
// decides a value (the XORs commute; the list of large boxes is built with one,
// but only says which slot of the workspace a ring takes).
#include <algorithm>
#include <climits>
#include <vector>

#include "common.h"
#include "polygon_core.h"

namespace tmh {

constexpr int kPolygonLdsWords = TMH_POLYGON_LDS_WORDS;  // the switch-over: bit-row words of a box
constexpr int kPolygonShortRows = 8;      // an edge spanning more rows is shared out over the wave
constexpr int kPolygonBigEdgeWaves = 64;  // waves per ring of k_polygons_big_edges
constexpr int kPolygonBigFillWaves = 256;
constexpr int kPolygonBigBatch = 32768;   // rings per memory-route launch
constexpr int64_t kPolygonBigWords = int64_t(32) << 20;  // their workspace, at most (one ring always)

enum { kPolyOk = 0, kPolyCoord = 1, kPolyPlane = 2, kPolyEmpty = 3, kPolyFirst = 4 };

struct PolygonCheck {
  int err;
  unsigned int n_big;
  int64_t begin, end;  // first[0], first[n_polygons]
};

// one ring whose box fits no LDS form: its workspace starts at word `offset`
struct PolygonBig {
  int32_t polygon;
  PolygonBox box;
  int32_t pad;
  int64_t offset;
};
static_assert(sizeof(PolygonBig) == 32, "PolygonBig layout");

struct PolygonJob {
  const int32_t* points;
  const int64_t* first;
  const int32_t* plane;
  int32_t* out;
  int H, W;
  int64_t y_offset, x_offset;
};

__global__ void k_polygon_check_lists(const int64_t* __restrict__ first,
                                      const int32_t* __restrict__ plane, int64_t n_polygons,
                                      int64_t n_planes, PolygonCheck* __restrict__ res) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_polygons) return;
  const int64_t a = first[p], b = first[p + 1];
  int err = kPolyOk;
  if (plane[p] < 0 || plane[p] >= n_planes) err = kPolyPlane;
  if (b == a) err = kPolyEmpty;
  if (b < a || (p == 0 && a < 0)) err = kPolyFirst;
  if (err) atomicMax(&res->err, err);
  if (p == 0) res->begin = a;
  if (p == n_polygons - 1) res->end = b;
}

__global__ void k_polygon_check_points(const int32_t* __restrict__ points, int64_t begin,
                                       int64_t end, int64_t y_offset, int64_t x_offset,
                                       PolygonCheck* __restrict__ res) {
  const int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= end) return;
  const int64_t x = polygon_xs(points[2 * i], x_offset), y = polygon_ys(points[2 * i + 1], y_offset);
  if (x <= -kPolygonCoordLimit || x >= kPolygonCoordLimit || y <= -kPolygonCoordLimit ||
      y >= kPolygonCoordLimit)
    atomicMax(&res->err, (int)kPolyCoord);
}

// the ring's clipped box, by all 64 lanes of the calling wave (checked
// coordinates fit an int)
__device__ PolygonBox polygon_ring_box(const PolygonJob& job, int64_t p0, int64_t n) {
  const int lane = threadIdx.x & 63;
  int lx = INT_MAX, hx = INT_MIN, ly = INT_MAX, hy = INT_MIN;
  for (int64_t i = lane; i < n; i += 64) {
    const int x = (int)polygon_xs(job.points[2 * (p0 + i)], job.x_offset);
    const int y = (int)polygon_ys(job.points[2 * (p0 + i) + 1], job.y_offset);
    lx = min(lx, x);
    hx = max(hx, x);
    ly = min(ly, y);
    hy = max(hy, y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lx = min(lx, __shfl_xor(lx, o, 64));
    hx = max(hx, __shfl_xor(hx, o, 64));
    ly = min(ly, __shfl_xor(ly, o, 64));
    hy = max(hy, __shfl_xor(hy, o, 64));
  }
  return polygon_box(lx, hx, ly, hy, job.H, job.W);
}

// The toggles of edges e0 + lane, e0 + stride + lane, ... of the ring by the
// calling wave (all 64 lanes).
template <class Flip>
__device__ void polygon_toggle(const PolygonJob& job, int64_t p0, int64_t n, const PolygonBox& b,
                               int wpr, int64_t e0, int64_t stride, Flip& flip) {
  const int lane = threadIdx.x & 63;
  for (; e0 < n; e0 += stride) {
    const int64_t i = e0 + lane;
    int xi = 0, yi = 0, xj = 0, yj = 0, lo = 0, hi = -1;
    if (i < n) {
      const int64_t j = (i ? i : n) - 1;
      xi = (int)polygon_xs(job.points[2 * (p0 + i)], job.x_offset);
      yi = (int)polygon_ys(job.points[2 * (p0 + i) + 1], job.y_offset);
      xj = (int)polygon_xs(job.points[2 * (p0 + j)], job.x_offset);
      yj = (int)polygon_ys(job.points[2 * (p0 + j) + 1], job.y_offset);
      polygon_edge_span(yi, yj, b, &lo, &hi);
    }
    const bool shared = hi - lo >= kPolygonShortRows;
    unsigned long long m = __ballot(shared);
    while (m) {
      const int src = __builtin_ctzll(m);
      m &= m - 1;
      polygon_edge_rows(__shfl(xi, src, 64), __shfl(yi, src, 64), __shfl(xj, src, 64),
                        __shfl(yj, src, 64), b, wpr, __shfl(lo, src, 64), __shfl(hi, src, 64), lane,
                        64, flip);
    }
    if (!shared) polygon_edge_rows(xi, yi, xj, yj, b, wpr, lo, hi, 0, 1, flip);
  }
}

struct PolygonFlipLds {
  uint64_t* mask;
  __device__ void operator()(int64_t word, uint64_t bit) {
    atomicXor(reinterpret_cast<unsigned long long*>(mask + word), (unsigned long long)bit);
  }
};

struct PolygonFlipMem {
  uint64_t* ws;
  __device__ void operator()(int64_t word, uint64_t bit) {
    atomicXor(reinterpret_cast<unsigned long long*>(ws + word), (unsigned long long)bit);
  }
};

// workgroup (one wave) b draws ring b, or lists it when its box is too large
__global__ __launch_bounds__(64) void k_polygons_lds(PolygonJob job, int64_t n_polygons,
                                                     PolygonCheck* __restrict__ res,
                                                     PolygonBig* __restrict__ big) {
  __shared__ uint64_t mask[kPolygonLdsWords];
  const int64_t p = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (p >= n_polygons) return;
  const int lane = threadIdx.x;
  const int64_t p0 = job.first[p], n = job.first[p + 1] - p0;
  const PolygonBox b = polygon_ring_box(job, p0, n);
  if (polygon_box_empty(b)) return;
  const int bh = b.maxr - b.minr + 1, bw = b.maxc - b.minc + 1, wpr = polygon_wpr(bw);
  const int64_t words = (int64_t)bh * wpr;
  if (words > kPolygonLdsWords) {
    if (lane == 0) {
      PolygonBig e;
      e.polygon = (int32_t)p;
      e.box = b;
      e.pad = 0;
      e.offset = 0;
      big[atomicAdd(&res->n_big, 1u)] = e;
    }
    return;
  }
  for (int i = lane; i < (int)words; i += 64) mask[i] = 0ull;
  __syncthreads();
  PolygonFlipLds flip{mask};
  polygon_toggle(job, p0, n, b, wpr, 0, 64, flip);
  __syncthreads();
  for (int r = lane; r < bh; r += 64) polygon_row_scan(mask + r * wpr, wpr);
  __syncthreads();
  int32_t* out = job.out + (int64_t)job.plane[p] * job.H * job.W + (int64_t)b.minr * job.W + b.minc;
  const int value = (int)p + 1;
  if (wpr == 1) {
    // rows of at most 64 pixels: 64 / span rows a step, span the power of two >= bw
    int shift = 0;
    while ((1 << shift) < bw) ++shift;
    const int per = 64 >> shift, sub = lane >> shift, col = lane & ((1 << shift) - 1);
    for (int r0 = 0; r0 < bh; r0 += per) {
      const int r = r0 + sub;
      if (r < bh && ((mask[r] >> col) & 1ull)) atomicMax(out + (int64_t)r * job.W + col, value);
    }
  } else {
    for (int r = 0; r < bh; ++r)
      for (int k = 0; k < wpr; ++k)
        if ((mask[r * wpr + k] >> lane) & 1ull)
          atomicMax(out + (int64_t)r * job.W + k * 64 + lane, value);
  }
}

// grid (waves, rings): wave x of ring y takes every gridDim.x-th 64 edges
__global__ __launch_bounds__(64) void k_polygons_big_edges(PolygonJob job,
                                                           const PolygonBig* __restrict__ big,
                                                           uint64_t* __restrict__ ws) {
  const PolygonBig e = big[blockIdx.y];
  const int64_t p0 = job.first[e.polygon], n = job.first[e.polygon + 1] - p0;
  PolygonFlipMem flip{ws + e.offset};
  polygon_toggle(job, p0, n, e.box, polygon_wpr(e.box.maxc - e.box.minc + 1),
                 (int64_t)blockIdx.x * 64, (int64_t)gridDim.x * 64, flip);
}

// grid (waves, rings): wave x of ring y takes every gridDim.x-th row.  The
// row's words go 64 at a time from the right, a word per lane; a ballot of the
// words' parities carries the suffix XOR across them.
__global__ __launch_bounds__(64) void k_polygons_big_fill(PolygonJob job,
                                                          const PolygonBig* __restrict__ big,
                                                          const uint64_t* __restrict__ ws) {
  const PolygonBig e = big[blockIdx.y];
  const int lane = threadIdx.x;
  const int bh = e.box.maxr - e.box.minr + 1, wpr = polygon_wpr(e.box.maxc - e.box.minc + 1);
  int32_t* out = job.out + (int64_t)job.plane[e.polygon] * job.H * job.W +
                 (int64_t)e.box.minr * job.W + e.box.minc;
  const int value = e.polygon + 1;
  for (int r = blockIdx.x; r < bh; r += gridDim.x) {
    const uint64_t* row = ws + e.offset + (int64_t)r * wpr;
    unsigned int carry = 0;  // the parity of the words already done
    for (int k0 = ((wpr - 1) >> 6) << 6; k0 >= 0; k0 -= 64) {
      const int k = k0 + lane;
      const uint64_t s = polygon_suffix_xor(k < wpr ? row[k] : 0ull);
      const unsigned long long odd = __ballot((s & 1ull) != 0);
      const unsigned int right = carry ^ ((unsigned)__popcll((odd >> lane) >> 1) & 1u);
      const uint64_t inside = right ? ~s : s;
      carry ^= (unsigned)__popcll(odd) & 1u;
      const unsigned int in_lo = (unsigned int)inside, in_hi = (unsigned int)(inside >> 32);
      const int k1 = min(wpr - k0, 64);
      for (int j = 0; j < k1; ++j) {
        const uint64_t v = (uint64_t)__shfl(in_lo, j, 64) | ((uint64_t)__shfl(in_hi, j, 64) << 32);
        if ((v >> lane) & 1ull)
          atomicMax(out + (int64_t)r * job.W + (int64_t)(k0 + j) * 64 + lane, value);
      }
    }
  }
}

// index + 1 -> label in place, 0 stays 0
__global__ __launch_bounds__(256) void k_polygon_labels(int32_t* __restrict__ out, int64_t n4,
                                                        int64_t total,
                                                        const int32_t* __restrict__ label) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int4* out4 = reinterpret_cast<int4*>(out);
  for (int64_t i = t; i < n4; i += stride) {
    int4 v = out4[i];
    if ((v.x | v.y | v.z | v.w) == 0) continue;
    v.x = v.x ? label[v.x - 1] : 0;
    v.y = v.y ? label[v.y - 1] : 0;
    v.z = v.z ? label[v.z - 1] : 0;
    v.w = v.w ? label[v.w - 1] : 0;
    out4[i] = v;
  }
  for (int64_t i = 4 * n4 + t; i < total; i += stride) {
    const int v = out[i];
    if (v) out[i] = label[v - 1];
  }
}

// The checks of tmh_polygon_fill_device that need the lists: throws TMH_EINVAL
// by name (waits; nothing is written to any output).  *n_points = first[n_polygons].
void polygons_check(const int32_t* points, const int64_t* first, const int32_t* plane,
                    int64_t n_polygons, int64_t n_planes, int64_t y_offset, int64_t x_offset,
                    void* check, int64_t* n_points, hipStream_t s) {
  PolygonCheck* d_res = static_cast<PolygonCheck*>(check);
  PolygonCheck h;
  TMH_HIP(hipMemsetAsync(d_res, 0, sizeof(PolygonCheck), s));
  hipLaunchKernelGGL(k_polygon_check_lists, dim3((unsigned)cdiv(n_polygons, 256)), dim3(256), 0, s,
                     first, plane, n_polygons, n_planes, d_res);
  TMH_HIP(hipGetLastError());
  TMH_HIP(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  TMH_CHECK(h.err != kPolyFirst, TMH_EINVAL, "first is not monotone from a start >= 0");
  TMH_CHECK(h.err != kPolyEmpty, TMH_EINVAL, "an empty ring");
  TMH_CHECK(h.err != kPolyPlane, TMH_EINVAL, "a plane index out of range");
  *n_points = h.end;
  if (h.end > h.begin) {
    hipLaunchKernelGGL(k_polygon_check_points, dim3((unsigned)cdiv(h.end - h.begin, 256)),
                       dim3(256), 0, s, points, h.begin, h.end, y_offset, x_offset, d_res);
    TMH_HIP(hipGetLastError());
    TMH_HIP(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
    TMH_HIP(hipStreamSynchronize(s));
    TMH_CHECK(h.err != kPolyCoord, TMH_EINVAL,
              "a coordinate of magnitude 2^24 or more after the offsets");
  }
}

int64_t polygons_check_bytes() { return (int64_t)sizeof(PolygonCheck); }

// Zeroes out [n_planes][H][W] and draws the checked lists into it (returns
// when done).  check: polygons_check's scratch, zeroed counters.
void polygons_fill(const int32_t* points, const int64_t* first, const int32_t* plane,
                   const int32_t* label, int64_t n_polygons, int64_t n_planes, int H, int W,
                   int64_t y_offset, int64_t x_offset, int32_t* out, void* check, hipStream_t s) {
  ProfScope prof("polygons", s);
  const int64_t total = n_planes * H * W;
  TMH_HIP(hipMemsetAsync(out, 0, (size_t)total * sizeof(int32_t), s));
  if (n_polygons == 0) {
    TMH_HIP(hipStreamSynchronize(s));
    return;
  }
  PolygonCheck* d_res = static_cast<PolygonCheck*>(check);
  PolygonBig* d_big = nullptr;
  uint64_t* d_ws = nullptr;
  struct Free {
    PolygonBig*& a;
    uint64_t*& b;
    ~Free() {
      if (a) (void)hipFree(a);
      if (b) (void)hipFree(b);
    }
  } guard{d_big, d_ws};
  if (hipMalloc(&d_big, (size_t)n_polygons * sizeof(PolygonBig)) != hipSuccess) {
    d_big = nullptr;
    throw Error{TMH_ENOMEM, "hipMalloc of the large rings' list failed"};
  }
  const PolygonJob job{points, first, plane, out, H, W, y_offset, x_offset};
  const unsigned gx = (unsigned)std::min<int64_t>(n_polygons, 65536);
  hipLaunchKernelGGL(k_polygons_lds, dim3(gx, (unsigned)cdiv(n_polygons, gx)), dim3(64), 0, s, job,
                     n_polygons, d_res, d_big);
  TMH_HIP(hipGetLastError());
  PolygonCheck h;
  TMH_HIP(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  if (h.n_big > 0) {
    // the memory route, in batches that share one workspace
    std::vector<PolygonBig> big(h.n_big);
    TMH_HIP(hipMemcpyAsync(big.data(), d_big, big.size() * sizeof(PolygonBig),
                           hipMemcpyDeviceToHost, s));
    TMH_HIP(hipStreamSynchronize(s));
    auto words_of = [](const PolygonBig& e) {
      return (int64_t)(e.box.maxr - e.box.minr + 1) * polygon_wpr(e.box.maxc - e.box.minc + 1);
    };
    std::vector<size_t> batch_end;
    int64_t ws_words = 0, used = 0;
    size_t begin = 0;
    for (size_t i = 0; i < big.size(); ++i) {
      const int64_t w = words_of(big[i]);
      if (i > begin && (used + w > kPolygonBigWords || i - begin >= (size_t)kPolygonBigBatch)) {
        batch_end.push_back(i);
        begin = i;
        used = 0;
      }
      big[i].offset = used;
      used += w;
      ws_words = std::max(ws_words, used);
    }
    batch_end.push_back(big.size());
    TMH_HIP(hipMemcpyAsync(d_big, big.data(), big.size() * sizeof(PolygonBig),
                           hipMemcpyHostToDevice, s));
    if (hipMalloc(&d_ws, (size_t)ws_words * 8) != hipSuccess) {
      d_ws = nullptr;
      throw Error{TMH_ENOMEM, "hipMalloc of the large rings' workspace failed"};
    }
    begin = 0;
    for (size_t end : batch_end) {
      int64_t batch_words = 0;
      for (size_t i = begin; i < end; ++i) batch_words += words_of(big[i]);
      TMH_HIP(hipMemsetAsync(d_ws, 0, (size_t)batch_words * 8, s));
      const unsigned n = (unsigned)(end - begin);
      hipLaunchKernelGGL(k_polygons_big_edges, dim3(kPolygonBigEdgeWaves, n), dim3(64), 0, s, job,
                         d_big + begin, d_ws);
      hipLaunchKernelGGL(k_polygons_big_fill, dim3(kPolygonBigFillWaves, n), dim3(64), 0, s, job,
                         d_big + begin, d_ws);
      TMH_HIP(hipGetLastError());
      begin = end;
    }
  }
  const int64_t n4 = (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? total / 4 : 0;
  const int64_t work = std::max<int64_t>(n4, total - 4 * n4);
  hipLaunchKernelGGL(k_polygon_labels, dim3((unsigned)std::min<int64_t>(cdiv(work, 256), 8192)),
                     dim3(256), 0, s, out, n4, total, label);
  TMH_HIP(hipGetLastError());
  TMH_HIP(hipStreamSynchronize(s));  // the list and the workspace are freed on return
}

}  // namespace tmh
