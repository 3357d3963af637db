// jterator object outlines (gfx950 / MI355X): what SegmentationImage.
// extract_polygons (tmlib/image.py:778-917) computes per label before it picks
// a shell and holes -- the mask of the label inside its padded bounding box on
// the border-zeroed plane, mh.open's opening by the 3x3 cross when the mask has
// more than one pixel, and every border cv2.findContours(RETR_CCOMP,
// CHAIN_APPROX_NONE) follows on it.  The rules are in contour_core.h, which
// tests/contour_host.cpp also compiles for the host; DESIGN.md section 21.
//
// One wave owns one object, a row of tmh_object_table's result with n > 0 and
// label > 0.  All 64 lanes stage the mask as bit rows (one ballot per 64
// pixels is one word; the interior pixel count and coordinate sums the first
// fallback needs fall out of the same loop) and open it a word per lane; lane
// 0 then follows the borders, which is serial in its steps.  The mask, the
// eroded copy and one int16 mark per pixel sit in LDS when the padded box has
// at most kContourLdsPixels pixels: k_contours_lds in three sizes -- 3 KB a
// wave up to kContourLdsTinyPixels (every row of the table gets a workgroup,
// most leave at once), 12 KB up to kContourLdsSmallPixels and 40 KB above
// (both dealt from lists) -- since LDS per wave is what bounds the waves a CU
// traces at once.  A larger box takes
// k_contours_big: the same code over a workspace in memory with int32 marks,
// exact for any box up to a whole plane, a slot per resident wave, objects
// dealt from a list.
//
// The result is compact and ordered: a count pass gives every object its
// number of borders and points, k_contour_scan turns the counts into offsets
// in (plane, label) order, and a write pass traces again at those offsets.  No
// atomic decides a position (the three lists are built with one, but only say
// which wave traces which object), so the bytes do not depend on scheduling.
#include <algorithm>

#include "common.h"
#include "contour_core.h"

namespace tmh {

constexpr int kContourLdsPixels = TMH_CONTOUR_LDS_PIXELS;  // the switch-over: padded box pixels
constexpr int kContourLdsSmallPixels = TMH_CONTOUR_LDS_SMALL_PIXELS;  // between the LDS sizes
constexpr int kContourLdsTinyPixels = TMH_CONTOUR_LDS_TINY_PIXELS;
// bit-row words of a box in LDS, tiny, small and large: only a box of under
// 16 columns (32 in the large form) with more rows than this has more, and
// goes one form up
constexpr int kContourLdsTinyWords = 64, kContourLdsSmallWords = 256, kContourLdsWords = 512;
constexpr int kContourBigWaves = 1024;                     // resident waves of k_contours_big
constexpr int64_t kContourBigBytes = int64_t(512) << 20;   // their workspace, at most (one slot always)

static_assert(sizeof(tmh_contour) == 32, "tmh_contour layout (include/tmhip.h)");
static_assert(sizeof(tmh_contour_object) == 64, "tmh_contour_object layout (include/tmhip.h)");
static_assert(kContourLdsPixels / 2 < 32767, "int16 marks hold every border of an LDS box");

struct ContourDims {
  unsigned long long words, pixels;  // the largest of any object of class 3
  unsigned int n_list[4];            // objects of class 4, 3, 2; unused
};

// 0: nothing to trace (or a row that is no bounding box of an H x W plane),
// 1, 2, 3: the box fits the tiny, the small, the large LDS form, 4: none
__device__ __forceinline__ int contour_class(const tmh_object_row& r, int label, int H, int W) {
  if (label == 0 || r.n <= 0) return 0;
  if (r.y0 < 0 || r.y0 >= r.y1 || r.y1 > H || r.x0 < 0 || r.x0 >= r.x1 || r.x1 > W) return 0;
  const int64_t h = (int64_t)r.y1 - r.y0 + 2, w = (int64_t)r.x1 - r.x0 + 2;
  const int64_t px = h * w, words = h * contour_wpr((int)w);
  if (px <= kContourLdsTinyPixels && words <= kContourLdsTinyWords) return 1;
  if (px <= kContourLdsSmallPixels && words <= kContourLdsSmallWords) return 2;
  return (px <= kContourLdsPixels && words <= kContourLdsWords) ? 3 : 4;
}

__global__ void k_contour_init(const tmh_object_row* __restrict__ rows, int64_t n_rows,
                               int32_t max_label, int H, int W,
                               tmh_contour_object* __restrict__ objects,
                               ContourDims* __restrict__ dims, int32_t* __restrict__ lists) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t per = (int64_t)max_label + 1;
  tmh_contour_object o;
  o.plane = (int32_t)(i / per);
  o.label = (int32_t)(i - (int64_t)o.plane * per);
  o.first_contour = o.first_point = 0;
  o.n_contours = o.opened = 0;
  o.n_points = o.n_interior = o.sum_y = o.sum_x = 0;
  objects[i] = o;
  const tmh_object_row r = rows[i];
  const int cls = contour_class(r, o.label, H, W);
  if (cls >= 2)  // list 4 - cls holds n_rows entries
    lists[(int64_t)(4 - cls) * n_rows + atomicAdd(&dims->n_list[4 - cls], 1u)] = (int32_t)i;
  if (cls == 4) {
    const unsigned long long h = (unsigned long long)(r.y1 - r.y0 + 2),
                             w = (unsigned long long)(r.x1 - r.x0 + 2);
    atomicMax(&dims->words, h * (unsigned long long)contour_wpr((int)w));
    atomicMax(&dims->pixels, h * w);
  }
}

struct ContourCount {
  int nc = 0;
  int64_t np = 0;
  __device__ void begin(int, int) { ++nc; }
  __device__ void point(int, int) { ++np; }
  __device__ void end() {}
};

struct ContourWrite {
  tmh_contour* tab;   // the object's first entry
  int32_t* pts;       // the object's first point
  int64_t base;       // its index among all points
  int plane, label;
  int nc = 0;
  int64_t np = 0, start = 0;
  __device__ void begin(int is_hole, int lnbd) {
    tmh_contour c;
    c.plane = plane;
    c.label = label;
    c.is_hole = is_hole;
    c.parent = contour_parent(is_hole, lnbd, lnbd >= 0 ? tab[lnbd].is_hole : 0,
                              lnbd >= 0 ? tab[lnbd].parent : -1);
    c.point_offset = base + np;
    c.n_points = 0;
    tab[nc] = c;
    start = np;
  }
  __device__ void point(int x, int y) {
    pts[2 * np] = x;
    pts[2 * np + 1] = y;
    ++np;
  }
  __device__ void end() {
    tab[nc].n_points = np - start;
    ++nc;
  }
};

struct ContourJob {
  const int32_t* planes;
  const tmh_object_row* rows;
  tmh_contour_object* objects;
  tmh_contour* contours;  // the write pass's
  int32_t* points;
  int H, W;
  int32_t max_label;
};

// Object `idx` by the calling wave (all 64 lanes, no other wave in the
// workgroup): mask and tmp hold h * wpr words, marks h * w.
template <class M, bool kWrite>
__device__ void contour_object(const ContourJob& job, int64_t idx, uint64_t* mask, uint64_t* tmp,
                               M* marks) {
  const int lane = threadIdx.x & 63;
  tmh_contour_object* obj = job.objects + idx;
  const int64_t per = (int64_t)job.max_label + 1;
  const int plane = (int)(idx / per), label = (int)(idx - plane * per);
  if (kWrite && obj->n_contours == 0) return;
  const tmh_object_row r = job.rows[idx];
  const int h = r.y1 - r.y0 + 2, w = r.x1 - r.x0 + 2, wpr = contour_wpr(w);
  const int32_t* img = job.planes + (int64_t)plane * job.H * job.W;
  // stage: pixel (y, x) of the padded box is plane pixel (y0 + y - 1, x0 + x - 1),
  // set if it holds the label and is off the plane's four border lines
  // (label > 0, so -1 stands for any pixel that cannot be set); kStage words'
  // loads are in flight before the first ballot
  constexpr int kStage = 4;
  const int64_t words = (int64_t)h * wpr;
  unsigned long long cnt = 0, sy = 0, sx = 0;
  for (int64_t i0 = 0; i0 < words; i0 += kStage) {
    int v[kStage], Y[kStage], X[kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const int64_t i = i0 + u;
      const int y = (int)(i / wpr), x = (int)(i - (int64_t)y * wpr) * 64 + lane;
      Y[u] = r.y0 + y - 1;
      X[u] = r.x0 + x - 1;
      const bool in = i < words && y >= 1 && y <= h - 2 && Y[u] >= 1 && Y[u] <= job.H - 2 &&
                      x >= 1 && x <= w - 2 && X[u] >= 1 && X[u] <= job.W - 2;
      v[u] = in ? img[(int64_t)Y[u] * job.W + X[u]] : -1;
    }
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const bool bit = v[u] == label;
      const unsigned long long word = __ballot(bit);
      if (lane == 0 && i0 + u < words) mask[i0 + u] = word;
      if (bit) {
        ++cnt;
        sy += (unsigned long long)Y[u];
        sx += (unsigned long long)X[u];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sy += __shfl_xor(sy, o, 64);
    sx += __shfl_xor(sx, o, 64);
  }
  if (cnt == 0) return;  // the label lives on the border lines only: nothing (k_contour_init's zeros)
  __syncthreads();
  const bool opened = cnt > 1;
  if (opened) {
    for (int64_t i = lane; i < words; i += 64)
      tmp[i] = contour_cross_word(mask, h, wpr, (int)(i / wpr), (int)(i % wpr), true);
    __syncthreads();
    for (int64_t i = lane; i < words; i += 64)
      mask[i] = contour_cross_word(tmp, h, wpr, (int)(i / wpr), (int)(i % wpr), false);
  }
  const int64_t pixels = (int64_t)h * w;
  for (int64_t i = lane; i < pixels; i += 64) marks[i] = (M)0;
  __syncthreads();
  if (lane != 0) return;
  if (kWrite) {
    ContourWrite sink;
    sink.tab = job.contours + obj->first_contour;
    sink.pts = job.points + 2 * obj->first_point;
    sink.base = obj->first_point;
    sink.plane = plane;
    sink.label = label;
    contour_follow(mask, marks, h, w, wpr, sink);
  } else {
    ContourCount sink;
    contour_follow(mask, marks, h, w, wpr, sink);
    obj->n_contours = sink.nc;
    obj->n_points = sink.np;
    obj->opened = opened ? 1 : 0;
    obj->n_interior = (int64_t)cnt;
    obj->sum_y = (int64_t)sy;
    obj->sum_x = (int64_t)sx;
  }
}

// list == null: workgroup b takes row b of the table if it is of class 1;
// else the object list[b]
template <bool kWrite, int kPixels, int kWords>
__global__ __launch_bounds__(64) void k_contours_lds(ContourJob job, int64_t n,
                                                     const int32_t* __restrict__ list) {
  __shared__ uint64_t mask[kWords], tmp[kWords];
  __shared__ int16_t marks[kPixels];
  int64_t idx = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (idx >= n) return;
  if (list) {
    idx = list[idx];
  } else {
    const int label = (int)(idx % ((int64_t)job.max_label + 1));
    if (contour_class(job.rows[idx], label, job.H, job.W) != 1) return;
  }
  contour_object<int16_t, kWrite>(job, idx, mask, tmp, marks);
}

// workspace slot of workgroup b: words mask, words tmp, pixels marks
template <bool kWrite>
__global__ __launch_bounds__(64) void k_contours_big(ContourJob job, const int32_t* __restrict__ list,
                                                     int n_big, uint64_t* __restrict__ ws,
                                                     int64_t slot_words, int64_t words) {
  uint64_t* mask = ws + (int64_t)blockIdx.x * slot_words;
  uint64_t* tmp = mask + words;
  int32_t* marks = reinterpret_cast<int32_t*>(tmp + words);
  for (int i = blockIdx.x; i < n_big; i += gridDim.x) {
    contour_object<int32_t, kWrite>(job, list[i], mask, tmp, marks);
    __syncthreads();  // the slot is reused
  }
}

// exclusive scan of the objects' border and point counts, (plane, label) order
__global__ __launch_bounds__(1024) void k_contour_scan(tmh_contour_object* __restrict__ objects,
                                                       int64_t n_rows, int64_t* __restrict__ totals) {
  __shared__ int64_t part_c[1024], part_p[1024];
  const int t = threadIdx.x;
  const int64_t per = cdiv(n_rows, 1024);
  const int64_t i0 = min(n_rows, t * per), i1 = min(n_rows, i0 + per);
  int64_t c = 0, p = 0;
  for (int64_t i = i0; i < i1; ++i) {
    c += objects[i].n_contours;
    p += objects[i].n_points;
  }
  part_c[t] = c;
  part_p[t] = p;
  __syncthreads();
  if (t == 0) {
    int64_t rc = 0, rp = 0;
    for (int k = 0; k < 1024; ++k) {
      const int64_t vc = part_c[k], vp = part_p[k];
      part_c[k] = rc;
      part_p[k] = rp;
      rc += vc;
      rp += vp;
    }
    totals[0] = rc;
    totals[1] = rp;
  }
  __syncthreads();
  c = part_c[t];
  p = part_p[t];
  for (int64_t i = i0; i < i1; ++i) {
    objects[i].first_contour = c;
    objects[i].first_point = p;
    c += objects[i].n_contours;
    p += objects[i].n_points;
  }
}

namespace {

struct BigPlan {
  int grid = 0;
  int64_t words = 0, slot_words = 0;
};

BigPlan big_plan(const ContourDims& d) {
  BigPlan b;
  if (d.n_list[0] == 0) return b;
  b.words = (int64_t)d.words;
  b.slot_words = 2 * b.words + ((int64_t)d.pixels + 1) / 2;  // int32 marks, two to a word
  const int64_t fit = std::max<int64_t>(1, kContourBigBytes / (b.slot_words * 8));
  b.grid = (int)std::min<int64_t>({(int64_t)d.n_list[0], (int64_t)kContourBigWaves, fit});
  return b;
}

template <bool kWrite>
void launch_contour_pass(const ContourJob& job, int64_t n_rows, const ContourDims& d,
                         const int32_t* lists, uint64_t* ws, hipStream_t s) {
  auto grid = [](int64_t n) {
    const unsigned gx = (unsigned)std::min<int64_t>(n, 65536);
    return dim3(gx, (unsigned)cdiv(n, gx));
  };
  hipLaunchKernelGGL((k_contours_lds<kWrite, kContourLdsTinyPixels, kContourLdsTinyWords>),
                     grid(n_rows), dim3(64), 0, s, job, n_rows, (const int32_t*)nullptr);
  if (d.n_list[2] > 0)
    hipLaunchKernelGGL((k_contours_lds<kWrite, kContourLdsSmallPixels, kContourLdsSmallWords>),
                       grid(d.n_list[2]), dim3(64), 0, s, job, (int64_t)d.n_list[2],
                       lists + 2 * n_rows);
  if (d.n_list[1] > 0)
    hipLaunchKernelGGL((k_contours_lds<kWrite, kContourLdsPixels, kContourLdsWords>),
                       grid(d.n_list[1]), dim3(64), 0, s, job, (int64_t)d.n_list[1],
                       lists + n_rows);
  const BigPlan b = big_plan(d);
  if (b.grid > 0)
    hipLaunchKernelGGL(k_contours_big<kWrite>, dim3((unsigned)b.grid), dim3(64), 0, s, job, lists,
                       (int)d.n_list[0], ws, b.slot_words, b.words);
  TMH_HIP(hipGetLastError());
}

}  // namespace

// Count pass and scan: objects [n_planes * (max_label + 1)] filled, the totals
// (borders, points) on the host.  scratch: what the write pass reuses.
void contours_measure(const int32_t* planes, int64_t n_planes, int H, int W, int32_t max_label,
                      const tmh_object_row* rows, tmh_contour_object* objects,
                      ContourScratch& scratch, int64_t* n_contours, int64_t* n_points,
                      hipStream_t s) {
  ProfScope prof("contours", s);
  const int64_t n_rows = n_planes * ((int64_t)max_label + 1);
  scratch.n_rows = n_rows;
  TMH_HIP(hipMalloc(&scratch.lists, (size_t)n_rows * 3 * sizeof(int32_t)));  // class 4, 3, 2
  TMH_HIP(hipMalloc(&scratch.dims, sizeof(ContourDims) + 2 * sizeof(int64_t)));
  ContourDims* d_dims = static_cast<ContourDims*>(scratch.dims);
  int64_t* d_totals = reinterpret_cast<int64_t*>(d_dims + 1);
  TMH_HIP(hipMemsetAsync(d_dims, 0, sizeof(ContourDims) + 2 * sizeof(int64_t), s));
  hipLaunchKernelGGL(k_contour_init, dim3((unsigned)cdiv(n_rows, 256)), dim3(256), 0, s, rows, n_rows,
                     max_label, H, W, objects, d_dims, scratch.lists);
  ContourDims d;
  TMH_HIP(hipMemcpyAsync(&d, d_dims, sizeof(d), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  scratch.words = d.words;
  scratch.pixels = d.pixels;
  for (int i = 0; i < 3; ++i) scratch.n_list[i] = d.n_list[i];
  const BigPlan b = big_plan(d);
  if (b.grid > 0) {
    if (hipMalloc(&scratch.ws, (size_t)b.grid * b.slot_words * 8) != hipSuccess) {
      scratch.ws = nullptr;
      throw Error{TMH_ENOMEM, "hipMalloc of the large objects' contour workspace failed"};
    }
  }
  ContourJob job{planes, rows, objects, nullptr, nullptr, H, W, max_label};
  launch_contour_pass<false>(job, n_rows, d, scratch.lists, scratch.ws, s);
  hipLaunchKernelGGL(k_contour_scan, dim3(1), dim3(1024), 0, s, objects, n_rows, d_totals);
  TMH_HIP(hipGetLastError());
  int64_t totals[2];
  TMH_HIP(hipMemcpyAsync(totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  *n_contours = totals[0];
  *n_points = totals[1];
}

// Write pass after contours_measure on the same arguments (returns when done).
void contours_write(const int32_t* planes, int H, int W, int32_t max_label,
                    const tmh_object_row* rows, tmh_contour_object* objects,
                    const ContourScratch& scratch, tmh_contour* contours, int32_t* points,
                    hipStream_t s) {
  ProfScope prof("contours", s);
  ContourDims d;
  d.words = scratch.words;
  d.pixels = scratch.pixels;
  for (int i = 0; i < 3; ++i) d.n_list[i] = scratch.n_list[i];
  d.n_list[3] = 0;
  ContourJob job{planes, rows, objects, contours, points, H, W, max_label};
  launch_contour_pass<true>(job, scratch.n_rows, d, scratch.lists, scratch.ws, s);
  TMH_HIP(hipStreamSynchronize(s));
}

ContourScratch::~ContourScratch() {
  if (lists) (void)hipFree(lists);
  if (dims) (void)hipFree(dims);
  if (ws) (void)hipFree(ws);
}

}  // namespace tmh
