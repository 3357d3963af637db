// Stand-alone host harness over tmlibrary_amd/csrc/polygon_core.h: the box, the
// edge toggles and the suffix XOR the polygon kernels run, compiled with g++
// (and, by tests/test_polygons_cpu.py, once more under
// -fsanitize=address,undefined).
//
//   polygon_host IN OUT [REPS]
// IN:  int32 n_cases, then per case int32 H, W, n_rings, int64 y_offset,
//      x_offset, and per ring int32 label, n and n global (x, y) int32 pairs.
// OUT: per case the H * W int32 of the plane, the rings drawn in list order.
//      A ring with n = 0 or a transformed coordinate of magnitude 2^24 or more
//      ends the run with status 7, as the library refuses them.
// REPS > 1 repeats the work (tools/bench_polygons.py times it); OUT is the
// last repeat's.  Every buffer is a heap block of its exact size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define TMH_CHD inline
#include "../tmlibrary_amd/csrc/polygon_core.h"

namespace {

struct Flip {
  uint64_t* mask;
  void operator()(int64_t word, uint64_t bit) { mask[word] ^= bit; }
};

bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// one ring into the plane; false: refused
bool draw(int32_t* plane, int H, int W, int32_t label, const int32_t* pts, int n, int64_t y_offset,
          int64_t x_offset) {
  if (n <= 0) return false;
  int64_t* xs = (int64_t*)malloc((size_t)n * 8);
  int64_t* ys = (int64_t*)malloc((size_t)n * 8);
  int64_t lx = INT64_MAX, hx = INT64_MIN, ly = INT64_MAX, hy = INT64_MIN;
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    xs[i] = tmh::polygon_xs(pts[2 * i], x_offset);
    ys[i] = tmh::polygon_ys(pts[2 * i + 1], y_offset);
    const int64_t lim = tmh::kPolygonCoordLimit;
    if (xs[i] <= -lim || xs[i] >= lim || ys[i] <= -lim || ys[i] >= lim) ok = false;
    if (xs[i] < lx) lx = xs[i];
    if (xs[i] > hx) hx = xs[i];
    if (ys[i] < ly) ly = ys[i];
    if (ys[i] > hy) hy = ys[i];
  }
  if (ok) {
    const tmh::PolygonBox b = tmh::polygon_box(lx, hx, ly, hy, H, W);
    if (!tmh::polygon_box_empty(b)) {
      const int bh = b.maxr - b.minr + 1, bw = b.maxc - b.minc + 1, wpr = tmh::polygon_wpr(bw);
      uint64_t* mask = (uint64_t*)calloc((size_t)bh * wpr, 8);
      Flip flip{mask};
      for (int i = 0; i < n; ++i) {
        const int j = (i ? i : n) - 1;
        int lo, hi;
        tmh::polygon_edge_span(ys[i], ys[j], b, &lo, &hi);
        tmh::polygon_edge_rows(xs[i], ys[i], xs[j], ys[j], b, wpr, lo, hi, 0, 1, flip);
      }
      for (int r = 0; r < bh; ++r) {
        tmh::polygon_row_scan(mask + (size_t)r * wpr, wpr);
        for (int k = 0; k < bw; ++k)
          if ((mask[(size_t)r * wpr + (k >> 6)] >> (k & 63)) & 1ull)
            plane[(size_t)(b.minr + r) * W + b.minc + k] = label;
      }
      free(mask);
    }
  }
  free(xs);
  free(ys);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: polygon_host IN OUT [REPS]\n");
    return 2;
  }
  const int reps = argc > 3 ? atoi(argv[3]) : 1;
  for (int rep = 0; rep < reps; ++rep) {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t n_cases = 0;
    if (!read_all(in, &n_cases, 4)) return 4;
    for (int32_t c = 0; c < n_cases; ++c) {
      int32_t hdr[3];
      int64_t off[2];
      if (!read_all(in, hdr, 12) || !read_all(in, off, 16)) return 4;
      const int H = hdr[0], W = hdr[1];
      if (H < 1 || W < 1) return 5;
      int32_t* plane = (int32_t*)calloc((size_t)H * W, 4);
      for (int32_t k = 0; k < hdr[2]; ++k) {
        int32_t ring[2];
        if (!read_all(in, ring, 8) || ring[1] < 0) return 4;
        int32_t* pts = (int32_t*)malloc((size_t)ring[1] * 8 + 1);
        if (!read_all(in, pts, (size_t)ring[1] * 8)) return 4;
        const bool ok = draw(plane, H, W, ring[0], pts, ring[1], off[0], off[1]);
        free(pts);
        if (!ok) return 7;
      }
      fwrite(plane, 4, (size_t)H * W, out);
      free(plane);
    }
    fclose(in);
    if (fclose(out) != 0) return 6;
  }
  return 0;
}
