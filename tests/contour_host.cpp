// Stand-alone host harness over tmlibrary_amd/csrc/contour_core.h: the opening
// and the border follower the contour kernels run, compiled with g++ (and, by
// tests/test_contours_cpu.py, once more under -fsanitize=address,undefined).
//
//   contour_host IN OUT [REPS]
// IN:  int32 n_cases, then per case int32 h, w, open and h * w bytes (a mask
//      whose outermost rows and columns are zero).
// OUT: per case the h * w bytes of the mask after the opening (if open), int32
//      n_contours, then per contour int32 is_hole, parent, n_points and
//      n_points (x, y) int32 pairs, in discovery order.
// REPS > 1 repeats the work (tools/bench_contours.py times it); OUT is the
// last repeat's.  Every buffer is a heap block of its exact size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define TMH_CHD inline
#include "../tmlibrary_amd/csrc/contour_core.h"

namespace {

struct Border {
  int is_hole, parent;
  std::vector<int32_t> xy;
};

struct Sink {
  std::vector<Border> borders;
  void begin(int is_hole, int lnbd) {
    Border b;
    b.is_hole = is_hole;
    b.parent = tmh::contour_parent(is_hole, lnbd, lnbd >= 0 ? borders[(size_t)lnbd].is_hole : 0,
                                   lnbd >= 0 ? borders[(size_t)lnbd].parent : -1);
    borders.push_back(b);
  }
  void point(int x, int y) {
    borders.back().xy.push_back(x);
    borders.back().xy.push_back(y);
  }
  void end() {}
};

bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: contour_host IN OUT [REPS]\n");
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
      if (!read_all(in, hdr, 12)) return 4;
      const int h = hdr[0], w = hdr[1], wpr = tmh::contour_wpr(w);
      if (h < 3 || w < 3) return 5;
      uint8_t* px = (uint8_t*)malloc((size_t)h * w);
      if (!read_all(in, px, (size_t)h * w)) return 4;
      const size_t words = (size_t)h * wpr;
      uint64_t* mask = (uint64_t*)calloc(words, 8);
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
          if (px[(size_t)y * w + x]) mask[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
      if (hdr[2]) {
        uint64_t* tmp = (uint64_t*)calloc(words, 8);
        for (int y = 0; y < h; ++y)
          for (int k = 0; k < wpr; ++k)
            tmp[(size_t)y * wpr + k] = tmh::contour_cross_word(mask, h, wpr, y, k, true);
        for (int y = 0; y < h; ++y)
          for (int k = 0; k < wpr; ++k)
            mask[(size_t)y * wpr + k] = tmh::contour_cross_word(tmp, h, wpr, y, k, false);
        free(tmp);
      }
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) px[(size_t)y * w + x] = (uint8_t)tmh::contour_bit(mask, wpr, y, x);
      fwrite(px, 1, (size_t)h * w, out);
      int32_t* marks = (int32_t*)calloc((size_t)h * w, 4);
      Sink sink;
      tmh::contour_follow(mask, marks, h, w, wpr, sink);
      const int32_t n = (int32_t)sink.borders.size();
      fwrite(&n, 4, 1, out);
      for (const Border& b : sink.borders) {
        const int32_t e[3] = {b.is_hole, b.parent, (int32_t)(b.xy.size() / 2)};
        fwrite(e, 4, 3, out);
        fwrite(b.xy.data(), 4, b.xy.size(), out);
      }
      free(marks);
      free(mask);
      free(px);
    }
    fclose(in);
    if (fclose(out) != 0) return 6;
  }
  return 0;
}
