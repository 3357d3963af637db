// Filling one outline of jterator's create_from_polygons (tmlib/image.py:740-776):
// skimage.draw.polygon's rule as scikit-image 0.13.0 has it -- every integer
// pixel (r, c) of the ring's bounding box, clipped to the plane, is inside when
// an odd number of edges (i, j = i - 1) satisfy
//   (ys[i] <= r < ys[j] or ys[j] <= r < ys[i]) and
//   c < (xs[j] - xs[i]) * (r - ys[i]) / (ys[j] - ys[i]) + xs[i]
// in f64.  Kept free of HIP headers so that the code k_polygons_lds and the
// memory route run (polygon_kernels.hip) also builds for the host
// (tests/polygon_host.cpp).  DESIGN.md section 25.
//
// With integer vertices below 2^24 in magnitude the comparison is the exact
// rational one (25.1), and for integer c, c < q is c < ceil(q).  So an edge
// does not test pixels: in every row it spans it toggles ONE bit, at column
// ceil(q), of a bit row of the box -- bit k of a row is column minc + k, word
// k / 64, wpr words a row -- and a suffix XOR along the row (pixel k is the
// XOR of the bits at k and above) turns the toggles into the inside mask.  A
// toggle for column t flips the pixels c < t, so it is stored at bit
// t - minc - 1: t <= minc flips nothing in the box and is dropped, t > maxc
// flips the whole row and lands on the last bit.
#pragma once

#include <cstdint>

#ifndef TMH_CHD
#define TMH_CHD __host__ __device__ __forceinline__
#endif

namespace tmh {

namespace {

// transformed coordinates must stay below this in magnitude (25.1)
constexpr int64_t kPolygonCoordLimit = int64_t(1) << 24;

struct PolygonBox {
  int minr, maxr, minc, maxc;  // both ends inclusive; empty when minr > maxr or minc > maxc
};

TMH_CHD int polygon_wpr(int w) { return (w + 63) >> 6; }

// xs = x - x_offset, ys = -y - y_offset of a stored (x, y) pair
TMH_CHD int64_t polygon_xs(int32_t x, int64_t x_offset) { return (int64_t)x - x_offset; }
TMH_CHD int64_t polygon_ys(int32_t y, int64_t y_offset) { return -(int64_t)y - y_offset; }

// The scanned box from the ring's extremes (integers, so the rule's ceil is
// the identity): rows max(0, min ys) .. min(H - 1, max ys), columns alike.
TMH_CHD PolygonBox polygon_box(int64_t min_x, int64_t max_x, int64_t min_y, int64_t max_y, int H,
                               int W) {
  PolygonBox b;
  b.minr = (int)(min_y < 0 ? 0 : (min_y > H ? H : min_y));
  b.maxr = (int)(max_y > H - 1 ? H - 1 : (max_y < -1 ? -1 : max_y));
  b.minc = (int)(min_x < 0 ? 0 : (min_x > W ? W : min_x));
  b.maxc = (int)(max_x > W - 1 ? W - 1 : (max_x < -1 ? -1 : max_x));
  return b;
}

TMH_CHD bool polygon_box_empty(const PolygonBox& b) { return b.minr > b.maxr || b.minc > b.maxc; }

// ceil(n / d), d > 0
TMH_CHD int64_t polygon_ceil_div(int64_t n, int64_t d) {
  if (d == 1) return n;
  return n >= 0 ? (n + d - 1) / d : -((-n) / d);
}

// ceil of the rule's crossing abscissa of edge (xi, yi) <- (xj, yj) in row r,
// yi != yj: xi + ceil((xj - xi) * (r - yi) / (yj - yi)).  Differences stay
// below 2^25, their product below 2^50.
TMH_CHD int64_t polygon_crossing(int64_t xi, int64_t yi, int64_t xj, int64_t yj, int64_t r) {
  int64_t num = (xj - xi) * (r - yi), den = yj - yi;
  if (den < 0) {
    num = -num;
    den = -den;
  }
  return xi + polygon_ceil_div(num, den);
}

// Rows of the box the edge spans: ylo <= r < yhi, clipped.  lo > hi: none.
TMH_CHD void polygon_edge_span(int64_t yi, int64_t yj, const PolygonBox& b, int* lo, int* hi) {
  const int64_t ylo = yi < yj ? yi : yj, yhi = (yi < yj ? yj : yi) - 1;
  *lo = (int)(ylo < b.minr ? b.minr : (ylo > (int64_t)b.maxr + 1 ? (int64_t)b.maxr + 1 : ylo));
  *hi = (int)(yhi > b.maxr ? b.maxr : (yhi < (int64_t)b.minr - 1 ? (int64_t)b.minr - 1 : yhi));
}

// The edge's toggles in rows lo + first, lo + first + step, ... <= hi of its
// span: flip(word index, bit mask) XORs into the box's bit rows.
template <class Flip>
TMH_CHD void polygon_edge_rows(int64_t xi, int64_t yi, int64_t xj, int64_t yj, const PolygonBox& b,
                               int wpr, int lo, int hi, int first, int step, Flip& flip) {
  for (int r = lo + first; r <= hi; r += step) {
    int64_t t = polygon_crossing(xi, yi, xj, yj, r);
    if (t <= b.minc) continue;
    if (t > (int64_t)b.maxc + 1) t = (int64_t)b.maxc + 1;
    const int k = (int)(t - b.minc - 1);
    flip((int64_t)(r - b.minr) * wpr + (k >> 6), 1ull << (k & 63));
  }
}

// bit k of the result: the XOR of bits k..63
TMH_CHD uint64_t polygon_suffix_xor(uint64_t v) {
  v ^= v >> 1;
  v ^= v >> 2;
  v ^= v >> 4;
  v ^= v >> 8;
  v ^= v >> 16;
  v ^= v >> 32;
  return v;
}

// One bit row from toggles to the inside mask, in place: the suffix XOR, the
// parity of the words to the right carried into each word.
TMH_CHD void polygon_row_scan(uint64_t* row, int wpr) {
  uint64_t carry = 0;
  for (int k = wpr - 1; k >= 0; --k) {
    const uint64_t v = polygon_suffix_xor(row[k]) ^ carry;
    row[k] = v;
    carry = (v & 1ull) ? ~0ull : 0ull;
  }
}

}  // namespace

}  // namespace tmh
