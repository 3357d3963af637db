// Object outlines of jterator's extract_polygons (tmlib/image.py:778-917): the
// opening by the 3x3 cross (mh.open's default structuring element) and Suzuki
// and Abe's border following (Algorithm 1, what cv2.findContours runs with
// RETR_CCOMP and CHAIN_APPROX_NONE) on one object's padded bounding-box mask.
// Kept free of HIP headers so that the code k_contours_lds and k_contours_big run
// (contour_kernels.hip) also builds for the host (tests/contour_host.cpp).
// DESIGN.md section 21.
//
// A mask is h rows of wpr = ceil(w / 64) words, pixel x of a row in bit x % 64
// of word x / 64; bits at x >= w are zero.  Row 0, row h - 1, column 0 and
// column w - 1 hold no set pixel (the reference's one-pixel pad), so no
// neighbour of a set pixel lies outside the array.
#pragma once

#include <cstdint>

#ifndef TMH_CHD
#define TMH_CHD __host__ __device__ __forceinline__
#endif

namespace tmh {

namespace {

TMH_CHD int contour_wpr(int w) { return (w + 63) >> 6; }

TMH_CHD uint64_t contour_word(const uint64_t* m, int h, int wpr, int y, int k) {
  return (y < 0 || y >= h || k < 0 || k >= wpr) ? 0ull : m[(int64_t)y * wpr + k];
}

TMH_CHD int contour_bit(const uint64_t* m, int wpr, int y, int x) {
  return (int)((m[(int64_t)y * wpr + (x >> 6)] >> (x & 63)) & 1ull);
}

// Word k of row y after an erosion (erode) or a dilation by the cross: the
// word combined with its two row neighbours and with itself shifted one pixel
// either way, the shifts carrying across word boundaries.  Outside the array
// is zero; the pad keeps that from ever showing.
TMH_CHD uint64_t contour_cross_word(const uint64_t* m, int h, int wpr, int y, int k, bool erode) {
  const uint64_t c = contour_word(m, h, wpr, y, k);
  const uint64_t west = (c << 1) | (contour_word(m, h, wpr, y, k - 1) >> 63);
  const uint64_t east = (c >> 1) | (contour_word(m, h, wpr, y, k + 1) << 63);
  const uint64_t north = contour_word(m, h, wpr, y - 1, k);
  const uint64_t south = contour_word(m, h, wpr, y + 1, k);
  return erode ? (c & west & east & north & south) : (c | west | east | north | south);
}

// Directions in counter-clockwise order with y pointing down:
// 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE.  Clockwise is the index falling.
TMH_CHD int contour_dx(int d) { return (int)((0x21000122u >> (4 * d)) & 3u) - 1; }
TMH_CHD int contour_dy(int d) { return (int)((0x22210001u >> (4 * d)) & 3u) - 1; }

// Pixels x - 1, x, x + 1 of a row (bit 0: x - 1), 1 <= x <= w - 2.
TMH_CHD unsigned contour_bits3(const uint64_t* row, int x) {
  const int k = (x - 1) >> 6, s = (x - 1) & 63;
  uint64_t v = row[k] >> s;
  if (s > 61) v |= row[k + 1] << (64 - s);  // x + 1 <= w - 1 lies in the row, so word k + 1 does
  return (unsigned)(v & 7ull);
}

// The eight neighbours of set pixel (x, y), bit d = direction d: three row
// reads that do not wait for each other, where a probe per neighbour would.
TMH_CHD unsigned contour_neighbours(const uint64_t* mask, int wpr, int y, int x) {
  const unsigned n = contour_bits3(mask + (int64_t)(y - 1) * wpr, x);
  const unsigned m = contour_bits3(mask + (int64_t)y * wpr, x);
  const unsigned s = contour_bits3(mask + (int64_t)(y + 1) * wpr, x);
  return ((m >> 2) & 1u) | (((n >> 2) & 1u) << 1) | (((n >> 1) & 1u) << 2) | ((n & 1u) << 3) |
         ((m & 1u) << 4) | ((s & 1u) << 5) | (((s >> 1) & 1u) << 6) | (((s >> 2) & 1u) << 7);
}

// Border following over `mask` with one mark per pixel (zeroed by the caller):
// 0 is Suzuki's f = 1 (not yet on a border), +-(b + 1) his +-NBD of border b,
// borders numbered from 0 in the order the raster scan finds them.  M holds
// the number of borders the mask can have (at most half its pixels).
//
// sink.begin(is_hole, lnbd) opens border b = 0, 1, ...: lnbd is the border
// last met on this row (Suzuki's LNBD, -1 for the frame), from which the sink
// takes the parent.  sink.point(x, y) is every pixel of the border in tracing
// order, sink.end() closes it.
//
// The raster scan only stops at pixels with a zero to their left or right, a
// word at a time.  LNBD is looked up when a hole border starts: it is the mark
// of the nearest marked pixel to the left, which is what a scan carrying it
// along would hold -- marks are never cleared, and a trace that marks pixels
// behind the scan starts at a pixel the scan then passes as marked.
template <class M, class Sink>
TMH_CHD void contour_follow(const uint64_t* mask, M* marks, int h, int w, int wpr, Sink& sink) {
  int nbd = 0;
  for (int y = 1; y < h - 1; ++y) {
    const uint64_t* row = mask + (int64_t)y * wpr;
    M* mrow = marks + (int64_t)y * w;
    for (int k = 0; k < wpr; ++k) {
      const uint64_t c = row[k];
      if (!c) continue;
      const uint64_t west = (c << 1) | (k ? row[k - 1] >> 63 : 0ull);
      const uint64_t east = (c >> 1) | (k + 1 < wpr ? row[k + 1] << 63 : 0ull);
      uint64_t cand = c & ~(west & east);
      while (cand) {
        const int b = __builtin_ctzll(cand);
        cand &= cand - 1;
        const int x = k * 64 + b;
        const int f = (int)mrow[x];
        bool hole;
        if (f == 0 && !((west >> b) & 1ull)) {
          hole = false;  // f == 1 and a zero to the left: an outer border
        } else if (f >= 0 && !((east >> b) & 1ull)) {
          hole = true;   // f >= 1 and a zero to the right: a hole border
        } else {
          continue;
        }
        int lnbd = -1;
        if (hole) {
          if (f > 0) {
            lnbd = f - 1;
          } else {
            for (int xx = x - 1; xx >= 0; --xx) {
              const int g = (int)mrow[xx];
              if (g != 0) {
                lnbd = (g < 0 ? -g : g) - 1;
                break;
              }
            }
          }
        }
        const int id = nbd++;
        sink.begin(hole ? 1 : 0, lnbd);
        // the first search runs clockwise from the left (outer) or right (hole) neighbour
        const int d0 = hole ? 0 : 4;
        const unsigned nb0 = contour_neighbours(mask, wpr, y, x);
        int d1 = -1;
        for (int t = 0; t < 8; ++t) {
          const int d = (d0 - t) & 7;
          if ((nb0 >> d) & 1u) {
            d1 = d;
            break;
          }
        }
        if (d1 < 0) {  // no neighbour: one point
          mrow[x] = (M)(-(id + 1));
          sink.point(x, y);
          sink.end();
          continue;
        }
        const int x1 = x + contour_dx(d1), y1 = y + contour_dy(d1);
        int cx = x, cy = y, dp = d1;  // the current pixel and the direction of the one before it
        for (;;) {
          // counter-clockwise from direction s, one past the pixel just left
          // (which itself ends the search at the latest): the neighbours
          // rotated so that s is bit 0, the first set bit t steps on.  East is
          // looked at after (0 - s) & 7 steps: examined and zero if before t.
          const unsigned nb = contour_neighbours(mask, wpr, cy, cx);
          const int s = (dp + 1) & 7;
          const unsigned rot = ((nb >> s) | (nb << (8 - s))) & 0xffu;
          const int t = __builtin_ctz(rot);
          const int dn = (s + t) & 7;
          const bool east_zero = ((8 - s) & 7) < t;
          M* cm = marks + (int64_t)cy * w + cx;
          if (east_zero) {
            *cm = (M)(-(id + 1));
          } else if (*cm == 0) {
            *cm = (M)(id + 1);
          }
          sink.point(cx, cy);
          const int nx = cx + contour_dx(dn), ny = cy + contour_dy(dn);
          if (nx == x && ny == y && cx == x1 && cy == y1) break;
          dp = (dn + 4) & 7;
          cx = nx;
          cy = ny;
        }
        sink.end();
      }
    }
  }
}

// RETR_CCOMP's parent of a new border from LNBD: an outer border has none;
// a hole's is LNBD when that is an outer border, else LNBD's own parent
// (Suzuki's table 1, two levels).
TMH_CHD int contour_parent(int is_hole, int lnbd, int lnbd_is_hole, int lnbd_parent) {
  if (!is_hole || lnbd < 0) return -1;
  return lnbd_is_hole ? lnbd_parent : lnbd;
}

}  // namespace

}  // namespace tmh
