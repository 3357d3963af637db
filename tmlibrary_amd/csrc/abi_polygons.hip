// C-ABI of libtmhip.so (include/tmhip.h): jterator object input -- label
// planes from stored outlines (create_from_polygons for all planes of a site).
#include <climits>

#include "abi_internal.h"

namespace tmh {

static void check_polygon_args(const void* points, const void* first, const void* plane,
                               const void* label, int64_t n_polygons, int64_t n_planes, int height,
                               int width, const void* out) {
  TMH_CHECK(n_polygons >= 0 && n_planes >= 0 && height > 0 && width > 0, TMH_EINVAL,
            "bad geometry");
  TMH_CHECK(n_planes <= 65535, TMH_EINVAL, "at most 65,535 label planes per call");
  TMH_CHECK(n_polygons < INT_MAX, TMH_EINVAL, "at most 2^31 - 2 rings per call");
  TMH_CHECK(n_planes == 0 || out, TMH_EINVAL, "planes_out pointer is NULL");
  TMH_CHECK(n_polygons == 0 || (points && first && plane && label), TMH_EINVAL,
            "points, first, plane or label pointer is NULL");
  TMH_CHECK(n_polygons == 0 || n_planes > 0, TMH_EINVAL, "a plane index out of range");
  TMH_CHECK(((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(plane) |
              reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(out)) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(first) & 7) == 0,
            TMH_EINVAL, "the lists and planes_out must be aligned to their elements");
}

static void check_polygon_overlap(const void* points, const void* first, const void* plane,
                                  const void* label, int64_t n_polygons, int64_t n_points,
                                  const void* out, size_t out_bytes) {
  const size_t n = (size_t)n_polygons;
  TMH_CHECK(!overlap(out, out_bytes, points, (size_t)n_points * 8) &&
                !overlap(out, out_bytes, first, (n + 1) * 8) &&
                !overlap(out, out_bytes, plane, n * 4) && !overlap(out, out_bytes, label, n * 4),
            TMH_EINVAL, "planes_out overlaps an input");
}

static void polygon_fill_dev(const int32_t* dev_points, const int64_t* dev_first,
                             const int32_t* dev_plane, const int32_t* dev_label, int64_t n_polygons,
                             int64_t n_planes, int height, int width, int64_t y_offset,
                             int64_t x_offset, int32_t* dev_out, hipStream_t s) {
  check_polygon_args(dev_points, dev_first, dev_plane, dev_label, n_polygons, n_planes, height,
                     width, dev_out);
  if (n_planes == 0) return;
  DBuf<char> check;
  if (n_polygons > 0) {
    check.alloc((size_t)polygons_check_bytes());
    int64_t n_points = 0;
    polygons_check(dev_points, dev_first, dev_plane, n_polygons, n_planes, y_offset, x_offset,
                   check.p, &n_points, s);
    check_polygon_overlap(dev_points, dev_first, dev_plane, dev_label, n_polygons, n_points,
                          dev_out, (size_t)n_planes * height * width * 4);
  }
  polygons_fill(dev_points, dev_first, dev_plane, dev_label, n_polygons, n_planes, height, width,
                y_offset, x_offset, dev_out, check.p, s);
}

}  // namespace tmh

extern "C" {

int tmh_polygon_fill_device(const int32_t* dev_points, const int64_t* dev_first,
                            const int32_t* dev_plane, const int32_t* dev_label,
                            int64_t n_polygons, int64_t n_planes, int height, int width,
                            int64_t y_offset, int64_t x_offset, int32_t* dev_planes_out,
                            void* stream) {
  return guard([&] {
    polygon_fill_dev(dev_points, dev_first, dev_plane, dev_label, n_polygons, n_planes, height,
                     width, y_offset, x_offset, dev_planes_out, (hipStream_t)stream);
  });
}

int tmh_polygon_fill(const int32_t* host_points, const int64_t* host_first,
                     const int32_t* host_plane, const int32_t* host_label, int64_t n_polygons,
                     int64_t n_planes, int height, int width, int64_t y_offset, int64_t x_offset,
                     int32_t* host_planes_out) {
  return guard([&] {
    check_polygon_args(host_points, host_first, host_plane, host_label, n_polygons, n_planes,
                       height, width, host_planes_out);
    if (n_planes == 0) return;
    const size_t total = (size_t)n_planes * height * width;
    DBuf<int32_t> points, plane, label, out;
    DBuf<int64_t> first;
    if (n_polygons > 0) {
      // the extent of the points comes from first: it has to be sound before it is used
      TMH_CHECK(host_first[0] >= 0, TMH_EINVAL, "first is not monotone from a start >= 0");
      for (int64_t p = 0; p < n_polygons; ++p)
        TMH_CHECK(host_first[p + 1] >= host_first[p], TMH_EINVAL,
                  "first is not monotone from a start >= 0");
      for (int64_t p = 0; p < n_polygons; ++p)
        TMH_CHECK(host_first[p + 1] > host_first[p], TMH_EINVAL, "an empty ring");
      const int64_t n_points = host_first[n_polygons];
      check_polygon_overlap(host_points, host_first, host_plane, host_label, n_polygons, n_points,
                            host_planes_out, total * 4);
      points.upload(host_points, (size_t)(2 * n_points));
      first.upload(host_first, (size_t)n_polygons + 1);
      plane.upload(host_plane, (size_t)n_polygons);
      label.upload(host_label, (size_t)n_polygons);
    }
    out.alloc(total);
    polygon_fill_dev(points.p, first.p, plane.p, label.p, n_polygons, n_planes, height, width,
                     y_offset, x_offset, out.p, nullptr);
    out.download(host_planes_out, total);
  });
}

}  // extern "C"
