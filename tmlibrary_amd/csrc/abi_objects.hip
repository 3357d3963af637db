// C-ABI of libtmhip.so (include/tmhip.h): jterator object tables -- label
// range and the per-label integer sums of int32 label planes -- and the
// objects' outlines (extract_polygons' contours).
#include <climits>

#include "abi_internal.h"

namespace tmh {

void check_planes_args(const void* planes, int64_t n_planes, int height, int width) {
  TMH_CHECK(n_planes >= 0 && height > 0 && width > 0, TMH_EINVAL, "bad geometry");
  TMH_CHECK(n_planes <= 65535, TMH_EINVAL, "at most 65,535 label planes per call");
  TMH_CHECK(n_planes == 0 || planes, TMH_EINVAL, "planes pointer is NULL");
  TMH_CHECK((reinterpret_cast<uintptr_t>(planes) & 3) == 0, TMH_EINVAL,
            "label planes must be 4-byte aligned");
}

static void label_max_dev(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                          int32_t* dev_max, int32_t* dev_min, void* stream) {
  check_planes_args(dev_planes, n_planes, height, width);
  TMH_CHECK(n_planes == 0 || (dev_max && dev_min), TMH_EINVAL, "max or min pointer is NULL");
  launch_label_minmax(dev_planes, n_planes, (int64_t)height * width, dev_max, dev_min,
                      (hipStream_t)stream);
}

int32_t check_label_range(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                          int32_t max_label, hipStream_t s) {
  DBuf<int32_t> mm;
  mm.alloc((size_t)(2 * n_planes));
  launch_label_minmax(dev_planes, n_planes, (int64_t)height * width, mm.p, mm.p + n_planes, s);
  std::vector<int32_t> h((size_t)(2 * n_planes));
  TMH_HIP(hipMemcpyAsync(h.data(), mm.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  int32_t hi = INT_MIN, lo = INT_MAX;
  for (int64_t p = 0; p < n_planes; ++p) {
    hi = std::max(hi, h[(size_t)p]);
    lo = std::min(lo, h[(size_t)(n_planes + p)]);
  }
  TMH_CHECK(lo >= 0, TMH_EINVAL, "a label plane holds a negative label");
  TMH_CHECK(hi <= max_label, TMH_EINVAL, "a label plane holds a label above max_label");
  return hi;
}

static void object_table_dev(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                             int32_t max_label, tmh_object_row* dev_rows, void* stream,
                             bool range_known) {
  check_planes_args(dev_planes, n_planes, height, width);
  TMH_CHECK(max_label >= 0, TMH_EINVAL, "max_label is negative");
  TMH_CHECK(n_planes == 0 || dev_rows, TMH_EINVAL, "rows pointer is NULL");
  if (n_planes == 0) return;
  if (!range_known)
    check_label_range(dev_planes, n_planes, height, width, max_label, (hipStream_t)stream);
  launch_object_table(dev_planes, n_planes, height, width, max_label, dev_rows,
                      (hipStream_t)stream);
}

static int64_t contour_rows(int64_t n_planes, int32_t max_label) {
  const int64_t n_rows = n_planes * ((int64_t)max_label + 1);
  TMH_CHECK(n_rows <= INT_MAX, TMH_EINVAL, "at most 2^31 - 1 (plane, label) rows per call");
  return n_rows;
}

// the two-call contract of tmh_object_contours_device; the host form passes
// the capacity of its rows too (row_capacity < 0: none to check)
static void object_contours_dev(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                                int32_t max_label, const tmh_object_row* dev_rows,
                                tmh_contour_object* dev_objects, tmh_contour* dev_contours,
                                int64_t contour_capacity, int32_t* dev_points,
                                int64_t point_capacity, int64_t* n_contours, int64_t* n_points,
                                void* stream) {
  check_planes_args(dev_planes, n_planes, height, width);
  TMH_CHECK(max_label >= 0, TMH_EINVAL, "max_label is negative");
  TMH_CHECK(n_contours && n_points, TMH_EINVAL, "n_contours or n_points pointer is NULL");
  *n_contours = *n_points = 0;
  if (n_planes == 0) return;
  TMH_CHECK(dev_rows && dev_objects, TMH_EINVAL, "rows or objects pointer is NULL");
  TMH_CHECK((dev_contours == nullptr) == (dev_points == nullptr), TMH_EINVAL,
            "contours and points are given together or not at all");
  TMH_CHECK(contour_capacity >= 0 && point_capacity >= 0, TMH_EINVAL, "negative capacity");
  contour_rows(n_planes, max_label);
  ContourScratch scratch;
  contours_measure(dev_planes, n_planes, height, width, max_label, dev_rows, dev_objects, scratch,
                   n_contours, n_points, (hipStream_t)stream);
  if (!dev_contours) return;
  TMH_CHECK(contour_capacity >= *n_contours && point_capacity >= *n_points, TMH_EINVAL,
            "contour or point capacity smaller than *n_contours, *n_points");
  contours_write(dev_planes, height, width, max_label, dev_rows, dev_objects, scratch, dev_contours,
                 dev_points, (hipStream_t)stream);
}

}  // namespace tmh

extern "C" {

int tmh_label_max_device(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                         int32_t* dev_max, int32_t* dev_min, void* stream) {
  return guard(
      [&] { label_max_dev(dev_planes, n_planes, height, width, dev_max, dev_min, stream); });
}

int tmh_object_table_device(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                            int32_t max_label, tmh_object_row* dev_rows, void* stream) {
  return guard([&] {
    object_table_dev(dev_planes, n_planes, height, width, max_label, dev_rows, stream, false);
  });
}

int tmh_object_table(const int32_t* host_planes, int64_t n_planes, int height, int width,
                     int32_t* max_label, tmh_object_row* host_rows, int64_t row_capacity) {
  return guard([&] {
    check_planes_args(host_planes, n_planes, height, width);
    if (!has_label_planes(n_planes, max_label)) return;
    HostLabels a;
    const int32_t hi = a.upload(host_planes, n_planes, height, width, max_label);
    const int64_t n_rows = n_planes * ((int64_t)hi + 1);
    TMH_CHECK(host_rows && row_capacity >= n_rows, TMH_EINVAL,
              "row capacity smaller than n_planes * (*max_label + 1) rows");
    DBuf<tmh_object_row> rows;
    rows.alloc((size_t)n_rows);
    object_table_dev(a.dev.p, n_planes, height, width, hi, rows.p, nullptr, true);
    TMH_HIP(hipStreamSynchronize(nullptr));
    rows.download(host_rows, (size_t)n_rows);
  });
}

int tmh_object_contours_device(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                               int32_t max_label, const tmh_object_row* dev_rows,
                               tmh_contour_object* dev_objects, tmh_contour* dev_contours,
                               int64_t contour_capacity, int32_t* dev_points,
                               int64_t point_capacity, int64_t* n_contours, int64_t* n_points,
                               void* stream) {
  return guard([&] {
    object_contours_dev(dev_planes, n_planes, height, width, max_label, dev_rows, dev_objects,
                        dev_contours, contour_capacity, dev_points, point_capacity, n_contours,
                        n_points, stream);
  });
}

int tmh_object_contours(const int32_t* host_planes, int64_t n_planes, int height, int width,
                        int32_t* max_label, tmh_object_row* host_rows,
                        tmh_contour_object* host_objects, int64_t row_capacity,
                        tmh_contour* host_contours, int64_t contour_capacity,
                        int32_t* host_points, int64_t point_capacity, int64_t* n_contours,
                        int64_t* n_points) {
  return guard([&] {
    check_planes_args(host_planes, n_planes, height, width);
    TMH_CHECK(max_label && n_contours && n_points, TMH_EINVAL, "a count pointer is NULL");
    *max_label = 0;
    *n_contours = *n_points = 0;
    if (n_planes == 0) return;
    HostLabels a;
    const int32_t hi = a.upload(host_planes, n_planes, height, width, max_label);
    const int64_t n_rows = contour_rows(n_planes, hi);
    DBuf<tmh_object_row> rows;
    rows.alloc((size_t)n_rows);
    DBuf<tmh_contour_object> objects;
    objects.alloc((size_t)n_rows);
    object_table_dev(a.dev.p, n_planes, height, width, hi, rows.p, nullptr, true);
    // measure, check every capacity before anything is written, then fill
    object_contours_dev(a.dev.p, n_planes, height, width, hi, rows.p, objects.p, nullptr, 0,
                        nullptr, 0, n_contours, n_points, nullptr);
    TMH_CHECK(host_rows && host_objects && row_capacity >= n_rows, TMH_EINVAL,
              "row capacity smaller than n_planes * (*max_label + 1) rows");
    TMH_CHECK(contour_capacity >= *n_contours && point_capacity >= *n_points &&
                  (host_contours || *n_contours == 0) && (host_points || *n_points == 0),
              TMH_EINVAL, "contour or point capacity smaller than *n_contours, *n_points");
    DBuf<tmh_contour> contours;
    contours.alloc((size_t)std::max<int64_t>(*n_contours, 1));
    DBuf<int32_t> points;
    points.alloc((size_t)std::max<int64_t>(2 * *n_points, 2));
    int64_t nc = 0, np = 0;
    object_contours_dev(a.dev.p, n_planes, height, width, hi, rows.p, objects.p, contours.p,
                        *n_contours, points.p, *n_points, &nc, &np, nullptr);
    rows.download(host_rows, (size_t)n_rows);
    objects.download(host_objects, (size_t)n_rows);
    if (nc) contours.download(host_contours, (size_t)nc);
    if (np) points.download(host_points, (size_t)(2 * np));
  });
}

}  // extern "C"
