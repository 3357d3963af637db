// C-ABI of libtmhip.so (include/tmhip.h): jterator object tables -- label
// range and the per-label integer sums of int32 label planes.
#include <climits>

#include "abi_internal.h"

namespace tmh {

static void check_planes_args(const void* planes, int64_t n_planes, int height, int width) {
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

// the largest and smallest label of all planes, on the host (waits for them)
static void label_range(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                        hipStream_t s, int32_t* hi, int32_t* lo) {
  DBuf<int32_t> mm;
  mm.alloc((size_t)(2 * n_planes));
  launch_label_minmax(dev_planes, n_planes, (int64_t)height * width, mm.p, mm.p + n_planes, s);
  std::vector<int32_t> h((size_t)(2 * n_planes));
  TMH_HIP(hipMemcpyAsync(h.data(), mm.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  *hi = INT_MIN;
  *lo = INT_MAX;
  for (int64_t p = 0; p < n_planes; ++p) {
    *hi = std::max(*hi, h[(size_t)p]);
    *lo = std::min(*lo, h[(size_t)(n_planes + p)]);
  }
}

static void object_table_dev(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                             int32_t max_label, tmh_object_row* dev_rows, void* stream,
                             bool range_known) {
  check_planes_args(dev_planes, n_planes, height, width);
  TMH_CHECK(max_label >= 0, TMH_EINVAL, "max_label is negative");
  TMH_CHECK(n_planes == 0 || dev_rows, TMH_EINVAL, "rows pointer is NULL");
  if (n_planes == 0) return;
  if (!range_known) {
    int32_t hi, lo;
    label_range(dev_planes, n_planes, height, width, (hipStream_t)stream, &hi, &lo);
    TMH_CHECK(lo >= 0, TMH_EINVAL, "a label plane holds a negative label");
    TMH_CHECK(hi <= max_label, TMH_EINVAL, "a label plane holds a label above max_label");
  }
  launch_object_table(dev_planes, n_planes, height, width, max_label, dev_rows,
                      (hipStream_t)stream);
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
    TMH_CHECK(max_label, TMH_EINVAL, "max_label pointer is NULL");
    *max_label = 0;
    if (n_planes == 0) return;
    DBuf<int32_t> a;
    a.upload(host_planes, (size_t)n_planes * height * width);
    int32_t hi, lo;
    label_range(a.p, n_planes, height, width, nullptr, &hi, &lo);
    TMH_CHECK(lo >= 0, TMH_EINVAL, "a label plane holds a negative label");
    *max_label = hi;
    const int64_t n_rows = n_planes * ((int64_t)hi + 1);
    TMH_CHECK(host_rows && row_capacity >= n_rows, TMH_EINVAL,
              "row capacity smaller than n_planes * (*max_label + 1) rows");
    DBuf<tmh_object_row> rows;
    rows.alloc((size_t)n_rows);
    object_table_dev(a.p, n_planes, height, width, hi, rows.p, nullptr, true);
    TMH_HIP(hipStreamSynchronize(nullptr));
    rows.download(host_rows, (size_t)n_rows);
  });
}

}  // extern "C"
