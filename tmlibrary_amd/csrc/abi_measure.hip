// C-ABI of libtmhip.so (include/tmhip.h): jterator intensity measurements --
// the per-label integer rows of intensity planes under int32 label planes and
// the five features taken from them.
#include <climits>

#include "abi_internal.h"

namespace tmh {

static int64_t intensity_rows(int64_t n_planes, int32_t max_label, int n_channels) {
  const int64_t n_rows = n_planes * ((int64_t)max_label + 1) * n_channels;
  TMH_CHECK(n_rows <= INT_MAX, TMH_EINVAL,
            "at most 2^31 - 1 (plane, label, channel) rows per call");
  return n_rows;
}

static void check_channels(int n_channels) {
  TMH_CHECK(n_channels >= 1 && n_channels <= TMH_INTENSITY_MAX_CHANNELS, TMH_EINVAL,
            "n_channels must be 1..16");
}

static void intensity_table_dev(const int32_t* dev_labels, const void* dev_pixels, int elem_bytes,
                                int64_t n_planes, int height, int width, int n_channels,
                                int64_t cs, int64_t ps, int64_t rs, int64_t xs, int32_t max_label,
                                bool range_known, tmh_intensity_row* dev_rows, void* stream) {
  check_planes_args(dev_labels, n_planes, height, width);
  check_channels(n_channels);
  TMH_CHECK(elem_bytes == 1 || elem_bytes == 2, TMH_EINVAL,
            "elem_bytes must be 1 (uint8) or 2 (uint16): float and int32 images are not measured");
  TMH_CHECK(cs >= 0 && ps >= 0 && rs >= 0 && xs >= 0, TMH_EINVAL, "a stride is negative");
  TMH_CHECK(max_label >= 0, TMH_EINVAL, "max_label is negative");
  if (n_planes == 0) return;
  TMH_CHECK(dev_pixels && dev_rows, TMH_EINVAL, "pixels or rows pointer is NULL");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_pixels) & (uintptr_t)(elem_bytes - 1)) == 0,
            TMH_EINVAL, "pixels must be aligned to elem_bytes");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_rows) & 7) == 0, TMH_EINVAL,
            "rows must be 8-byte aligned");
  const int64_t n_rows = intensity_rows(n_planes, max_label, n_channels);
  // the last element the strides reach
  const int64_t reach = (n_channels - 1) * cs + (n_planes - 1) * ps + (int64_t)(height - 1) * rs +
                        (int64_t)(width - 1) * xs + 1;
  const size_t row_bytes = (size_t)n_rows * sizeof(tmh_intensity_row);
  TMH_CHECK(!overlap(dev_rows, row_bytes, dev_pixels, (size_t)reach * elem_bytes) &&
                !overlap(dev_rows, row_bytes, dev_labels,
                         (size_t)n_planes * height * width * sizeof(int32_t)),
            TMH_EINVAL, "dev_rows overlaps an input");
  if (!range_known)
    check_label_range(dev_labels, n_planes, height, width, max_label, (hipStream_t)stream);
  launch_intensity_table(dev_labels, dev_pixels, elem_bytes, n_planes, height, width, n_channels,
                         cs, ps, rs, xs, max_label, dev_rows, (hipStream_t)stream);
}

static void intensity_features_dev(const tmh_intensity_row* dev_rows, int64_t n_planes,
                                   int64_t n_groups, int32_t max_label, int n_channels,
                                   double* dev_features, void* stream) {
  TMH_CHECK(n_planes >= 0 && n_groups >= 0, TMH_EINVAL, "bad geometry");
  TMH_CHECK(n_planes <= 65535, TMH_EINVAL, "at most 65,535 label planes per call");
  check_channels(n_channels);
  TMH_CHECK(max_label >= 0, TMH_EINVAL, "max_label is negative");
  TMH_CHECK((n_groups == 0) == (n_planes == 0) && (n_groups == 0 || n_planes % n_groups == 0),
            TMH_EINVAL, "n_groups must divide n_planes");
  if (n_planes == 0) return;
  TMH_CHECK(dev_rows && dev_features, TMH_EINVAL, "rows or features pointer is NULL");
  const int64_t n_rows = intensity_rows(n_planes, max_label, n_channels);
  TMH_CHECK(!overlap(dev_rows, (size_t)n_rows * sizeof(tmh_intensity_row), dev_features,
                     (size_t)(n_rows / (n_planes / n_groups)) * 5 * sizeof(double)),
            TMH_EINVAL, "dev_features overlaps dev_rows");
  launch_intensity_features(dev_rows, n_planes, n_groups, max_label, n_channels, dev_features,
                            (hipStream_t)stream);
}

}  // namespace tmh

extern "C" {

int tmh_intensity_table_device(const int32_t* dev_labels, const void* dev_pixels, int elem_bytes,
                               int64_t n_planes, int height, int width, int n_channels,
                               int64_t channel_stride, int64_t plane_stride, int64_t row_stride,
                               int64_t pix_stride, int32_t max_label,
                               const tmh_object_row* dev_object_rows, tmh_intensity_row* dev_rows,
                               void* stream) {
  return guard([&] {
    intensity_table_dev(dev_labels, dev_pixels, elem_bytes, n_planes, height, width, n_channels,
                        channel_stride, plane_stride, row_stride, pix_stride, max_label,
                        dev_object_rows != nullptr, dev_rows, stream);
  });
}

int tmh_intensity_features_device(const tmh_intensity_row* dev_rows, int64_t n_planes,
                                  int64_t n_groups, int32_t max_label, int n_channels,
                                  double* dev_features, void* stream) {
  return guard([&] {
    intensity_features_dev(dev_rows, n_planes, n_groups, max_label, n_channels, dev_features,
                           stream);
  });
}

int tmh_intensity_table(const int32_t* host_labels, const void* host_pixels, int elem_bytes,
                        int64_t n_planes, int height, int width, int n_channels,
                        int32_t* max_label, tmh_intensity_row* host_rows, int64_t row_capacity) {
  return guard([&] {
    check_planes_args(host_labels, n_planes, height, width);
    check_channels(n_channels);
    TMH_CHECK(elem_bytes == 1 || elem_bytes == 2, TMH_EINVAL,
              "elem_bytes must be 1 (uint8) or 2 (uint16): float and int32 images are not measured");
    if (!has_label_planes(n_planes, max_label)) return;
    TMH_CHECK(host_pixels, TMH_EINVAL, "pixels pointer is NULL");
    const int64_t npx = (int64_t)height * width;
    HostLabels labels;
    const int32_t hi = labels.upload(host_labels, n_planes, height, width, max_label);
    const int64_t n_rows = intensity_rows(n_planes, hi, n_channels);
    TMH_CHECK(host_rows && row_capacity >= n_rows, TMH_EINVAL,
              "row capacity smaller than n_planes * (*max_label + 1) * n_channels rows");
    DBuf<uint8_t> pixels;
    pixels.upload(host_pixels, (size_t)(n_channels * n_planes * npx * elem_bytes));
    DBuf<tmh_intensity_row> rows;
    rows.alloc((size_t)n_rows);
    intensity_table_dev(labels.dev.p, pixels.p, elem_bytes, n_planes, height, width, n_channels,
                        n_planes * npx, npx, width, 1, hi, true, rows.p, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    rows.download(host_rows, (size_t)n_rows);
  });
}

int tmh_intensity_features(const tmh_intensity_row* host_rows, int64_t n_planes, int64_t n_groups,
                           int32_t max_label, int n_channels, double* host_features) {
  return guard([&] {
    TMH_CHECK(n_planes == 0 || (host_rows && host_features), TMH_EINVAL,
              "rows or features pointer is NULL");
    TMH_CHECK(n_planes >= 0 && n_planes <= 65535 && max_label >= 0, TMH_EINVAL, "bad geometry");
    check_channels(n_channels);
    TMH_CHECK(n_planes == 0 || (n_groups > 0 && n_planes % n_groups == 0), TMH_EINVAL,
              "n_groups must divide n_planes");
    if (n_planes == 0) return;
    const int64_t n_rows = intensity_rows(n_planes, max_label, n_channels);
    const int64_t n_out = n_rows / (n_planes / n_groups) * 5;
    DBuf<tmh_intensity_row> rows;
    rows.upload(host_rows, (size_t)n_rows);
    DBuf<double> out;
    out.alloc((size_t)n_out);
    intensity_features_dev(rows.p, n_planes, n_groups, max_label, n_channels, out.p, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    out.download(host_features, (size_t)n_out);
  });
}

}  // extern "C"
