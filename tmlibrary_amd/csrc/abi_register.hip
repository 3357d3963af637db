// C-ABI of libtmhip.so (include/tmhip.h): registration (the align step) and the xcorr plane.
#include "abi_internal.h"

namespace tmh {

static void check_register_args(const void* targets, int64_t n, const void* refs, int64_t m,
                                int height, int width, int elem_bytes, const int32_t* ref_of,
                                const int32_t* y, const int32_t* x) {
  TMH_CHECK(n >= 0 && m >= 0 && n < (int64_t(1) << 31) && m < (int64_t(1) << 31), TMH_EINVAL,
            "target and reference counts must be in 0..2^31-1");
  TMH_CHECK(elem_bytes == 1 || elem_bytes == 2, TMH_EINVAL, "elem_bytes must be 1 or 2");
  TMH_CHECK(height >= 1 && width >= 1, TMH_EINVAL, "height and width must be at least 1");
  TMH_CHECK(n == 0 || (targets && refs && ref_of && y && x), TMH_EINVAL,
            "targets, references, ref_of_target, y or x pointer is NULL");
  TMH_CHECK(n == 0 || m > 0, TMH_EINVAL, "targets without references");
}

static void register_shifts_dev(const void* dev_targets, int64_t n, const void* dev_refs, int64_t m,
                                int height, int width, int elem_bytes,
                                const int32_t* host_ref_of_target, void* dev_scratch,
                                int64_t scratch_bytes, int32_t* host_y, int32_t* host_x,
                                float* host_peak, void* stream) {
  check_register_args(dev_targets, n, dev_refs, m, height, width, elem_bytes, host_ref_of_target,
                      host_y, host_x);
  (void)register_scratch_bytes(n, m, height, width);  // the line limit, before anything else
  if (n == 0) return;
  TMH_CHECK(dev_scratch, TMH_EINVAL, "scratch pointer is NULL");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_scratch) & 255) == 0 &&
                ((reinterpret_cast<uintptr_t>(dev_targets) | reinterpret_cast<uintptr_t>(dev_refs)) &
                 (uintptr_t)(elem_bytes - 1)) == 0,
            TMH_EINVAL, "scratch must be 256-byte aligned, images aligned to their element");
  launch_register(dev_targets, n, dev_refs, m, height, width, elem_bytes, host_ref_of_target,
                  dev_scratch, scratch_bytes, host_y, host_x, host_peak, nullptr,
                  (hipStream_t)stream);
}

static void xcorr_plane_dev(const void* dev_target, const void* dev_ref, int height, int width,
                            int elem_bytes, void* dev_scratch, int64_t scratch_bytes,
                            float* dev_plane, void* stream) {
  TMH_CHECK(elem_bytes == 1 || elem_bytes == 2, TMH_EINVAL, "elem_bytes must be 1 or 2");
  TMH_CHECK(dev_target && dev_ref && dev_scratch && dev_plane, TMH_EINVAL,
            "target, reference, scratch or plane pointer is NULL");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_scratch) & 255) == 0 &&
                (reinterpret_cast<uintptr_t>(dev_plane) & 3) == 0 &&
                ((reinterpret_cast<uintptr_t>(dev_target) | reinterpret_cast<uintptr_t>(dev_ref)) &
                 (uintptr_t)(elem_bytes - 1)) == 0,
            TMH_EINVAL,
            "scratch must be 256-byte, the plane 4-byte aligned, images aligned to their element");
  const int32_t ref_of = 0;
  int32_t y = 0, x = 0;
  launch_register(dev_target, 1, dev_ref, 1, height, width, elem_bytes, &ref_of, dev_scratch,
                  scratch_bytes, &y, &x, nullptr, dev_plane, (hipStream_t)stream);
}

}  // namespace tmh

extern "C" {

int64_t tmh_register_scratch_bytes(int64_t n, int64_t m, int height, int width) {
  int64_t bytes = 0;
  const int rc = guard([&] {
    TMH_CHECK(n >= 0 && m >= 0 && n < (int64_t(1) << 31) && m < (int64_t(1) << 31), TMH_EINVAL,
              "target and reference counts must be in 0..2^31-1");
    bytes = register_scratch_bytes(n, m, height, width);
  });
  return rc ? rc : bytes;
}

int tmh_register_shifts_device(const void* dev_targets, int64_t n, const void* dev_refs, int64_t m,
                               int height, int width, int elem_bytes,
                               const int32_t* host_ref_of_target, void* dev_scratch,
                               int64_t scratch_bytes, int32_t* host_y, int32_t* host_x,
                               float* host_peak, void* stream) {
  return guard([&] {
    register_shifts_dev(dev_targets, n, dev_refs, m, height, width, elem_bytes, host_ref_of_target,
                        dev_scratch, scratch_bytes, host_y, host_x, host_peak, stream);
  });
}

int tmh_register_shifts(const void* host_targets, int64_t n, const void* host_refs, int64_t m,
                        int height, int width, int elem_bytes, const int32_t* ref_of_target,
                        int32_t* y, int32_t* x, float* peak) {
  return guard([&] {
    check_register_args(host_targets, n, host_refs, m, height, width, elem_bytes, ref_of_target, y,
                        x);
    const int64_t sb = register_scratch_bytes(n, m, height, width);
    if (n == 0) return;
    const size_t img = (size_t)height * width * elem_bytes;
    DBuf<uint8_t> t, r, scratch;
    t.upload(host_targets, (size_t)n * img);
    r.upload(host_refs, (size_t)m * img);
    scratch.alloc((size_t)sb);
    register_shifts_dev(t.p, n, r.p, m, height, width, elem_bytes, ref_of_target, scratch.p, sb,
                        y, x, peak, nullptr);
  });
}

int tmh_xcorr_plane_device(const void* dev_target, const void* dev_ref, int height, int width,
                           int elem_bytes, void* dev_scratch, int64_t scratch_bytes,
                           float* dev_plane, void* stream) {
  return guard([&] {
    xcorr_plane_dev(dev_target, dev_ref, height, width, elem_bytes, dev_scratch, scratch_bytes,
                    dev_plane, stream);
  });
}

int tmh_xcorr_plane(const void* host_target, const void* host_ref, int height, int width,
                    int elem_bytes, float* host_plane) {
  return guard([&] {
    TMH_CHECK(elem_bytes == 1 || elem_bytes == 2, TMH_EINVAL, "elem_bytes must be 1 or 2");
    TMH_CHECK(host_target && host_ref && host_plane, TMH_EINVAL,
              "target, reference or plane pointer is NULL");
    const int64_t sb = register_scratch_bytes(1, 1, height, width);
    const size_t px = (size_t)height * width;
    DBuf<uint8_t> t, r, scratch;
    DBuf<float> plane;
    t.upload(host_target, px * elem_bytes);
    r.upload(host_ref, px * elem_bytes);
    scratch.alloc((size_t)sb);
    plane.alloc(px);
    xcorr_plane_dev(t.p, r.p, height, width, elem_bytes, scratch.p, sb, plane.p, nullptr);
    plane.download(host_plane, px);
  });
}

}  // extern "C"
