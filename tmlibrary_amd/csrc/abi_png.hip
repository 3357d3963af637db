// C-ABI of libtmhip.so (include/tmhip.h): channel images as PNG files.
#include "abi_internal.h"

namespace tmh {

static void check_png_geometry(int64_t n_images, int height, int width, int elem_bytes) {
  TMH_CHECK(elem_bytes == 1 || elem_bytes == 2, TMH_EINVAL, "elem_bytes must be 1 or 2");
  TMH_CHECK(n_images >= 0 && height > 0 && width > 0, TMH_EINVAL,
            "n_images must not be negative, height and width must be positive");
  // PNG's own limit is 2^31 - 1 per side; the row and piece indices are 32-bit
  TMH_CHECK((int64_t)height <= 2147483647 && (int64_t)width <= 2147483647 &&
                (int64_t)height * width <= (int64_t(1) << 40),
            TMH_EINVAL, "height or width above 2^31 - 1, or more than 2^40 pixels");
  const int64_t pieces =
      cdiv((int64_t)height * (1 + (int64_t)width * elem_bytes), png_piece_bytes());
  TMH_CHECK(n_images < (int64_t(1) << 31) && n_images * height / 4 < (int64_t(1) << 31) &&
                n_images * pieces < (int64_t(1) << 31),
            TMH_EINVAL, "more than 2^31-1 workgroups of rows or pieces in one call");
}

static void png_encode_dev(const void* dev_images, int64_t n_images, int height, int width,
                           int elem_bytes, uint8_t* dev_dst, int64_t dst_bytes, int64_t* dev_offsets,
                           void* dev_scratch, int64_t scratch_bytes, void* stream) {
  check_png_geometry(n_images, height, width, elem_bytes);
  TMH_CHECK(dev_offsets, TMH_EINVAL, "offsets pointer is NULL");
  if (n_images == 0) {
    TMH_HIP(hipMemsetAsync(dev_offsets, 0, sizeof(int64_t), (hipStream_t)stream));
    return;
  }
  TMH_CHECK(dev_images && dev_dst && dev_scratch, TMH_EINVAL,
            "images, destination or scratch pointer is NULL");
  const int64_t need = n_images * png_bound_bytes(height, width, elem_bytes);
  TMH_CHECK(dst_bytes >= need, TMH_EINVAL,
            "dst_bytes smaller than n_images * tmh_png_bound(height, width, elem_bytes)");
  TMH_CHECK(scratch_bytes >= png_scratch_bytes(n_images, height, width, elem_bytes), TMH_EINVAL,
            "scratch_bytes smaller than tmh_png_scratch_bytes");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_scratch) & 15) == 0, TMH_EINVAL,
            "scratch must be 16-byte aligned");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_images) & (uintptr_t)(elem_bytes - 1)) == 0, TMH_EINVAL,
            "images must be aligned to their element");
  const size_t src_bytes = (size_t)n_images * height * width * elem_bytes;
  TMH_CHECK(!overlap(dev_images, src_bytes, dev_dst, (size_t)dst_bytes) &&
                !overlap(dev_images, src_bytes, dev_scratch, (size_t)scratch_bytes) &&
                !overlap(dev_dst, (size_t)dst_bytes, dev_scratch, (size_t)scratch_bytes) &&
                !overlap(dev_offsets, (size_t)(n_images + 1) * 8, dev_dst, (size_t)dst_bytes),
            TMH_EINVAL, "images, destination, offsets and scratch must not overlap");
  launch_png(static_cast<const uint8_t*>(dev_images), n_images, height, width, elem_bytes, dev_dst,
             dev_offsets, static_cast<uint8_t*>(dev_scratch), (hipStream_t)stream);
}

}  // namespace tmh

extern "C" {

int64_t tmh_png_piece_bytes(void) { return png_piece_bytes(); }

int64_t tmh_png_bound(int height, int width, int elem_bytes) {
  return height > 0 && width > 0 && (elem_bytes == 1 || elem_bytes == 2)
             ? png_bound_bytes(height, width, elem_bytes)
             : 0;
}

int64_t tmh_png_scratch_bytes(int64_t n_images, int height, int width, int elem_bytes) {
  return n_images > 0 && height > 0 && width > 0 && (elem_bytes == 1 || elem_bytes == 2)
             ? png_scratch_bytes(n_images, height, width, elem_bytes)
             : 0;
}

int tmh_png_encode_device(const void* dev_images, int64_t n_images, int height, int width,
                          int elem_bytes, uint8_t* dev_dst, int64_t dst_bytes, int64_t* dev_offsets,
                          void* dev_scratch, int64_t scratch_bytes, void* stream) {
  return guard([&] {
    png_encode_dev(dev_images, n_images, height, width, elem_bytes, dev_dst, dst_bytes, dev_offsets,
                   dev_scratch, scratch_bytes, stream);
  });
}

int tmh_png_encode(const void* host_images, int64_t n_images, int height, int width, int elem_bytes,
                   uint8_t* host_blob, int64_t blob_capacity, int64_t* host_offsets, int64_t* total) {
  return guard([&] {
    check_png_geometry(n_images, height, width, elem_bytes);
    TMH_CHECK(total && host_offsets, TMH_EINVAL, "offsets or total pointer is NULL");
    *total = 0;
    host_offsets[0] = 0;
    if (n_images == 0) return;
    TMH_CHECK(host_images && blob_capacity >= 0 && (host_blob || blob_capacity == 0), TMH_EINVAL,
              "images or blob pointer is NULL");
    const int64_t dst_b = n_images * png_bound_bytes(height, width, elem_bytes);
    const int64_t sb = png_scratch_bytes(n_images, height, width, elem_bytes);
    DBuf<uint8_t> images, dst, scratch;
    DBuf<int64_t> off;
    images.upload(host_images, (size_t)n_images * height * width * elem_bytes);
    dst.alloc((size_t)dst_b);
    scratch.alloc((size_t)sb);
    off.alloc((size_t)n_images + 1);
    png_encode_dev(images.p, n_images, height, width, elem_bytes, dst.p, dst_b, off.p, scratch.p, sb,
                   nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    off.download(host_offsets, (size_t)n_images + 1);
    *total = host_offsets[n_images];
    TMH_CHECK(*total <= blob_capacity, TMH_EINVAL,
              "blob capacity smaller than the files (*total has their bytes)");
    dst.download(host_blob, (size_t)*total);
  });
}

}  // extern "C"
