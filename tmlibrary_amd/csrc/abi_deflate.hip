// C-ABI of libtmhip.so (include/tmhip.h): site-image output -- chunk gather,
// GPU deflate, the z projection of imextract.
#include "abi_internal.h"

namespace tmh {

static int64_t chunk_count(int64_t n_images, int height, int width, int chunk_rows, int chunk_cols) {
  return n_images * cdiv(height, chunk_rows) * cdiv(width, chunk_cols);
}

static void check_gather_args(const void* images, int64_t n_images, int height, int width,
                              int elem_bytes, int chunk_rows, int chunk_cols, const void* chunks,
                              const void* raw) {
  TMH_CHECK(n_images >= 0 && height > 0 && width > 0 && chunk_rows > 0 && chunk_cols > 0 &&
                (elem_bytes == 1 || elem_bytes == 2),
            TMH_EINVAL, "bad geometry (elem_bytes must be 1 or 2)");
  TMH_CHECK(chunk_count(n_images, height, width, chunk_rows, chunk_cols) < (int64_t(1) << 31),
            TMH_EINVAL, "more than 2^31-1 chunks");
  TMH_CHECK(n_images == 0 || (images && chunks && raw), TMH_EINVAL,
            "images, chunk table or raw pointer is NULL");
}

static void gather_chunks_dev(const void* dev_images, int64_t n_images, int height, int width,
                              int elem_bytes, int chunk_rows, int chunk_cols,
                              tmh_zchunk* dev_chunks, uint8_t* dev_raw, void* stream) {
  check_gather_args(dev_images, n_images, height, width, elem_bytes, chunk_rows, chunk_cols,
                    dev_chunks, dev_raw);
  if (n_images == 0) return;
  launch_gather_chunks(static_cast<const uint8_t*>(dev_images), n_images, height, width,
                       elem_bytes, chunk_rows, chunk_cols, dev_chunks, dev_raw,
                       (hipStream_t)stream);
}

static void deflate_dev(const uint8_t* dev_raw, int64_t raw_bytes, tmh_zchunk* dev_chunks,
                        int64_t n_chunks, int64_t raw_max, uint8_t* dev_dst, int64_t dst_bytes,
                        void* dev_scratch, int64_t scratch_bytes, int32_t* dev_status,
                        int64_t* dev_total_bytes, void* stream) {
  TMH_CHECK(n_chunks >= 0 && raw_bytes >= 0 && dst_bytes >= 0 && raw_max >= 0, TMH_EINVAL,
            "bad sizes");
  TMH_CHECK(n_chunks < (int64_t(1) << 31) && raw_max < (int64_t(1) << 31), TMH_EINVAL,
            "chunk count and chunk size must be below 2^31");
  TMH_CHECK(dev_total_bytes, TMH_EINVAL, "total bytes pointer is NULL");
  if (n_chunks == 0) {
    TMH_HIP(hipMemsetAsync(dev_total_bytes, 0, sizeof(int64_t), (hipStream_t)stream));
    return;
  }
  TMH_CHECK(dev_raw && dev_chunks && dev_dst && dev_scratch && dev_status, TMH_EINVAL,
            "raw, chunk table, destination, scratch or status pointer is NULL");
  TMH_CHECK(dst_bytes >= n_chunks * deflate_bound_bytes(raw_max), TMH_EINVAL,
            "destination smaller than n_chunks * tmh_deflate_bound(raw_max)");
  TMH_CHECK(scratch_bytes >= deflate_scratch_bytes(n_chunks, raw_max), TMH_EINVAL,
            "scratch smaller than tmh_deflate_scratch_bytes");
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_scratch) & 15) == 0, TMH_EINVAL,
            "scratch must be 16-byte aligned");
  launch_deflate(dev_raw, raw_bytes, dev_chunks, n_chunks, raw_max, dev_dst,
                 static_cast<uint8_t*>(dev_scratch), dev_status, dev_total_bytes,
                 (hipStream_t)stream);
}

static void check_zproject_args(const void* planes, int64_t n_sites, int z, int height, int width,
                                int elem_bytes, const void* out) {
  TMH_CHECK(n_sites >= 0 && z >= 1 && height > 0 && width > 0 &&
                (elem_bytes == 1 || elem_bytes == 2),
            TMH_EINVAL, "bad geometry (z must be at least 1, elem_bytes 1 or 2)");
  TMH_CHECK(n_sites == 0 || (planes && out), TMH_EINVAL, "planes or output pointer is NULL");
}

static void zproject_max_dev(const void* dev_planes, int64_t n_sites, int z, int height, int width,
                             int elem_bytes, void* dev_out, void* stream) {
  check_zproject_args(dev_planes, n_sites, z, height, width, elem_bytes, dev_out);
  TMH_CHECK(((reinterpret_cast<uintptr_t>(dev_planes) | reinterpret_cast<uintptr_t>(dev_out)) &
             (uintptr_t)(elem_bytes - 1)) == 0,
            TMH_EINVAL, "planes and output must be aligned to their element");
  launch_zproject_max(dev_planes, n_sites, z, height, width, elem_bytes, dev_out,
                      (hipStream_t)stream);
}

}  // namespace tmh

extern "C" {

int64_t tmh_deflate_bound(int64_t raw_len) { return raw_len >= 0 ? deflate_bound_bytes(raw_len) : 0; }

int64_t tmh_deflate_scratch_bytes(int64_t n_chunks, int64_t raw_max) {
  return n_chunks > 0 && raw_max >= 0 ? deflate_scratch_bytes(n_chunks, raw_max) : 0;
}

int tmh_gather_chunks_device(const void* dev_images, int64_t n_images, int height, int width,
                             int elem_bytes, int chunk_rows, int chunk_cols,
                             tmh_zchunk* dev_chunks, uint8_t* dev_raw, void* stream) {
  return guard([&] {
    gather_chunks_dev(dev_images, n_images, height, width, elem_bytes, chunk_rows, chunk_cols,
                      dev_chunks, dev_raw, stream);
  });
}

int tmh_deflate_device(const uint8_t* dev_raw, int64_t raw_bytes, tmh_zchunk* dev_chunks,
                       int64_t n_chunks, int64_t raw_max, uint8_t* dev_dst, int64_t dst_bytes,
                       void* dev_scratch, int64_t scratch_bytes, int32_t* dev_status,
                       int64_t* dev_total_bytes, void* stream) {
  return guard([&] {
    deflate_dev(dev_raw, raw_bytes, dev_chunks, n_chunks, raw_max, dev_dst, dst_bytes, dev_scratch,
                scratch_bytes, dev_status, dev_total_bytes, stream);
  });
}

int tmh_zproject_max_device(const void* dev_planes, int64_t n_sites, int z, int height, int width,
                            int elem_bytes, void* dev_out, void* stream) {
  return guard([&] {
    zproject_max_dev(dev_planes, n_sites, z, height, width, elem_bytes, dev_out, stream);
  });
}

int tmh_deflate_images(const void* host_images, int64_t n_images, int height, int width,
                       int elem_bytes, int chunk_rows, int chunk_cols, tmh_zchunk* host_chunks,
                       uint8_t* host_blob, int64_t blob_capacity, int32_t* host_status,
                       int64_t* total) {
  return guard([&] {
    check_gather_args(host_images, n_images, height, width, elem_bytes, chunk_rows, chunk_cols,
                      host_chunks, host_blob);
    TMH_CHECK(total && (n_images == 0 || host_status), TMH_EINVAL,
              "status or total pointer is NULL");
    *total = 0;
    if (n_images == 0) return;
    const int64_t n = chunk_count(n_images, height, width, chunk_rows, chunk_cols);
    const int64_t raw_max = (int64_t)chunk_rows * chunk_cols * elem_bytes;
    const int64_t dst_b = n * deflate_bound_bytes(raw_max), sb = deflate_scratch_bytes(n, raw_max);
    DBuf<uint8_t> images, raw, dst, scratch;
    DBuf<tmh_zchunk> chunks;
    DBuf<int32_t> status;
    DBuf<int64_t> tot;
    images.upload(host_images, (size_t)n_images * height * width * elem_bytes);
    raw.alloc((size_t)(n * raw_max));
    dst.alloc((size_t)dst_b);
    scratch.alloc((size_t)sb);
    chunks.alloc((size_t)n);
    status.alloc((size_t)n);
    tot.alloc(1);
    gather_chunks_dev(images.p, n_images, height, width, elem_bytes, chunk_rows, chunk_cols,
                      chunks.p, raw.p, nullptr);
    deflate_dev(raw.p, n * raw_max, chunks.p, n, raw_max, dst.p, dst_b, scratch.p, sb, status.p,
                tot.p, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    tot.download(total, 1);
    chunks.download(host_chunks, (size_t)n);
    status.download(host_status, (size_t)n);
    TMH_CHECK(*total <= blob_capacity, TMH_EINVAL,
              "blob capacity smaller than the streams (*total has their bytes)");
    dst.download(host_blob, (size_t)*total);
  });
}

int tmh_zproject_max(const void* host_planes, int64_t n_sites, int z, int height, int width,
                     int elem_bytes, void* host_out) {
  return guard([&] {
    check_zproject_args(host_planes, n_sites, z, height, width, elem_bytes, host_out);
    if (n_sites == 0) return;
    const size_t out_b = (size_t)n_sites * height * width * elem_bytes;
    DBuf<uint8_t> a, b;
    a.upload(host_planes, out_b * z);
    b.alloc(out_b);
    zproject_max_dev(a.p, n_sites, z, height, width, elem_bytes, b.p, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    b.download(host_out, out_b);
  });
}

}  // extern "C"
