// C-ABI of libtmhip.so (include/tmhip.h): the illuminati tile pyramid and its JPEG coding.
#include "abi_internal.h"

namespace tmh {

static constexpr int kPyrTile = 256;

static void check_tile_rects(const tmh_tile_rect* r, int64_t n, int64_t n_sites, int H, int W,
                             int64_t n_tiles) {
  for (int64_t i = 0; i < n; ++i) {
    const tmh_tile_rect& q = r[i];
    TMH_CHECK(q.tile >= 0 && q.tile < n_tiles, TMH_EINVAL, "tile index out of range");
    TMH_CHECK(q.site >= 0 && q.site < n_sites, TMH_EINVAL, "site index out of range");
    TMH_CHECK(q.height > 0 && q.width > 0, TMH_EINVAL, "rectangle has a non-positive size");
    TMH_CHECK(q.src_y >= 0 && q.src_x >= 0 && (int64_t)q.src_y + q.height <= H &&
                  (int64_t)q.src_x + q.width <= W,
              TMH_EINVAL, "rectangle leaves its site");
    TMH_CHECK(q.dst_y >= 0 && q.dst_x >= 0 && (int64_t)q.dst_y + q.height <= kPyrTile &&
                  (int64_t)q.dst_x + q.width <= kPyrTile,
              TMH_EINVAL, "rectangle leaves its tile");
  }
}

static void check_tiles_args(const void* sites, int64_t n_sites, int height, int width,
                             const tmh_tile_rect* rects, int64_t n_rects, const void* tiles,
                             int tile_rows, int tile_cols) {
  TMH_CHECK(sites && tiles, TMH_EINVAL, "sites or tiles pointer is NULL");
  TMH_CHECK(rects || n_rects == 0, TMH_EINVAL, "rectangle table is NULL");
  TMH_CHECK(n_sites > 0 && height > 0 && width > 0 && tile_rows > 0 && tile_cols > 0 &&
                n_rects >= 0,
            TMH_EINVAL, "sizes must be positive");
  TMH_CHECK((int64_t)tile_rows * tile_cols < (int64_t(1) << 31) && n_rects < (int64_t(1) << 31),
            TMH_EINVAL, "more than 2^31 tiles or rectangles");
  check_tile_rects(rects, n_rects, n_sites, height, width, (int64_t)tile_rows * tile_cols);
}

static void tiles_base_dev(const uint8_t* dev_sites, int64_t n_sites, int height, int width,
                           const tmh_tile_rect* host_rects, int64_t n_rects, uint8_t* dev_tiles,
                           int tile_rows, int tile_cols, void* stream) {
  check_tiles_args(dev_sites, n_sites, height, width, host_rects, n_rects, dev_tiles, tile_rows,
                   tile_cols);
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_tiles) & 15) == 0, TMH_EINVAL,
            "tiles must be 16-byte aligned");
  const int64_t nt = (int64_t)tile_rows * tile_cols;
  // counting sort by tile: tbeg[t] .. tbeg[t + 1] index tile t's rectangles
  std::vector<int> tbeg((size_t)nt + 1, 0);
  for (int64_t i = 0; i < n_rects; ++i) tbeg[(size_t)host_rects[i].tile + 1] += 1;
  for (int64_t t = 0; t < nt; ++t) tbeg[(size_t)t + 1] += tbeg[(size_t)t];
  std::vector<tmh_tile_rect> sorted((size_t)std::max<int64_t>(n_rects, 1));
  {
    std::vector<int> at(tbeg.begin(), tbeg.end() - 1);
    for (int64_t i = 0; i < n_rects; ++i) sorted[(size_t)at[(size_t)host_rects[i].tile]++] = host_rects[i];
  }
  DBuf<tmh_tile_rect> d_rects;
  DBuf<int> d_tbeg;
  d_rects.alloc(sorted.size());
  d_tbeg.alloc(tbeg.size());
  const hipStream_t s = (hipStream_t)stream;
  TMH_HIP(hipMemcpyAsync(d_rects.p, sorted.data(), sorted.size() * sizeof(tmh_tile_rect),
                         hipMemcpyHostToDevice, s));
  TMH_HIP(hipMemcpyAsync(d_tbeg.p, tbeg.data(), tbeg.size() * sizeof(int), hipMemcpyHostToDevice,
                         s));
  launch_tiles_base(dev_sites, n_sites, height, width, d_rects.p, d_tbeg.p, dev_tiles, nt, s);
  TMH_HIP(hipStreamSynchronize(s));  // the table's buffers are freed on return
}

// side of the last output mosaic along an axis of n source tiles
static int last_mosaic_side(int n, int last) {
  return (n & 1) ? last : kPyrTile + last;
}

static void check_shrink_args(const void* src, int rows, int cols, int last_h, int last_w,
                              const void* dst, const int* dlh, const int* dlw) {
  TMH_CHECK(src && dst && dlh && dlw, TMH_EINVAL, "NULL pointer");
  TMH_CHECK(rows > 0 && cols > 0, TMH_EINVAL, "sizes must be positive");
  TMH_CHECK(last_h >= 1 && last_h <= kPyrTile && last_w >= 1 && last_w <= kPyrTile, TMH_EINVAL,
            "last tile row height / column width must be in 1..256");
  TMH_CHECK(last_mosaic_side(rows, last_h) >= 2 && last_mosaic_side(cols, last_w) >= 2, TMH_EINVAL,
            "a last mosaic one pixel wide has no half");
  TMH_CHECK(src != dst, TMH_EINVAL, "source and output level must be distinct");
}

static void pyramid_shrink2_dev(const uint8_t* dev_src, int src_rows, int src_cols, int src_last_h,
                                int src_last_w, uint8_t* dev_dst, int* dst_last_h, int* dst_last_w,
                                void* stream) {
  check_shrink_args(dev_src, src_rows, src_cols, src_last_h, src_last_w, dev_dst, dst_last_h,
                    dst_last_w);
  TMH_CHECK(((reinterpret_cast<uintptr_t>(dev_src) | reinterpret_cast<uintptr_t>(dev_dst)) & 15) == 0,
            TMH_EINVAL, "levels must be 16-byte aligned");
  launch_pyramid_shrink2(dev_src, src_rows, src_cols, src_last_h, src_last_w, dev_dst,
                         (hipStream_t)stream);
  *dst_last_h = last_mosaic_side(src_rows, src_last_h) / 2;
  *dst_last_w = last_mosaic_side(src_cols, src_last_w) / 2;
}

static void check_jpeg_args(const void* level, int rows, int cols, int last_h, int last_w,
                            const void* out, int64_t out_capacity, const void* offsets,
                            const void* total) {
  TMH_CHECK(level && offsets && total, TMH_EINVAL, "level, offsets or total pointer is NULL");
  TMH_CHECK(rows >= 1 && cols >= 1, TMH_EINVAL, "sizes must be positive");
  TMH_CHECK((int64_t)rows * cols < (int64_t(1) << 31) - 1, TMH_EINVAL, "more than 2^31 tiles");
  TMH_CHECK(last_h >= 1 && last_h <= kPyrTile && last_w >= 1 && last_w <= kPyrTile, TMH_EINVAL,
            "last tile row height / column width must be in 1..256");
  TMH_CHECK(!out || out_capacity >= 0, TMH_EINVAL, "negative output capacity");
}

// dev_out == NULL: measures only (the offsets and *total)
static void jpeg_encode_level_dev(const uint8_t* dev_level, int rows, int cols, int last_h,
                                  int last_w, int quality, uint8_t* dev_out, int64_t out_capacity,
                                  int64_t* dev_offsets, int64_t* total, void* stream) {
  check_jpeg_args(dev_level, rows, cols, last_h, last_w, dev_out, out_capacity, dev_offsets,
                  total);
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_level) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(dev_offsets) & 7) == 0,
            TMH_EINVAL, "the level must be 16-byte and the offsets 8-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)rows * cols;
  std::vector<uint8_t> tab(jpeg_tables_bytes());
  jpeg_tables_host(quality, tab.data());
  DBuf<uint8_t> d_tab;
  d_tab.alloc(tab.size());
  TMH_HIP(hipMemcpyAsync(d_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
  launch_jpeg_measure(dev_level, rows, cols, last_h, last_w, d_tab.p, dev_offsets, s);
  TMH_HIP(hipMemcpyAsync(total, dev_offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  TMH_HIP(hipStreamSynchronize(s));
  if (!dev_out) return;
  TMH_CHECK(out_capacity >= *total, TMH_EINVAL,
            "the output holds " + std::to_string(out_capacity) + " bytes, the level's files " +
                std::to_string(*total));
  launch_jpeg_write(dev_level, rows, cols, last_h, last_w, d_tab.p, dev_offsets, dev_out, s);
  TMH_HIP(hipStreamSynchronize(s));  // complete on return; the tables are freed
}

static void check_roundtrip_args(const void* level, int rows, int cols, int last_h, int last_w,
                                 const void* out) {
  TMH_CHECK(level && out, TMH_EINVAL, "level or output pointer is NULL");
  TMH_CHECK(rows >= 1 && cols >= 1, TMH_EINVAL, "sizes must be positive");
  TMH_CHECK((int64_t)rows * cols < (int64_t(1) << 31) - 1, TMH_EINVAL, "more than 2^31 tiles");
  TMH_CHECK(last_h >= 1 && last_h <= kPyrTile && last_w >= 1 && last_w <= kPyrTile, TMH_EINVAL,
            "last tile row height / column width must be in 1..256");
  TMH_CHECK(level != out, TMH_EINVAL, "level and output must be distinct");
}

static void jpeg_roundtrip_level_dev(const uint8_t* dev_level, int rows, int cols, int last_h,
                                     int last_w, int quality, uint8_t* dev_out, void* stream) {
  check_roundtrip_args(dev_level, rows, cols, last_h, last_w, dev_out);
  TMH_CHECK(((reinterpret_cast<uintptr_t>(dev_level) | reinterpret_cast<uintptr_t>(dev_out)) & 15) == 0,
            TMH_EINVAL, "levels must be 16-byte aligned");
  launch_jpeg_roundtrip(dev_level, rows, cols, last_h, last_w, quality, dev_out,
                        (hipStream_t)stream);
}

static void check_decode_args(const void* blob, const void* offsets, int64_t n, const void* tiles,
                              const void* dims, const void* status) {
  TMH_CHECK(n >= 0 && n < (int64_t(1) << 31) - 1, TMH_EINVAL, "file count must be in 0..2^31-2");
  TMH_CHECK(offsets, TMH_EINVAL, "offsets pointer is NULL");
  TMH_CHECK(n == 0 || (blob && tiles && dims && status), TMH_EINVAL,
            "blob, tiles, dims or status pointer is NULL");
}

static void jpeg_decode_tiles_dev(const uint8_t* dev_blob, const int64_t* dev_offsets, int64_t n,
                                  uint8_t* dev_tiles, int32_t* dev_dims, int32_t* dev_status,
                                  void* stream) {
  check_decode_args(dev_blob, dev_offsets, n, dev_tiles, dev_dims, dev_status);
  TMH_CHECK((reinterpret_cast<uintptr_t>(dev_tiles) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(dev_offsets) & 7) == 0 &&
                ((reinterpret_cast<uintptr_t>(dev_dims) | reinterpret_cast<uintptr_t>(dev_status)) & 3) == 0,
            TMH_EINVAL, "tiles must be 16-byte, offsets 8-byte, dims and status 4-byte aligned");
  if (n == 0) return;
  const hipStream_t s = (hipStream_t)stream;
  std::vector<uint8_t> tab(jpeg_decode_tables_bytes());
  jpeg_decode_tables_host(tab.data());
  DBuf<uint8_t> d_tab;
  d_tab.alloc(tab.size());
  TMH_HIP(hipMemcpyAsync(d_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
  launch_jpeg_decode_tiles(dev_blob, dev_offsets, n, d_tab.p, dev_tiles, dev_dims, dev_status, s);
  TMH_HIP(hipStreamSynchronize(s));  // complete on return; the tables are freed
}

}  // namespace tmh

extern "C" {

int tmh_tiles_base_device(const uint8_t* dev_sites, int64_t n_sites, int height, int width,
                          const tmh_tile_rect* host_rects, int64_t n_rects, uint8_t* dev_tiles,
                          int tile_rows, int tile_cols, void* stream) {
  return guard([&] {
    tiles_base_dev(dev_sites, n_sites, height, width, host_rects, n_rects, dev_tiles, tile_rows,
                   tile_cols, stream);
  });
}

int tmh_tiles_base(const uint8_t* host_sites, int64_t n_sites, int height, int width,
                   const tmh_tile_rect* host_rects, int64_t n_rects, uint8_t* host_tiles,
                   int tile_rows, int tile_cols) {
  return guard([&] {
    check_tiles_args(host_sites, n_sites, height, width, host_rects, n_rects, host_tiles,
                     tile_rows, tile_cols);
    const size_t in_b = (size_t)n_sites * height * width;
    const size_t out_b = (size_t)tile_rows * tile_cols * kPyrTile * kPyrTile;
    DBuf<uint8_t> a, b;
    a.upload(host_sites, in_b);
    b.alloc(out_b);
    tiles_base_dev(a.p, n_sites, height, width, host_rects, n_rects, b.p, tile_rows, tile_cols,
                   nullptr);
    b.download(host_tiles, out_b);
  });
}

int tmh_pyramid_shrink2_device(const uint8_t* dev_src, int src_rows, int src_cols, int src_last_h,
                               int src_last_w, uint8_t* dev_dst, int* dst_last_h, int* dst_last_w,
                               void* stream) {
  return guard([&] {
    pyramid_shrink2_dev(dev_src, src_rows, src_cols, src_last_h, src_last_w, dev_dst, dst_last_h,
                        dst_last_w, stream);
  });
}

int tmh_pyramid_shrink2(const uint8_t* host_src, int src_rows, int src_cols, int src_last_h,
                        int src_last_w, uint8_t* host_dst, int* dst_last_h, int* dst_last_w) {
  return guard([&] {
    check_shrink_args(host_src, src_rows, src_cols, src_last_h, src_last_w, host_dst, dst_last_h,
                      dst_last_w);
    const size_t tb = (size_t)kPyrTile * kPyrTile;
    const size_t in_b = (size_t)src_rows * src_cols * tb;
    const size_t out_b = (size_t)((src_rows + 1) / 2) * ((src_cols + 1) / 2) * tb;
    DBuf<uint8_t> a, b;
    a.upload(host_src, in_b);
    b.upload(host_dst, out_b);  // odd mosaics keep theirs
    pyramid_shrink2_dev(a.p, src_rows, src_cols, src_last_h, src_last_w, b.p, dst_last_h,
                        dst_last_w, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    b.download(host_dst, out_b);
  });
}

int tmh_jpeg_encode_level_device(const uint8_t* dev_level, int rows, int cols, int last_h,
                                 int last_w, int quality, uint8_t* dev_out, int64_t out_capacity,
                                 int64_t* dev_offsets, int64_t* total, void* stream) {
  return guard([&] {
    jpeg_encode_level_dev(dev_level, rows, cols, last_h, last_w, quality, dev_out, out_capacity,
                          dev_offsets, total, stream);
  });
}

int tmh_jpeg_encode_level(const uint8_t* host_level, int rows, int cols, int last_h, int last_w,
                          int quality, uint8_t* host_out, int64_t out_capacity,
                          int64_t* host_offsets, int64_t* total) {
  return guard([&] {
    check_jpeg_args(host_level, rows, cols, last_h, last_w, host_out, out_capacity, host_offsets,
                    total);
    const size_t n = (size_t)rows * cols, in_b = n * kPyrTile * kPyrTile;
    DBuf<uint8_t> a, b;
    DBuf<int64_t> off;
    a.upload(host_level, in_b);
    off.alloc(n + 1);
    jpeg_encode_level_dev(a.p, rows, cols, last_h, last_w, quality, nullptr, 0, off.p, total,
                          nullptr);
    off.download(host_offsets, n + 1);
    if (!host_out) return;
    TMH_CHECK(out_capacity >= *total, TMH_EINVAL,
              "the output holds " + std::to_string(out_capacity) + " bytes, the level's files " +
                  std::to_string(*total));
    b.alloc((size_t)*total);
    jpeg_encode_level_dev(a.p, rows, cols, last_h, last_w, quality, b.p, *total, off.p, total,
                          nullptr);
    b.download(host_out, (size_t)*total);
  });
}

int tmh_jpeg_roundtrip_level_device(const uint8_t* dev_level, int rows, int cols, int last_h,
                                    int last_w, int quality, uint8_t* dev_out, void* stream) {
  return guard([&] {
    jpeg_roundtrip_level_dev(dev_level, rows, cols, last_h, last_w, quality, dev_out, stream);
  });
}

int tmh_jpeg_roundtrip_level(const uint8_t* host_level, int rows, int cols, int last_h, int last_w,
                             int quality, uint8_t* host_out) {
  return guard([&] {
    check_roundtrip_args(host_level, rows, cols, last_h, last_w, host_out);
    const size_t bytes = (size_t)rows * cols * kPyrTile * kPyrTile;
    DBuf<uint8_t> a, b;
    a.upload(host_level, bytes);
    b.alloc(bytes);
    jpeg_roundtrip_level_dev(a.p, rows, cols, last_h, last_w, quality, b.p, nullptr);
    TMH_HIP(hipStreamSynchronize(nullptr));
    b.download(host_out, bytes);
  });
}

int tmh_jpeg_decode_tiles_device(const uint8_t* dev_blob, const int64_t* dev_offsets, int64_t n,
                                 uint8_t* dev_tiles, int32_t* dev_dims, int32_t* dev_status,
                                 void* stream) {
  return guard([&] {
    jpeg_decode_tiles_dev(dev_blob, dev_offsets, n, dev_tiles, dev_dims, dev_status, stream);
  });
}

int tmh_jpeg_decode_tiles(const uint8_t* host_blob, const int64_t* host_offsets, int64_t n,
                          uint8_t* host_tiles, int32_t* host_dims, int32_t* host_status) {
  return guard([&] {
    check_decode_args(host_blob, host_offsets, n, host_tiles, host_dims, host_status);
    if (n == 0) return;
    TMH_CHECK(host_offsets[0] >= 0, TMH_EINVAL, "offsets must not be negative");
    for (int64_t i = 0; i < n; ++i)
      TMH_CHECK(host_offsets[i + 1] >= host_offsets[i], TMH_EINVAL, "offsets must not decrease");
    const size_t blob_b = (size_t)host_offsets[n], tiles_b = (size_t)n * kPyrTile * kPyrTile;
    DBuf<uint8_t> blob, tiles;
    DBuf<int64_t> off;
    DBuf<int32_t> dims, status;
    blob.alloc(blob_b ? blob_b : 1);
    TMH_HIP(hipMemcpy(blob.p, host_blob, blob_b, hipMemcpyHostToDevice));
    off.upload(host_offsets, (size_t)n + 1);
    tiles.alloc(tiles_b);
    dims.alloc(2 * (size_t)n);
    status.alloc((size_t)n);
    jpeg_decode_tiles_dev(blob.p, off.p, n, tiles.p, dims.p, status.p, nullptr);
    tiles.download(host_tiles, tiles_b);
    dims.download(host_dims, 2 * (size_t)n);
    status.download(host_status, (size_t)n);
  });
}

}  // extern "C"
