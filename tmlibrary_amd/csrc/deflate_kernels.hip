// GPU deflate of HDF5 gzip chunks (gfx950 / MI355X) -- the site-image output
// path: the mirror of inflate_kernels.hip.
//
// Reference: tmlib/workflow/imextract/api.py:88-157 (planes of a site,
// np.max(np.dstack(planes), axis=2) when there are several, then
// ChannelImageFile.put) and tmlib/models/file.py:353-363 /
// writers.py:384-387 (h5py writes the gzip-filtered /array dataset: libhdf5's
// deflate filter runs zlib's deflate on every chunk).  Each HDF5 chunk is an
// independent zlib stream, so a batch of sites is thousands of independent
// streams: k_gather_chunks cuts [image][H][W] into chunk-major raw bytes
// (the inverse of k_place_chunks), k_deflate_chunks codes one chunk per
// workgroup (deflate_core.h, the same code tests/deflate_host.cpp runs on the
// CPU: the bytes are identical), k_scan_streams / k_copy_streams pack the
// streams into one dense blob and fill src_off / src_len of the tmh_zchunk
// table that tmh_inflate_device and libtmh5's raw-chunk writer read.
// k_zproject_max is imextract's projection over the z planes of a site.
#include "common.h"
#include "deflate_core.h"

namespace tmh {

constexpr int kDGrid = 512;  // workgroups of k_deflate_chunks (each with its own scratch)

static int64_t align16(int64_t v) { return (v + 15) & ~int64_t(15); }

struct DeflateScratch {
  int64_t lens, slots, slot_stride, dist, head, total;
};
static DeflateScratch deflate_layout(int64_t n_chunks, int64_t raw_max) {
  DeflateScratch L;
  const int64_t g = std::min<int64_t>(n_chunks, kDGrid);
  L.lens = 0;
  L.slots = align16(n_chunks * 8);
  L.slot_stride = align16(deflate_slot_bytes(raw_max));
  L.dist = L.slots + n_chunks * L.slot_stride;
  L.head = L.dist + g * (int64_t)kDSeg * 2;  // a multiple of 16
  L.total = L.head + g * (int64_t(4) << kDHashBits);
  return L;
}

int64_t deflate_bound_bytes(int64_t raw_len) { return deflate_bound(raw_len); }

int64_t deflate_scratch_bytes(int64_t n_chunks, int64_t raw_max) {
  return deflate_layout(n_chunks, raw_max).total;
}

// Chunk ci of the table (n_images x chunk rows x chunk columns, row-major):
// the table entry, and its chunk_rows x chunk_cols elements out of image
// ci / (chunks per image), zero (HDF5's fill value) past the dataset's extent.
// Workgroups of 256 threads, gridDim.y per chunk, 16-byte copies where the
// rows allow, else per byte.
__global__ __launch_bounds__(256) void k_gather_chunks(const uint8_t* __restrict__ images,
                                                       int64_t n_chunks, int height, int width,
                                                       int esize, int chunk_rows, int chunk_cols,
                                                       int per_row, int per_image,
                                                       tmh_zchunk* __restrict__ chunks,
                                                       uint8_t* __restrict__ raw) {
  const int64_t ci = blockIdx.x;
  if (ci >= n_chunks) return;
  const int64_t image = ci / per_image;
  const int k = (int)(ci - image * per_image);
  const int row0 = (k / per_row) * chunk_rows, col0 = (k % per_row) * chunk_cols;
  const int64_t chunk_bytes = (int64_t)chunk_rows * chunk_cols * esize;
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    tmh_zchunk c;
    c.src_off = 0;
    c.src_len = 0;
    c.raw_off = ci * chunk_bytes;
    c.raw_len = chunk_bytes;
    c.image = image;
    c.row0 = row0;
    c.col0 = col0;
    c.flags = 0;
    c.reserved = 0;
    chunks[ci] = c;
  }
  const int rows = min(chunk_rows, height - row0);
  const int cols = min(chunk_cols, width - col0);
  const int64_t rb = (int64_t)cols * esize;             // bytes of a row inside the image
  const int64_t dstride = (int64_t)chunk_cols * esize;   // raw row stride
  const int64_t sstride = (int64_t)width * esize;
  const uint8_t* s = images + (image * height + row0) * sstride + (int64_t)col0 * esize;
  uint8_t* d = raw + ci * chunk_bytes;
  const bool v16 = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0 &&
                   (rb & 15) == 0 && (sstride & 15) == 0 && (dstride & 15) == 0;
  const int64_t step = (int64_t)gridDim.y * 256;
  if (v16) {
    const int64_t vrow = dstride / 16, vin = rb / 16;
    for (int64_t t = (int64_t)blockIdx.y * 256 + threadIdx.x; t < chunk_rows * vrow; t += step) {
      const int64_t r = t / vrow, q = t - r * vrow;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r < rows && q < vin) v = reinterpret_cast<const uint4*>(s + r * sstride)[q];
      reinterpret_cast<uint4*>(d + r * dstride)[q] = v;
    }
  } else {
    for (int64_t t = (int64_t)blockIdx.y * 256 + threadIdx.x; t < chunk_bytes; t += step) {
      const int64_t r = t / dstride, q = t - r * dstride;
      d[t] = (r < rows && q < rb) ? s[r * sstride + q] : (uint8_t)0;
    }
  }
}

// One workgroup per chunk (grid-strided): deflate_core.h deflate_chunk.  The
// segment's bytes, match lengths, token bitmap, histograms and codes live in
// LDS (one workgroup per CU); match distances and hash buckets in the
// workgroup's part of the scratch.
__global__ __launch_bounds__(kDMaxThreads) void k_deflate_chunks(
    const uint8_t* __restrict__ raw, int64_t raw_bytes, const tmh_zchunk* __restrict__ chunks,
    int64_t n_chunks, int64_t raw_max, uint8_t* __restrict__ scratch, DeflateScratch L,
    int32_t* __restrict__ status) {
  __shared__ DShared z;
  const int tid = threadIdx.x;
  int64_t* lens = reinterpret_cast<int64_t*>(scratch + L.lens);
  uint16_t* dist = reinterpret_cast<uint16_t*>(scratch + L.dist) + (int64_t)blockIdx.x * kDSeg;
  uint32_t* head = reinterpret_cast<uint32_t*>(scratch + L.head) + ((int64_t)blockIdx.x << kDHashBits);
  for (int64_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    const tmh_zchunk c = chunks[ci];
    if (c.raw_off < 0 || c.raw_len < 0 || c.raw_len > raw_max || c.raw_off + c.raw_len > raw_bytes) {
      if (tid == 0) {
        lens[ci] = 0;
        status[ci] = TMH_Z_INPUT;
      }
      continue;  // uniform: c is the same for every thread
    }
    uint32_t* slot = reinterpret_cast<uint32_t*>(scratch + L.slots + ci * L.slot_stride);
    const int64_t len = deflate_chunk(z, raw + c.raw_off, c.raw_len, slot, dist, head, tid, kDMaxThreads);
    if (tid == 0) {
      lens[ci] = len;
      status[ci] = TMH_Z_OK;
    }
  }
}

// Exclusive scan of the stream lengths into the table (one workgroup): thread
// t the chunks [t * per, (t + 1) * per).
__global__ __launch_bounds__(1024) void k_scan_streams(const int64_t* __restrict__ lens,
                                                       int64_t n_chunks,
                                                       tmh_zchunk* __restrict__ chunks,
                                                       int64_t* __restrict__ total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = cdiv(n_chunks, 1024);
  const int64_t i0 = min(n_chunks, t * per), i1 = min(n_chunks, i0 + per);
  int64_t sum = 0;
  for (int64_t i = i0; i < i1; ++i) sum += lens[i];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int k = 0; k < 1024; ++k) {
      const int64_t v = part[k];
      part[k] = run;
      run += v;
    }
    *total = run;
  }
  __syncthreads();
  int64_t off = part[t];
  for (int64_t i = i0; i < i1; ++i) {
    chunks[i].src_off = off;
    chunks[i].src_len = lens[i];
    off += lens[i];
  }
}

// Stream ci from its slot to dst + src_off: aligned 4-byte stores (the
// slot's side of a word is unaligned), the head and tail per byte.
__global__ __launch_bounds__(256) void k_copy_streams(const uint8_t* __restrict__ scratch,
                                                      DeflateScratch L,
                                                      const tmh_zchunk* __restrict__ chunks,
                                                      uint8_t* __restrict__ dst) {
  const int64_t ci = blockIdx.x;
  const uint8_t* s = scratch + L.slots + ci * L.slot_stride;
  const int64_t len = chunks[ci].src_len;
  uint8_t* d = dst + chunks[ci].src_off;
  const int64_t lead = min(len, (int64_t)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3));
  const int64_t words = (len - lead) / 4;
  for (int64_t i = threadIdx.x; i < words; i += 256) {
    uint32_t v;
    __builtin_memcpy(&v, s + lead + 4 * i, 4);
    *reinterpret_cast<uint32_t*>(d + lead + 4 * i) = v;
  }
  for (int64_t i = threadIdx.x; i < len; i += 256)
    if (i < lead || i >= lead + 4 * words) d[i] = s[i];
}

// out[site] = the elementwise maximum of planes[site][0..z): 16 bytes per
// thread and plane where the plane size and the pointers allow, else per
// element.  Memory-bound: every plane byte is read once.
template <typename V>
__global__ __launch_bounds__(256) void k_zproject_max(const V* __restrict__ planes, int64_t n_sites,
                                                      int z, int64_t per_plane,
                                                      V* __restrict__ out) {
  const int64_t n = n_sites * per_plane;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t site = i / per_plane, q = i - site * per_plane;
    const V* p = planes + site * z * per_plane + q;
    V m = p[0];
    for (int k = 1; k < z; ++k) m = __builtin_elementwise_max(m, p[(int64_t)k * per_plane]);
    out[i] = m;
  }
}

void launch_gather_chunks(const uint8_t* images, int64_t n_images, int height, int width,
                          int esize, int chunk_rows, int chunk_cols, tmh_zchunk* chunks,
                          uint8_t* raw, hipStream_t s) {
  const int per_row = (int)cdiv(width, chunk_cols), per_col = (int)cdiv(height, chunk_rows);
  const int64_t n_chunks = n_images * per_row * per_col;
  if (n_chunks <= 0) return;
  ProfScope prof("gather_chunks", s);
  const int64_t vecs = ((int64_t)chunk_rows * chunk_cols * esize + 15) / 16;
  const unsigned ry = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, cdiv(vecs, 256)));
  hipLaunchKernelGGL(k_gather_chunks, dim3((unsigned)n_chunks, ry), dim3(256), 0, s, images,
                     n_chunks, height, width, esize, chunk_rows, chunk_cols, per_row,
                     per_row * per_col, chunks, raw);
  TMH_HIP(hipGetLastError());
}

void launch_deflate(const uint8_t* raw, int64_t raw_bytes, tmh_zchunk* chunks, int64_t n_chunks,
                    int64_t raw_max, uint8_t* dst, uint8_t* scratch, int32_t* status,
                    int64_t* total, hipStream_t s) {
  if (n_chunks <= 0) return;
  const DeflateScratch L = deflate_layout(n_chunks, raw_max);
  {
    ProfScope prof("deflate", s);
    hipLaunchKernelGGL(k_deflate_chunks, dim3((unsigned)std::min<int64_t>(n_chunks, kDGrid)),
                       dim3(kDMaxThreads), 0, s, raw, raw_bytes, chunks, n_chunks, raw_max, scratch,
                       L, status);
  }
  {
    ProfScope prof("deflate_compact", s);
    hipLaunchKernelGGL(k_scan_streams, dim3(1), dim3(1024), 0, s,
                       reinterpret_cast<const int64_t*>(scratch + L.lens), n_chunks, chunks, total);
    hipLaunchKernelGGL(k_copy_streams, dim3((unsigned)n_chunks), dim3(256), 0, s, scratch, L,
                       chunks, dst);
  }
  TMH_HIP(hipGetLastError());
}

void launch_zproject_max(const void* planes, int64_t n_sites, int z, int height, int width,
                         int esize, void* out, hipStream_t s) {
  if (n_sites <= 0) return;
  ProfScope prof("zproject_max", s);
  typedef uint8_t U8x16 __attribute__((ext_vector_type(16)));
  typedef uint16_t U16x8 __attribute__((ext_vector_type(8)));
  const int64_t plane_bytes = (int64_t)height * width * esize;
  const bool v16 = (plane_bytes & 15) == 0 &&
                   ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t per_plane = v16 ? plane_bytes / 16 : (int64_t)height * width;
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n_sites * per_plane, 256), 256 * 32);
  if (v16 && esize == 1)
    hipLaunchKernelGGL(k_zproject_max<U8x16>, dim3(grid), dim3(256), 0, s, (const U8x16*)planes,
                       n_sites, z, per_plane, (U8x16*)out);
  else if (v16)
    hipLaunchKernelGGL(k_zproject_max<U16x8>, dim3(grid), dim3(256), 0, s, (const U16x8*)planes,
                       n_sites, z, per_plane, (U16x8*)out);
  else if (esize == 1)
    hipLaunchKernelGGL(k_zproject_max<uint8_t>, dim3(grid), dim3(256), 0, s,
                       (const uint8_t*)planes, n_sites, z, per_plane, (uint8_t*)out);
  else
    hipLaunchKernelGGL(k_zproject_max<uint16_t>, dim3(grid), dim3(256), 0, s,
                       (const uint16_t*)planes, n_sites, z, per_plane, (uint16_t*)out);
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
