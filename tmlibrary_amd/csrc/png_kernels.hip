// GPU encode of greyscale channel images as PNG files (gfx950 / MI355X).
//
// Reference: tmlib/image.py:672-682 (ChannelImage.png_encode: cv2.imencode of
// the pixel array, what the server's channel-image download and the bulk
// export send).  A PNG is a zlib stream of the filtered rows inside CRC-ed
// chunks.  k_png_filter picks and applies a filter per row (one wave per row)
// into the staging stream; k_png_pieces codes the stream's pieces, one
// workgroup each over a persistent grid (deflate_core.h deflate_piece: the
// code k_deflate_chunks runs, so one image's single stream spreads over many
// workgroups), and computes each piece's IDAT CRC with all its threads;
// k_png_scan joins the Adler-32s and scans the sizes; k_png_pack writes the
// framing and copies the pieces into one dense blob.  png_core.h holds the
// rules, and tests/png_host.cpp runs the same code on the CPU: the bytes are
// identical.
#include "common.h"
#include "png_core.h"

namespace tmh {

constexpr int kPGrid = 512;  // workgroups of k_png_pieces (each with its own match scratch)

static int64_t palign16(int64_t v) { return (v + 15) & ~int64_t(15); }

struct PngScratch {
  int64_t stream, pieces;  // per image: filtered bytes, pieces
  int64_t stage, stage_stride, lens, rel, flen, sums, crc, adler, slots, slot_stride, dist, head, total;
};
static PngScratch png_layout(int64_t n_images, int height, int width, int esize) {
  PngScratch L;
  L.stream = png_stream_bytes(height, width, esize);
  L.pieces = png_pieces(L.stream);
  const int64_t np = n_images * L.pieces, g = std::min<int64_t>(np, kPGrid);
  L.stage = 0;
  L.stage_stride = palign16(L.stream);  // pieces start 16-byte aligned
  L.lens = L.stage + n_images * L.stage_stride;
  L.rel = L.lens + palign16(np * 8);
  L.flen = L.rel + palign16(np * 8);
  L.sums = L.flen + palign16(n_images * 8);
  L.crc = L.sums + palign16(np * 8);
  L.adler = L.crc + palign16(np * 4);
  L.slots = L.adler + palign16(n_images * 4);
  L.slot_stride = palign16(deflate_piece_slot_bytes(std::min<int64_t>(L.stream, kPngPiece)));
  L.dist = L.slots + np * L.slot_stride;
  L.head = L.dist + g * (int64_t)kDSeg * 2;
  L.total = L.head + g * (int64_t(4) << kDHashBits);
  return L;
}

int64_t png_piece_bytes() { return kPngPiece; }
int64_t png_bound_bytes(int height, int width, int esize) { return png_bound(height, width, esize); }
int64_t png_scratch_bytes(int64_t n_images, int height, int width, int esize) {
  return png_layout(n_images, height, width, esize).total;
}

// One wave per row (four rows per workgroup): png_core.h png_filter_row.  The
// row and the row above are read twice (the second time from the caches), 16
// bytes per lane where the rows are 16-byte aligned.
__global__ __launch_bounds__(256) void k_png_filter(const uint8_t* __restrict__ images,
                                                    int64_t n_rows, int height, int width, int esize,
                                                    uint8_t* __restrict__ stage, int64_t stage_stride) {
  const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gr >= n_rows) return;  // a whole wave
  const int64_t image = gr / height, r = gr - image * height;
  const int64_t nb = (int64_t)width * esize;
  const uint8_t* row = images + gr * nb;
  png_filter_row(row, r ? row - nb : nullptr, nb, esize, stage + image * stage_stride + r * (1 + nb),
                 threadIdx.x & 63, 64);
}

// One workgroup per piece (grid-strided): the piece's bytes into its slot,
// its Adler sums, then the CRC-32 of its IDAT chunk.  LDS as k_deflate_chunks
// plus the CRC's table and partial values.
__global__ __launch_bounds__(kDMaxThreads) void k_png_pieces(uint8_t* __restrict__ scratch,
                                                             PngScratch L, int64_t n_pieces) {
  __shared__ DShared z;
  __shared__ PShared ps;
  const int tid = threadIdx.x;
  int64_t* lens = reinterpret_cast<int64_t*>(scratch + L.lens);
  uint32_t* sums = reinterpret_cast<uint32_t*>(scratch + L.sums);
  uint32_t* crcs = reinterpret_cast<uint32_t*>(scratch + L.crc);
  uint16_t* dist = reinterpret_cast<uint16_t*>(scratch + L.dist) + (int64_t)blockIdx.x * kDSeg;
  uint32_t* head = reinterpret_cast<uint32_t*>(scratch + L.head) + ((int64_t)blockIdx.x << kDHashBits);
  png_crc_table(ps, tid, kDMaxThreads);
  for (int64_t pk = blockIdx.x; pk < n_pieces; pk += gridDim.x) {
    const int64_t image = pk / L.pieces, k = pk - image * L.pieces;
    const uint8_t* src = scratch + L.stage + image * L.stage_stride + k * kPngPiece;
    uint32_t* slot = reinterpret_cast<uint32_t*>(scratch + L.slots + pk * L.slot_stride);
    const int64_t len =
        deflate_piece(z, src, png_piece_len(L.stream, k), k == 0, k == L.pieces - 1, slot,
                      L.slot_stride / 4, dist, head, sums + 2 * pk, tid, kDMaxThreads);
    TMH_DSYNC_GLOBAL();  // the slot's words are in L2 before the CRC reads them there
    const uint32_t crc = png_crc_idat(ps, slot, len, tid, kDMaxThreads);
    if (tid == 0) {
      lens[pk] = len;
      crcs[pk] = crc;
    }
  }
}

// One workgroup: thread t the images [t * per, (t + 1) * per).  Per image the
// place of every piece's chunk in its file, the Adler-32 joined in piece order
// and the file's size; then the exclusive scan of the sizes into offsets.
__global__ __launch_bounds__(1024) void k_png_scan(uint8_t* __restrict__ scratch, PngScratch L,
                                                   int64_t n_images, int64_t* __restrict__ offsets) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t* lens = reinterpret_cast<const int64_t*>(scratch + L.lens);
  const uint32_t* sums = reinterpret_cast<const uint32_t*>(scratch + L.sums);
  int64_t* rel = reinterpret_cast<int64_t*>(scratch + L.rel);
  int64_t* flen = reinterpret_cast<int64_t*>(scratch + L.flen);
  uint32_t* adler = reinterpret_cast<uint32_t*>(scratch + L.adler);
  const int64_t per = cdiv(n_images, 1024);
  const int64_t i0 = min(n_images, t * per), i1 = min(n_images, i0 + per);
  int64_t sum = 0;
  for (int64_t i = i0; i < i1; ++i) {
    uint32_t a = 1, b = 0;
    int64_t at = kPngHead;
    for (int64_t k = 0; k < L.pieces; ++k) {
      const int64_t pk = i * L.pieces + k;
      rel[pk] = at;
      at += 12 + lens[pk];
      png_adler_join(a, b, sums[2 * pk], sums[2 * pk + 1], png_piece_len(L.stream, k));
    }
    adler[i] = b << 16 | a;
    flen[i] = at + kPngTail;
    sum += at + kPngTail;
  }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int k = 0; k < 1024; ++k) {
      const int64_t v = part[k];
      part[k] = run;
      run += v;
    }
    offsets[n_images] = run;
  }
  __syncthreads();
  int64_t off = part[t];
  for (int64_t i = i0; i < i1; ++i) {
    offsets[i] = off;
    off += flen[i];
  }
}

// One workgroup per piece: its IDAT chunk into the file (the copy as
// k_copy_streams: aligned 4-byte stores, head and tail per byte); the first
// piece's workgroup also writes the signature and IHDR, the last one's the
// Adler-32's IDAT and IEND.
__global__ __launch_bounds__(256) void k_png_pack(const uint8_t* __restrict__ scratch, PngScratch L,
                                                  int height, int width, int esize,
                                                  const int64_t* __restrict__ offsets,
                                                  uint8_t* __restrict__ dst) {
  const int64_t pk = blockIdx.x;
  const int64_t image = pk / L.pieces, k = pk - image * L.pieces;
  const int64_t len = reinterpret_cast<const int64_t*>(scratch + L.lens)[pk];
  uint8_t* file = dst + offsets[image];
  uint8_t* chunk = file + reinterpret_cast<const int64_t*>(scratch + L.rel)[pk];
  if (threadIdx.x == 0) {
    png_write_idat_frame(chunk, len, reinterpret_cast<const uint32_t*>(scratch + L.crc)[pk]);
    if (k == 0) png_write_head(file, height, width, esize);
    if (k == L.pieces - 1)
      png_write_tail(chunk + 12 + len, reinterpret_cast<const uint32_t*>(scratch + L.adler)[image]);
  }
  const uint8_t* s = scratch + L.slots + pk * L.slot_stride;
  uint8_t* d = chunk + 8;
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

void launch_png(const uint8_t* images, int64_t n_images, int height, int width, int esize,
                uint8_t* dst, int64_t* offsets, uint8_t* scratch, hipStream_t s) {
  if (n_images <= 0) return;
  const PngScratch L = png_layout(n_images, height, width, esize);
  const int64_t np = n_images * L.pieces, rows = n_images * height;
  {
    ProfScope prof("png_filter", s);
    hipLaunchKernelGGL(k_png_filter, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, images, rows,
                       height, width, esize, scratch + L.stage, L.stage_stride);
  }
  {
    ProfScope prof("png_pieces", s);
    hipLaunchKernelGGL(k_png_pieces, dim3((unsigned)std::min<int64_t>(np, kPGrid)),
                       dim3(kDMaxThreads), 0, s, scratch, L, np);
  }
  {
    ProfScope prof("png_pack", s);
    hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(1024), 0, s, scratch, L, n_images, offsets);
    hipLaunchKernelGGL(k_png_pack, dim3((unsigned)np), dim3(256), 0, s, scratch, L, height, width,
                       esize, offsets, dst);
  }
  TMH_HIP(hipGetLastError());
}

}  // namespace tmh
