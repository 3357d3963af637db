// Host build of the GPU PNG encoder's core (tmlibrary_amd/csrc/png_core.h over
// deflate_core.h) for tests/test_png_cpu.py: the same filter, piece, CRC and
// framing code, run as a workgroup of one thread and a wave of one lane on
// the CPU, so its files can be checked against Pillow and zlib without a GPU
// (and under the sanitizers).  The steps are those of png_kernels.hip.
//   png_host CASES OUT OUTLENS
// CASES: per case four int64 (images, height, width, bytes per element) and
// the pixels; writes the files one after another and one int64 length per file.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define TMH_DDEV static inline
#define TMH_DHD static inline
#define TMH_DSYNC() (void)0
#define TMH_DSYNC_GLOBAL() (void)0
#define TMH_DOR32(p, v) (*(p) |= (v))
#define TMH_DMAX32(p, v) (*(p) = std::max<uint32_t>(*(p), (v)))
#define TMH_DADD32(p, v) (*(p) += (v))
#define TMH_DLOAD32(p) (*(p))
#define TMH_PSUM64(v) (v)
#include "../tmlibrary_amd/csrc/png_core.h"

static std::vector<uint8_t> slurp(const char* p) {
  FILE* f = fopen(p, "rb");
  if (!f) exit(2);
  std::vector<uint8_t> v;
  static uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  using namespace tmh;
  if (argc != 4) return 2;
  const std::vector<uint8_t> in = slurp(argv[1]);
  static DShared z;
  static PShared ps;
  png_crc_table(ps, 0, 1);
  std::vector<uint16_t> dist(kDSeg);
  std::vector<uint32_t> head(size_t(1) << kDHashBits);
  std::vector<int64_t> olens;
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  size_t at = 0;
  while (at < in.size()) {
    int64_t hd[4];
    if (at + 32 > in.size()) return 3;
    memcpy(hd, in.data() + at, 32);
    at += 32;
    const int64_t n = hd[0];
    const int H = (int)hd[1], W = (int)hd[2], es = (int)hd[3];
    const int64_t nb = (int64_t)W * es, px = (int64_t)H * nb;
    if (n < 0 || H <= 0 || W <= 0 || (es != 1 && es != 2) || at + (size_t)(n * px) > in.size()) return 3;
    for (int64_t im = 0; im < n; ++im) {
      // exactly the bytes the kernels get: a read or write past them is the sanitizer's to find
      std::vector<uint8_t> img(in.begin() + at, in.begin() + at + px);
      at += (size_t)px;
      const int64_t F = png_stream_bytes(H, W, es), np = png_pieces(F);
      std::vector<uint8_t> stage((size_t)F);
      for (int r = 0; r < H; ++r) {
        // the vector form where a 16-byte load is an aligned one on this side too
        const uint8_t* row = img.data() + (int64_t)r * nb;
        png_filter_row(row, r ? row - nb : nullptr, nb, es, stage.data() + (int64_t)r * (1 + nb), 0, 1);
      }
      const int64_t slot_b = deflate_piece_slot_bytes(std::min<int64_t>(F, kPngPiece));
      std::vector<std::vector<uint32_t>> slots((size_t)np);
      std::vector<int64_t> lens((size_t)np);
      std::vector<uint32_t> crcs((size_t)np);
      uint32_t a = 1, b = 0;
      int64_t total = 0;
      for (int64_t k = 0; k < np; ++k) {
        const int64_t len = png_piece_len(F, k);
        slots[k].assign((size_t)(slot_b / 4), 0xA5A5A5A5u);
        std::vector<uint8_t> piece(stage.begin() + k * kPngPiece, stage.begin() + k * kPngPiece + len);
        uint32_t sums[2];
        lens[k] = deflate_piece(z, piece.data(), len, k == 0, k == np - 1, slots[k].data(), slot_b / 4,
                                dist.data(), head.data(), sums, 0, 1);
        if (lens[k] > deflate_piece_stored_bytes(len, k == 0, k == np - 1)) return 4;
        crcs[k] = png_crc_idat(ps, slots[k].data(), lens[k], 0, 1);
        png_adler_join(a, b, sums[0], sums[1], len);
        total += lens[k];
      }
      std::vector<uint8_t> file((size_t)png_file_bytes(total, np));
      if ((int64_t)file.size() > png_bound(H, W, es)) return 4;
      png_write_head(file.data(), H, W, es);
      int64_t rel = kPngHead;
      for (int64_t k = 0; k < np; ++k) {
        png_write_idat_frame(file.data() + rel, lens[k], crcs[k]);
        memcpy(file.data() + rel + 8, slots[k].data(), (size_t)lens[k]);
        rel += 12 + lens[k];
      }
      png_write_tail(file.data() + rel, b << 16 | a);
      if (rel + kPngTail != (int64_t)file.size()) return 5;
      fwrite(file.data(), 1, file.size(), fo);
      olens.push_back((int64_t)file.size());
    }
  }
  fclose(fo);
  FILE* fl = fopen(argv[3], "wb");
  if (!fl) return 2;
  fwrite(olens.data(), 8, olens.size(), fl);
  fclose(fl);
  return 0;
}
