// Host build of the GPU JPEG decoder's core and of the round trip
// (tmlibrary_amd/csrc/jpeg_core.h) for tests/test_jpeg_decode_cpu.py: the same
// header walk, bit reader, symbol decoder, dequantisation and inverse DCT
// k_jpeg_decode_tiles and k_jpeg_roundtrip run, one block after another on
// the CPU, so pictures and statuses can be compared with libjpeg-turbo's and
// the literal's without a GPU.  Stand-alone, so it also builds with
// -fsanitize=address,undefined.
//   jpeg_decode_host decode FILES OUT
// FILES: int64 n, n + 1 int64 offsets, then the files back to back (each is
// copied to a heap block of its exact size, so a read past it is an error a
// sanitizer sees).  OUT: per file int32 status, height, width, then
// height x width bytes.
//   jpeg_decode_host roundtrip TILES OUT
// TILES: per tile int32 height, width, quality, then height x width bytes;
// OUT: the round-tripped height x width bytes of every tile.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#define TMH_JHD inline
#include "../tmlibrary_amd/csrc/jpeg_core.h"

using namespace tmh;

static std::vector<uint8_t> slurp(const char* p) {
  FILE* f = fopen(p, "rb");
  if (!f) exit(2);
  std::vector<uint8_t> v;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

struct PutCoef {
  int* c;
  void operator()(int i, int v) { c[i] = v; }
};

// the file into 256-pitch tile storage, as the kernel leaves it
static int decode(const uint8_t* f, int64_t n, const JpegDecodeTables& t, uint8_t* tile, int* H,
                  int* W) {
  memset(tile, 0, 65536);
  *H = *W = 0;
  JpegFileInfo info;
  int status = jpeg_parse_header(f, n, t, &info);
  if (status) return status;
  const int bh = (info.height + 7) / 8, bw = (info.width + 7) / 8;
  JpegBitReader r(f, info.scan, n);
  int dc = 0;
  for (int b = 0; b < bh * bw && !status; ++b) {
    int c[64] = {0};
    PutCoef put{c};
    status = jpeg_decode_block(r, t, &dc, put);
    if (status) break;
    for (int i = 0; i < 64; ++i) c[i] *= info.q[i];
    jpeg_idct_block(c);
    const int by = b / bw, bx = b % bw;
    for (int y = 0; y < 8 && 8 * by + y < info.height; ++y) {
      const uint64_t v = jpeg_pack_row(c, y, info.width - 8 * bx);
      memcpy(tile + (8 * by + y) * 256 + 8 * bx, &v, 8);
    }
  }
  if (!status && !r.at_eoi()) status = kJpegCorrupt;
  if (status) {
    memset(tile, 0, 65536);
    return status;
  }
  *H = info.height;
  *W = info.width;
  return kJpegOk;
}

static int main_decode(const char* in_path, const char* out_path) {
  const std::vector<uint8_t> in = slurp(in_path);
  if (in.size() < 16) return 2;
  int64_t n;
  memcpy(&n, in.data(), 8);
  if (n < 0 || in.size() < 8 * (size_t)(n + 2)) return 2;
  std::vector<int64_t> off((size_t)n + 1);
  memcpy(off.data(), in.data() + 8, 8 * off.size());
  const uint8_t* blob = in.data() + 8 * (size_t)(n + 2);
  JpegDecodeTables t;
  jpeg_build_decode_tables(&t);
  FILE* fo = fopen(out_path, "wb");
  std::vector<uint8_t> tile(65536);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t size = off[(size_t)i + 1] - off[(size_t)i];
    if (size < 0 || 8 * (size_t)(n + 2) + (size_t)off[(size_t)i + 1] > in.size()) return 2;
    uint8_t* file = (uint8_t*)malloc(size ? (size_t)size : 1);
    memcpy(file, blob + off[(size_t)i], (size_t)size);
    int32_t shw[3];
    shw[0] = decode(file, size, t, tile.data(), &shw[1], &shw[2]);
    free(file);
    fwrite(shw, 4, 3, fo);
    for (int y = 0; y < shw[1]; ++y) fwrite(&tile[(size_t)y * 256], 1, (size_t)shw[2], fo);
    // outside the picture the storage is 0
    for (int y = 0; y < 256; ++y)
      for (int x = 0; x < 256; ++x)
        if ((y >= shw[1] || x >= shw[2]) && tile[(size_t)y * 256 + x]) return 3;
  }
  fclose(fo);
  return 0;
}

static int main_roundtrip(const char* in_path, const char* out_path) {
  const std::vector<uint8_t> in = slurp(in_path);
  FILE* fo = fopen(out_path, "wb");
  size_t p = 0;
  while (p + 12 <= in.size()) {
    int32_t hwq[3];
    memcpy(hwq, &in[p], 12);
    p += 12;
    const int H = hwq[0], W = hwq[1];
    if (H < 1 || H > 256 || W < 1 || W > 256 || p + (size_t)H * W > in.size()) return 2;
    JpegTables t;
    jpeg_build_tables(hwq[2], &t);
    std::vector<uint8_t> tile(65536, 0xAA), out(65536, 0x5C);
    for (int y = 0; y < H; ++y) memcpy(&tile[(size_t)y * 256], &in[p + (size_t)y * W], (size_t)W);
    const int bh = (H + 7) / 8, bw = (W + 7) / 8;
    for (int b = 0; b < bh * bw; ++b) {
      int d[64];
      jpeg_load_block(tile.data(), 256, H, W, b / bw, b % bw, d);
      jpeg_roundtrip_block(d, t);
      for (int y = 0; y < 8 && 8 * (b / bw) + y < H; ++y) {
        const uint64_t v = jpeg_pack_row(d, y, W - 8 * (b % bw));
        memcpy(&out[(size_t)(8 * (b / bw) + y) * 256 + 8 * (b % bw)], &v, 8);
      }
    }
    for (int y = 0; y < H; ++y) fwrite(&out[(size_t)y * 256], 1, (size_t)W, fo);
    p += (size_t)H * W;
  }
  fclose(fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "decode")) return main_decode(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "roundtrip")) return main_roundtrip(argv[2], argv[3]);
  return 2;
}
