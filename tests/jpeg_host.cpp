// Host build of the GPU JPEG encoder's core (tmlibrary_amd/csrc/jpeg_core.h)
// for tests/test_jpeg_cpu.py: the same sample, DCT, quantisation, symbol and
// bit emission code k_jpeg_tiles runs, one block after another on the CPU, so
// its files can be compared with libjpeg-turbo's byte for byte without a GPU.
//   jpeg_host TILES OUT SIZES
// TILES: per tile int32 height, width, quality, then height x width bytes;
// writes the files back to back to OUT and one int64 size per tile to SIZES.
//   jpeg_host --division
// checks jpeg_quantise against the plain division for every quantiser.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#define TMH_JHD inline
#include "../tmlibrary_amd/csrc/jpeg_core.h"

using namespace tmh;

struct OrHost {
  static void apply(uint32_t* p, uint32_t v) { *p |= v; }
};

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

static void encode(const uint8_t* px, int H, int W, int quality, std::vector<uint8_t>& out) {
  JpegTables t;
  jpeg_build_tables(quality, &t);
  // the tile as the kernel sees it: in the corner of 256-pitch storage, other bytes around it
  std::vector<uint8_t> tile(256 * 256, 0xAA);
  for (int y = 0; y < H; ++y) memcpy(&tile[(size_t)y * 256], px + (size_t)y * W, (size_t)W);
  const int bh = (H + 7) / 8, bw = (W + 7) / 8, nb = bh * bw;
  std::vector<uint32_t> coef((size_t)nb * kJpegCoefPitch);
  for (int b = 0; b < nb; ++b) {
    int d[64];
    jpeg_load_block(tile.data(), 256, H, W, b / bw, b % bw, d);
    jpeg_fdct_quantise(d, t, &coef[(size_t)b * kJpegCoefPitch]);
  }
  std::vector<int> at((size_t)nb + 1, 0);
  for (int b = 0; b < nb; ++b) {
    JpegCountSink c;
    jpeg_encode_block(&coef[(size_t)b * kJpegCoefPitch],
                      b ? jpeg_coef(&coef[(size_t)(b - 1) * kJpegCoefPitch], 0) : 0, t, c);
    if (c.bits > kJpegMaxBlockBits) exit(3);
    at[(size_t)b + 1] = at[(size_t)b] + c.bits;
  }
  const int bits = at[(size_t)nb];
  std::vector<uint32_t> words((size_t)bits / 32 + 2, 0u);
  for (int b = nb - 1; b >= 0; --b) {  // any order: a block's bits land at its offset
    JpegBitSink<OrHost> s(words.data(), at[(size_t)b]);
    jpeg_encode_block(&coef[(size_t)b * kJpegCoefPitch],
                      b ? jpeg_coef(&coef[(size_t)(b - 1) * kJpegCoefPitch], 0) : 0, t, s);
    s.finish();
  }
  for (int i = 0; i < kJpegHeaderBytes; ++i) out.push_back(jpeg_header_byte(t.header, i, H, W));
  const int nbytes = (bits + 7) / 8, pad = (8 - (bits & 7)) & 7;
  for (int i = 0; i < nbytes; ++i) {
    uint32_t v = jpeg_stream_byte(words.data(), i);
    if (i == nbytes - 1) v |= (1u << pad) - 1u;
    out.push_back((uint8_t)v);
    if (v == 255u) out.push_back(0);
  }
  out.push_back(0xFF);
  out.push_back(0xD9);
}

static int check_division() {
  for (int q = 1; q <= 255; ++q) {
    const uint32_t qv = 8u * (uint32_t)q;
    const uint32_t recip = (uint32_t)((uint64_t(1) << 32) / qv) + 1u;
    for (int x = -32768; x < 32768; ++x) {
      const int a = x < 0 ? -x : x;
      const int want = (x < 0 ? -1 : 1) * (int)(((uint32_t)a + (qv >> 1)) / qv);
      if (jpeg_quantise(x, qv, recip) != want) {
        printf("q %d x %d\n", q, x);
        return 1;
      }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--division")) return check_division();
  if (argc != 4) return 2;
  const std::vector<uint8_t> in = slurp(argv[1]);
  std::vector<uint8_t> out;
  std::vector<int64_t> sizes;
  size_t p = 0;
  while (p + 12 <= in.size()) {
    int32_t hwq[3];
    memcpy(hwq, &in[p], 12);
    p += 12;
    if (hwq[0] < 1 || hwq[0] > 256 || hwq[1] < 1 || hwq[1] > 256) return 2;
    if (p + (size_t)hwq[0] * hwq[1] > in.size()) return 2;
    const size_t before = out.size();
    encode(&in[p], hwq[0], hwq[1], hwq[2], out);
    sizes.push_back((int64_t)(out.size() - before));
    p += (size_t)hwq[0] * hwq[1];
  }
  FILE* fo = fopen(argv[2], "wb");
  fwrite(out.data(), 1, out.size(), fo);
  fclose(fo);
  FILE* fs = fopen(argv[3], "wb");
  fwrite(sizes.data(), 8, sizes.size(), fs);
  fclose(fs);
  return 0;
}
