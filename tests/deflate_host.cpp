// Host build of the GPU deflate core (tmlibrary_amd/csrc/deflate_core.h) for
// tests/test_deflate_cpu.py: the same encode code, run as a workgroup of one
// thread on the CPU, so its streams can be checked against zlib's inflate
// without a GPU (and under the sanitizers).
//   deflate_host RAW LENS OUT OUTLENS
// RAW: the chunks' bytes one after another; LENS: one int64 per chunk; writes
// the streams one after another and one int64 length per stream.
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
#include "../tmlibrary_amd/csrc/deflate_core.h"

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
  if (argc != 5) return 2;
  const std::vector<uint8_t> raw = slurp(argv[1]), lb = slurp(argv[2]);
  const size_t n = lb.size() / 8;
  std::vector<int64_t> lens(n), olens(n);
  if (n) memcpy(lens.data(), lb.data(), n * 8);
  static tmh::DShared z;
  std::vector<uint16_t> dist(tmh::kDSeg);
  std::vector<uint32_t> head(size_t(1) << tmh::kDHashBits);
  FILE* fo = fopen(argv[3], "wb");
  if (!fo) return 2;
  int64_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    if (lens[i] < 0 || off + lens[i] > (int64_t)raw.size()) return 3;
    // exactly the slot the kernel gets: a write past it is the sanitizer's to find
    std::vector<uint32_t> slot((size_t)(tmh::deflate_slot_bytes(lens[i]) / 4));
    std::vector<uint8_t> in(raw.begin() + off, raw.begin() + off + lens[i]);
    olens[i] = tmh::deflate_chunk(z, in.data(), lens[i], slot.data(), dist.data(), head.data(), 0, 1);
    if (olens[i] > tmh::deflate_bound(lens[i])) return 4;
    fwrite(slot.data(), 1, (size_t)olens[i], fo);
    off += lens[i];
  }
  fclose(fo);
  FILE* fl = fopen(argv[4], "wb");
  if (!fl) return 2;
  fwrite(olens.data(), 8, n, fl);
  fclose(fl);
  return 0;
}
