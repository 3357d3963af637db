// Host build of the intensity finalize (tmlibrary_amd/csrc/intensity_core.h):
// the merge and the features the finalize kernel runs, on rows read from a
// file.  tests/test_measure_cpu.py builds this with g++, plain and with
// -fsanitize=address,undefined, and compares the output bit for bit with
// tests/intensity_literal.py.
//
// in:  int64 n_groups, per_group, plane_rows; then tmh_intensity_row
//      [n_groups * per_group][plane_rows]
// out: f64 [n_groups][plane_rows][5]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tmlibrary_amd/csrc/intensity_core.h"

static_assert(sizeof(tmh_intensity_row) == 32, "tmh_intensity_row layout");

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t head[3];
  if (fread(head, sizeof(int64_t), 3, in) != 3) return 4;
  const int64_t n_groups = head[0], per_group = head[1], plane_rows = head[2];
  if (n_groups < 0 || per_group < 1 || plane_rows < 0 || n_groups > 65535 || per_group > 65535 ||
      plane_rows > (1 << 24))
    return 5;
  std::vector<tmh_intensity_row> rows((size_t)(n_groups * per_group * plane_rows));
  if (fread(rows.data(), sizeof(tmh_intensity_row), rows.size(), in) != rows.size()) return 6;
  fclose(in);
  std::vector<double> out((size_t)(n_groups * plane_rows * 5));
  for (int64_t g = 0; g < n_groups; ++g)
    for (int64_t k = 0; k < plane_rows; ++k) {
      const tmh_intensity_row* p = rows.data() + g * per_group * plane_rows + k;
      tmh_intensity_row r = p[0];
      for (int64_t z = 1; z < per_group; ++z) tmh::ic_merge(&r, p[z * plane_rows]);
      tmh::ic_features(r, out.data() + (g * plane_rows + k) * 5);
    }
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 7;
  if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 8;
  fclose(f);
  return 0;
}
