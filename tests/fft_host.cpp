// Stand-alone host harness over tmlibrary_amd/csrc/fft_core.h (the per-line
// arithmetic of register_kernels.hip), driven by tests/test_align_cpu.py.
//
//   fft_host fft L in out    in: L complex64.  out: the forward transform, then
//                            the inverse of that (unscaled), 2 L complex64.
//   fft_host corr L in out   in: two real f32 lines a, b of L values.  out: L
//                            f32, C[d] = sum_r a[r] b[(r + d) mod L], computed
//                            as the kernels do: z = a + i b zero-padded to
//                            fft_line_length(L), one forward transform, the
//                            Hermitian split and conj(F(a)) F(b), one inverse,
//                            then the fold back to period L.
// Every buffer is a heap block of its exact size, so the sanitizer build
// catches any index past a line or a table.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tmlibrary_amd/csrc/fft_core.h"

using tmh::cf;

static bool transform(std::vector<cf>& line, const std::vector<cf>& tw, bool inv) {
  tmh::FftPlan plan;
  const int n = (int)line.size();
  if (!tmh::fft_make_plan(n, &plan)) return false;
  std::vector<cf> other(line.size());
  cf* src = line.data();
  cf* dst = other.data();
  int Ns = 1;
  for (int p = 0; p < plan.npass; ++p) {
    tmh::fft_pass(src, dst, n, Ns, plan.radix[p], 1, n, tw.data(), inv, 0, 1);
    Ns *= plan.radix[p];
    cf* t = src;
    src = dst;
    dst = t;
  }
  if (src != line.data()) memcpy(line.data(), src, line.size() * sizeof(cf));
  return true;
}

template <typename T>
static bool read_exact(const char* path, std::vector<T>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(T), v.size(), f);
  fclose(f);
  return got == v.size();
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: fft_host fft|corr L in out\n");
    return 2;
  }
  const int L = atoi(argv[2]);
  if (L < 1) return 2;
  FILE* out = nullptr;
  if (!strcmp(argv[1], "fft")) {
    std::vector<cf> line(L), tw(L);
    if (!read_exact(argv[3], line)) return 3;
    tmh::fft_twiddles_host(L, tw.data());
    if (!transform(line, tw, false)) return 4;
    out = fopen(argv[4], "wb");
    if (!out) return 3;
    fwrite(line.data(), sizeof(cf), line.size(), out);
    if (!transform(line, tw, true)) return 4;
    fwrite(line.data(), sizeof(cf), line.size(), out);
  } else if (!strcmp(argv[1], "corr")) {
    std::vector<float> ab(2 * (size_t)L);
    if (!read_exact(argv[3], ab)) return 3;
    const int m = tmh::fft_line_length(L);
    std::vector<cf> z(m, cf{0.f, 0.f}), p(m), tw(m);
    for (int i = 0; i < L; ++i) z[i] = cf{ab[i], ab[L + i]};
    tmh::fft_twiddles_host(m, tw.data());
    if (!transform(z, tw, false)) return 4;
    const float scale = 0.25f / (float)m;
    for (int k = 0; k < m; ++k) {
      const cf a = z[k], b = tmh::cf_conj(z[(m - k) % m]);
      const cf ft = tmh::cf_add(a, b);                    // 2 F(a)
      const cf fr = tmh::cf_rot(tmh::cf_sub(a, b), false);  // 2 F(b)
      const cf q = tmh::cf_mul(tmh::cf_conj(ft), fr);
      p[k] = cf{q.x * scale, q.y * scale};
    }
    if (!transform(p, tw, true)) return 4;
    std::vector<float> c(L);
    for (int d = 0; d < L; ++d) {
      const int f = tmh::fft_fold_index(d, L, m);
      c[d] = p[d].x + (f >= 0 ? p[f].x : 0.f);
    }
    out = fopen(argv[4], "wb");
    if (!out) return 3;
    fwrite(c.data(), sizeof(float), c.size(), out);
  } else {
    return 2;
  }
  fclose(out);
  return 0;
}
