// Line FFT shared by register_kernels.hip and tests/fft_host.cpp: complex f32,
// Stockham autosort with radix 4, 2, 3 and 5 passes between two line buffers.
//
// A line of n values (n = 2^a 3^b 5^c <= kFftMaxLine) is transformed by
// plan.npass passes; pass p with radix R and Ns = the product of the radices
// before it runs n / R butterflies.  Butterfly j reads src[j + r n/R], r < R,
// twiddles element r by exp(-+2 pi i r k / (Ns R)) with k = j mod Ns (taken
// from the n-entry table tw[t] = exp(-2 pi i t / n), built in f64 on the host),
// applies the R-point DFT and writes dst[(j / Ns) Ns R + k + r Ns].  Neither
// direction scales.  The butterflies of one pass are independent, so any
// thread may run any of them; a barrier separates two passes.
//
// A length with a prime factor above 5 is not transformed: fft_line_length
// gives the 5-smooth m >= 2 L - 1 to zero-pad to, the transform then yields the
// LINEAR correlation, and fft_fold_index names the second term that folds it
// back to period L.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define TMH_FFT_HD __host__ __device__ inline
#else
#define TMH_FFT_HD inline
#endif

namespace tmh {

struct cf {
  float x, y;
};

constexpr int kFftMaxLine = 4096;  // 32 KB of complex f32
constexpr int kFftMaxPasses = 8;   // 3^7 = 2187 is the longest chain; 4^6 = 4096 takes 6

struct FftPlan {
  int n;
  int npass;
  int radix[kFftMaxPasses];
};

TMH_FFT_HD cf cf_add(cf a, cf b) { return cf{a.x + b.x, a.y + b.y}; }
TMH_FFT_HD cf cf_sub(cf a, cf b) { return cf{a.x - b.x, a.y - b.y}; }
TMH_FFT_HD cf cf_mul(cf a, cf b) { return cf{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
TMH_FFT_HD cf cf_conj(cf a) { return cf{a.x, -a.y}; }
// a * (+i) when inv, a * (-i) otherwise
TMH_FFT_HD cf cf_rot(cf a, bool inv) { return inv ? cf{-a.y, a.x} : cf{a.y, -a.x}; }

TMH_FFT_HD bool fft_is_smooth(int n) {
  if (n < 1) return false;
  while (n % 2 == 0) n /= 2;
  while (n % 3 == 0) n /= 3;
  while (n % 5 == 0) n /= 5;
  return n == 1;
}

// the smallest 5-smooth number >= n (n >= 1)
TMH_FFT_HD int fft_good_size(int n) {
  while (!fft_is_smooth(n)) ++n;
  return n;
}

// transformed length of an axis of L samples: L itself when it is 5-smooth,
// else the padded length of the linear correlation
TMH_FFT_HD int fft_line_length(int L) { return fft_is_smooth(L) ? L : fft_good_size(2 * L - 1); }

// Lag d of the period-L correlation from a length-m line (m = fft_line_length(L)):
// C[d] = line[d] + line[fft_fold_index(d, L, m)] when that index is >= 0.
// (lag 0 has no second term: lag -L does not overlap, and at m = 2 L - 1 its
// index would alias lag L - 1.)
TMH_FFT_HD int fft_fold_index(int d, int L, int m) { return (m == L || d == 0) ? -1 : m - L + d; }

// false when n is not 5-smooth or too long
TMH_FFT_HD bool fft_make_plan(int n, FftPlan* p) {
  p->n = n;
  p->npass = 0;
  if (n < 1 || n > kFftMaxLine || !fft_is_smooth(n)) return false;
  int r = n;
  while (r % 4 == 0) { p->radix[p->npass++] = 4; r /= 4; }
  while (r % 2 == 0) { p->radix[p->npass++] = 2; r /= 2; }
  while (r % 3 == 0) { p->radix[p->npass++] = 3; r /= 3; }
  while (r % 5 == 0) { p->radix[p->npass++] = 5; r /= 5; }
  return true;
}

// butterfly j of one pass (see the head of the file)
// (q, r) = (a / b, a % b) for 0 <= a < 2^22, 1 <= b, rcp_b = 1.0f / b: the f32
// quotient is off by at most one, which the remainder corrects (an integer
// division costs the device some forty instructions, and every butterfly
// would need two)
TMH_FFT_HD void fft_divmod(int a, int b, float rcp_b, int* q, int* r) {
  int t = (int)((float)a * rcp_b);
  int m = a - t * b;
  if (m < 0) { --t; m += b; }
  if (m >= b) { ++t; m -= b; }
  *q = t;
  *r = m;
}

template <int R>
TMH_FFT_HD void fft_butterfly(const cf* src, cf* dst, int n, int Ns, int tw_step, int jq, int k,
                              int j, const cf* tw, bool inv) {
  const int stride = n / R;
  const int tstep = tw_step * k;
  cf v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    v[r] = src[j + r * stride];
    if (r > 0 && k > 0) {
      cf w = tw[r * tstep];
      if (inv) w.y = -w.y;
      v[r] = cf_mul(v[r], w);
    }
  }
  cf* out = dst + jq * Ns * R + k;
  if constexpr (R == 2) {
    out[0] = cf_add(v[0], v[1]);
    out[Ns] = cf_sub(v[0], v[1]);
  } else if constexpr (R == 3) {
    const float h = 0.8660254037844386f;  // sin(2 pi / 3)
    const cf t = cf_add(v[1], v[2]);
    const cf m = cf{v[0].x - 0.5f * t.x, v[0].y - 0.5f * t.y};
    const cf d = cf_rot(cf{h * (v[1].x - v[2].x), h * (v[1].y - v[2].y)}, inv);
    out[0] = cf_add(v[0], t);
    out[Ns] = cf_add(m, d);
    out[2 * Ns] = cf_sub(m, d);
  } else if constexpr (R == 4) {
    const cf a = cf_add(v[0], v[2]), b = cf_sub(v[0], v[2]);
    const cf c = cf_add(v[1], v[3]), d = cf_rot(cf_sub(v[1], v[3]), inv);
    out[0] = cf_add(a, c);
    out[Ns] = cf_add(b, d);
    out[2 * Ns] = cf_sub(a, c);
    out[3 * Ns] = cf_sub(b, d);
  } else {
    const float c1 = 0.30901699437494745f, c2 = -0.8090169943749473f;  // cos(2 pi/5), cos(4 pi/5)
    const float s1 = 0.9510565162951535f, s2 = 0.5877852522924731f;    // sin(2 pi/5), sin(4 pi/5)
    const cf a1 = cf_add(v[1], v[4]), a2 = cf_add(v[2], v[3]);
    const cf b1 = cf_sub(v[1], v[4]), b2 = cf_sub(v[2], v[3]);
    const cf p1 = cf{v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y};
    const cf p2 = cf{v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y};
    const cf q1 = cf_rot(cf{s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y}, inv);
    const cf q2 = cf_rot(cf{s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y}, inv);
    out[0] = cf{v[0].x + a1.x + a2.x, v[0].y + a1.y + a2.y};
    out[Ns] = cf_add(p1, q1);
    out[2 * Ns] = cf_add(p2, q2);
    out[3 * Ns] = cf_sub(p2, q2);
    out[4 * Ns] = cf_sub(p1, q1);
  }
}

// butterflies first, first + step, ... of one pass over `lines` lines that lie
// line_stride values apart in src and in dst (the device calls it with
// first = thread, step = threads; the host with 0, 1)
TMH_FFT_HD void fft_pass(const cf* src, cf* dst, int n, int Ns, int R, int lines, int line_stride,
                         const cf* tw, bool inv, int first, int step) {
  const int per = n / R, total = per * lines, tw_step = n / (Ns * R);
  const float rcp_per = 1.0f / (float)per, rcp_ns = 1.0f / (float)Ns;
  const bool ns_pow2 = (Ns & (Ns - 1)) == 0;
  int ns_shift = 0;
  while (ns_pow2 && (1 << ns_shift) < Ns) ++ns_shift;
  for (int i = first; i < total; i += step) {
    int line = 0, j = i, jq, k;
    if (lines > 1) fft_divmod(i, per, rcp_per, &line, &j);
    if (ns_pow2) {
      jq = j >> ns_shift;
      k = j & (Ns - 1);
    } else {
      fft_divmod(j, Ns, rcp_ns, &jq, &k);
    }
    const cf* s = src + (int64_t)line * line_stride;
    cf* d = dst + (int64_t)line * line_stride;
    if (R == 4) fft_butterfly<4>(s, d, n, Ns, tw_step, jq, k, j, tw, inv);
    else if (R == 2) fft_butterfly<2>(s, d, n, Ns, tw_step, jq, k, j, tw, inv);
    else if (R == 3) fft_butterfly<3>(s, d, n, Ns, tw_step, jq, k, j, tw, inv);
    else fft_butterfly<5>(s, d, n, Ns, tw_step, jq, k, j, tw, inv);
  }
}

}  // namespace tmh

#include <cmath>
namespace tmh {
// tw[t] = exp(-2 pi i t / n), computed in f64 and rounded once
inline void fft_twiddles_host(int n, cf* tw) {
  for (int t = 0; t < n; ++t) {
    const double a = -2.0 * 3.14159265358979323846 * (double)t / (double)n;
    tw[t] = cf{(float)std::cos(a), (float)std::sin(a)};
  }
}
}  // namespace tmh
