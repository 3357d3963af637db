// Per-object intensity features from their integer rows:
// the merge of the z-planes of a time point and the five features, the same
// lines for the finalize kernel (measure_kernels.hip) and for the host build
// the CPU suite runs (tests/intensity_host.cpp).  Nothing here needs 128-bit
// compiler support: the device has no runtime conversion for __int128.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/tmhip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMH_IC_HD __host__ __device__ inline
#else
#define TMH_IC_HD inline
#endif

namespace tmh {

// a * b as (hi, lo) of 128 bits
TMH_IC_HD void ic_mul128(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
  const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);  // < 3 * 2^32
  *lo = (p00 & 0xffffffffull) | (mid << 32);
  *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

TMH_IC_HD int ic_clz64(uint64_t v) {  // v != 0
  int s = 0;
  for (int k = 32; k > 0; k >>= 1)
    if ((v >> (64 - k)) == 0) {
      v <<= k;
      s += k;
    }
  return s;
}

// (hi, lo) as f64 with ONE round-to-nearest: the top 64 bits, the dropped bits
// OR-ed into bit 0 as a sticky bit (bit 0 lies below the 53-bit result and its
// guard bit, so it only breaks ties), converted and scaled
TMH_IC_HD double ic_u128_to_double(uint64_t hi, uint64_t lo) {
  if (hi == 0) return (double)lo;
  const int s = ic_clz64(hi);
  uint64_t top = hi, dropped = lo;
  if (s) {
    top = (hi << s) | (lo >> (64 - s));
    dropped = lo << s;
  }
  top |= dropped != 0 ? 1ull : 0ull;
  return ldexp((double)top, 64 - s);
}

// b into a: sums add, max takes the max, min skips empty rows (they store 0)
TMH_IC_HD void ic_merge(tmh_intensity_row* a, const tmh_intensity_row& b) {
  if (b.n == 0) return;
  if (a->n == 0) {
    *a = b;
    return;
  }
  a->sum += b.sum;
  a->sum_sq += b.sum_sq;
  a->n += b.n;
  a->min = b.min < a->min ? b.min : a->min;
  a->max = b.max > a->max ? b.max : a->max;
}

// out[5] = max, mean, min, sum, std (np.std, ddof 0); n == 0: NaN.  std takes
// num = n * sum_sq - sum^2 exactly in 128 bits (both products < 2^94), one
// rounding to f64, sqrt, one division.  Rows no image gives (num < 0) give 0.
TMH_IC_HD void ic_features(const tmh_intensity_row& r, double* out) {
  if (r.n <= 0) {
    const double nan = NAN;
    out[0] = out[1] = out[2] = out[3] = out[4] = nan;
    return;
  }
  const double n = (double)r.n;
  out[0] = (double)r.max;
  out[1] = (double)r.sum / n;
  out[2] = (double)r.min;
  out[3] = (double)r.sum;
  uint64_t ah, al, bh, bl;
  ic_mul128((uint64_t)r.n, r.sum_sq, &ah, &al);
  ic_mul128(r.sum, r.sum, &bh, &bl);
  const bool negative = ah < bh || (ah == bh && al < bl);
  const uint64_t lo = al - bl, hi = ah - bh - (al < bl ? 1ull : 0ull);
  out[4] = negative ? 0.0 : sqrt(ic_u128_to_double(hi, lo)) / n;
}

}  // namespace tmh
