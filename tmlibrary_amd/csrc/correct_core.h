// The LUT-path correction of one pixel (tmlib/image.py:599-631), shared by the
// plain correct kernels (apply_kernels.hip) and the jterator channel stack
// (chain_kernels.hip): one definition, so the two produce the same bits and
// flag the same pixels for the f64 refinement.
#pragma once

#include "common.h"

namespace tmh {

constexpr float kLog2_10 = 3.32192809488736234787f;

// correct-path log10 of a value >= kLutLds as an f32 hi/lo pair (out of line:
// rare for microscopy data, and a global LUT load in the pixel loop would make
// the compiler wait for the prefetched sites)
__device__ __noinline__ inline float2 corr_log_slow(uint32_t u) {
  const double L = log10((double)u);
  const float hi = (float)L;
  return make_float2(hi, (float)(L - (double)hi));
}

// the correction of one pixel u (pixel index p) given its log10 (hi, lo) (or
// value) L; m = mconst (M hi, M lo, T, 0)
// (site s): a result beyond the f32 error bound T = m.z is flagged for the
// f64 refinement (common.h)
template <bool LOG, int BITS>
__device__ __forceinline__ uint32_t correct_l(float Lh, float Ll, const float4 c, const float4 m,
                                              int64_t s, int64_t p, const FixList& fl,
                                              int clip_lo, int clip_hi) {
  const float d = (Lh - c.x) + (Ll - c.y);        // (img - mean)
  const float t = fmaf(d, c.z, m.x) + m.y;         // * mean(std)/std + mean(mean)
  const float o = LOG ? exp2f(t * kLog2_10) : t;   // 10 ** t
  if (__builtin_fabsf(o) >= m.z) fix_push(fl, s, p);
  // numpy float64 -> uint astype on x86: trunc to int32 (out of range/NaN ->
  // INT32_MIN), keep the low bits (image.py:631)
  const int32_t iv = (o >= -2147483648.0f && o < 2147483648.0f) ? (int32_t)o : INT32_MIN;
  uint32_t r = (uint32_t)iv & ((1u << BITS) - 1u);
  if (clip_lo >= 0) {
    r = r < (uint32_t)clip_lo ? (uint32_t)clip_lo : r;
    r = r > (uint32_t)clip_hi ? (uint32_t)clip_hi : r;
  }
  return r;
}

template <bool LOG, int BITS>
__device__ __forceinline__ uint32_t correct1(uint32_t u, const float4 c, const float2* slut,
                                             const float4 m, int64_t s, int64_t p,
                                             const FixList& fl, int clip_lo, int clip_hi) {
  float2 l;
  if (LOG) {
    l = slut[u < (uint32_t)kLutLds ? u : 0u];
    if (u >= (uint32_t)kLutLds) l = corr_log_slow(u);
  } else {
    l = make_float2((float)u, 0.0f);
  }
  return correct_l<LOG, BITS>(l.x, l.y, c, m, s, p, fl, clip_lo, clip_hi);
}

}  // namespace tmh
