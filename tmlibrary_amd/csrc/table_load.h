// Scaling on load, shared by the kernels that read a feature table
// (cluster_kernels.hip, classify_kernels.hip): center[d] / scale[d] are applied
// as (x - c) / s -- one subtract, one divide, nothing to contract -- so the
// values are those k_robust_scale would have stored.
#pragma once

#include "common.h"

namespace tmh {

__device__ __forceinline__ double scaled(double v, const double* c, const double* s, int f) {
  return c ? (v - c[f]) / s[f] : v;
}

// center / scale into LDS (sc[0..d) centres, sc[256..256+d) scales); the
// caller synchronizes
__device__ __forceinline__ void stage_scaler(const double* __restrict__ cen,
                                             const double* __restrict__ scl, int d, double* sc) {
  if (!cen) return;
  for (int f = threadIdx.x; f < d; f += blockDim.x) {
    sc[f] = cen[f];
    sc[256 + f] = scl[f];
  }
}

}  // namespace tmh
