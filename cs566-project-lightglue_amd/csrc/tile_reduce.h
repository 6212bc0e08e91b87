// Row / column reductions of a 16-wave MFMA tile's accumulators, shared by the similarity kernels
// (assign_h3.hip, nn_match.hip): lane element (ti, tj, r) is row 16 ti + 4 (lane >> 4) + r, column
// 16 tj + (lane & 15) of the wave's 64 x 64 block, so a row lives in the 16 lanes of a DPP row and a
// column in the four lanes 16 apart.
#pragma once

#include "common.h"

namespace lg {

// reductions over the 16 lanes of a DPP row (lanes sharing lane >> 4)
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dppf<0xB1>(v));
  v = fmaxf(v, dppf<0x4E>(v));
  v = fmaxf(v, dppf<0x141>(v));
  return fmaxf(v, dppf<0x140>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dppf<0xB1>(v);
  v += dppf<0x4E>(v);
  v += dppf<0x141>(v);
  return v + dppf<0x140>(v);
}
// e^x for x <= 0 in the statistics sums: one v_exp_f32 (results below 2^-126 of the max, which
// cannot move an fp32 sum, flush to zero); expf's denormal / range handling costs ~7x the VALU
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
// (max, sum exp(x - max)) pairs: merge (commutative: both orders round identically)
template <bool FAST = true>
__device__ __forceinline__ void lse_merge(float& am, float& as, float bm, float bs) {
  const float m = fmaxf(am, bm);
  if (m == -INFINITY) return;
  const float ea = am == m ? 1.f : (FAST ? fast_exp(am - m) : expf(am - m));
  const float eb = bm == m ? 1.f : (FAST ? fast_exp(bm - m) : expf(bm - m));
  as = as * ea + bs * eb;
  am = m;
}
// the same merge with the lanes 16 and 32 apart (the four 16-lane rows of the wave)
__device__ __forceinline__ void lse_merge_rows(float& m, float& s) {
  {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    float m0 = __uint_as_float(a[0]), s0 = __uint_as_float(b[0]);
    lse_merge(m0, s0, __uint_as_float(a[1]), __uint_as_float(b[1]));
    m = m0;
    s = s0;
  }
  {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    float m0 = __uint_as_float(a[0]), s0 = __uint_as_float(b[0]);
    lse_merge(m0, s0, __uint_as_float(a[1]), __uint_as_float(b[1]));
    m = m0;
    s = s0;
  }
}
}  // namespace lg
