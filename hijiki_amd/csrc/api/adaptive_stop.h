// The stop rule of the adaptive queries - the ONE text of it: k_pa_accumulate (api/path_adaptive.hip) and k_ga_accumulate
// (api/gather_adaptive.hip) both call it.  Needs kernels/hj_num.h (f_max) before it; no include guard beyond the pragma.
#pragma once

#pragma clang fp contract(off)

namespace hj {

// The stop rule, after a round that brought the ray to m samples (2 <= spp_min <= m <= spp_max).  S1, S2: the float32 running sums
// of the samples' luminance Y and of Y * Y.  Every operation is float32, in this order, uncontracted; the divisions are correctly
// rounded; f_max is maxNum.
//   mean = S1 / (float)m
//   var  = max(0, S2 - S1 * mean) / (float)(m - 1)
//   sem2 = var / (float)m                                  (the squared standard error of the mean luminance)
//   thr  = rel_error * max(mean, floor)
//   stop = sem2 <= thr * thr  ||  m == spp_max             (a NaN sem2 compares false: such a ray stops only at spp_max)
HJ_DEV bool pa_stops(float S1, float S2, uint32_t m, uint32_t spp_max, float rel_error, float floor, float& sem2) {
  const float mean = S1 / (float)m;
  const float var = f_max(0.f, S2 - S1 * mean) / (float)(m - 1u);
  sem2 = var / (float)m;
  const float thr = rel_error * f_max(mean, floor);
  return sem2 <= thr * thr || m == spp_max;
}

struct AdaptiveArgs {
  uint32_t spp_max;
  float rel_error, floor;
};

}  // namespace hj
