// Irradiance probe volumes, the look-up ("Probe volumes"): irradiance at caller-given points from the eight probes
// around each.  include/hijiki_hip.h (hj_sample_probes) spells the arithmetic out; every operation here is float32, one rounding
// each, uncontracted, in that order.  The SH basis is kernels/hj_sh9.h's, the gather's own.
//   pv_axis       THE text of one axis' clamp: the two probe planes about a coordinate and their weights
//   pv_resolve_record  THE text of the bake's resolve: a probe's gather record to its 27 coefficients and the validity weight
//   k_pv_sample   a grid-stride loop over the points: eight 112-byte records per point as float4 loads, 27 sums in registers
//                 (left out under HJ_PROBES_NO_SAMPLE_KERNEL: a unit that wants pv_axis and PvGrid alone)
// Ordinary loads and stores, no LDS, no atomics and no inline assembly.  No index is formed from a value that has not been clamped:
// whatever the points hold - NaN, infinities - every load stays inside the volume.
#pragma once
#include "hj_sh9.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kPvThreads = 256u;   // threads of a k_pv_* workgroup (4 waves)
constexpr uint32_t kPvVec = 7u;         // float4 of a probe record: 27 coefficients and the validity weight

struct PvGrid {
  float origin[3], spacing[3];
  uint32_t count[3];
};

// One axis: g = (p - origin) / spacing clamped to [0, m] (a NaN becomes 0), m = count - 1; the planes i0 <= i1 <= m about it and the
// weight f of i1 (1 - f: of i0).
HJ_DEV void pv_axis(float p, float origin, float spacing, uint32_t count, uint32_t& i0, uint32_t& i1, float& f) {
  const uint32_t m = count - 1u;
  float g = (p - origin) / spacing;
  g = (g >= 0.0f) ? g : 0.0f;
  g = (g <= (float)m) ? g : (float)m;
  i0 = min((uint32_t)g, m > 0u ? m - 1u : 0u);
  f = g - (float)i0;
  i1 = min(i0 + 1u, m);
}

// THE text of the bake's resolve, for k_pv_resolve (api/probe_volume.hip) and k_pu_resolve (hj_probe_update.h).  r: the 9 float4 of
// one probe's gather record (hj_trace_irradiance's with HJ_GATHER_SH9).  v[3 j + c] = (sum[8 + 3 j + c] * s) * A_band(j), s =
// 12.5663706f / (float)spp; the bands' clamped-cosine factors are pi, 2 pi / 3, pi / 4.  v[27]: 1.0f when the nearest first hit
// (record word 5, +inf without one) is >= min_distance, else 0.0f.
HJ_DEV void pv_resolve_record(const float4* __restrict__ r, float s, float min_distance, float (&v)[28]) {
  constexpr float A0 = 3.14159274f, A1 = 2.09439516f, A2 = 0.785398185f;
  const float nearest = r[1].y;
#pragma unroll
  for (uint32_t m = 0; m < kPvVec; m++) {
    const float4 t = r[2 + m];
    v[4 * m] = t.x; v[4 * m + 1] = t.y; v[4 * m + 2] = t.z; v[4 * m + 3] = t.w;
  }
#pragma unroll
  for (uint32_t k = 0; k < 27u; k++) v[k] = (v[k] * s) * (k < 3u ? A0 : k < 12u ? A1 : A2);
  v[27] = (nearest >= min_distance) ? 1.0f : 0.0f;
}

#ifndef HJ_PROBES_NO_SAMPLE_KERNEL   // (hj_probe_vis.h takes the clamp and the grid above and leaves the kernel to api/probe_volume.hip)
// probes: count[0] * count[1] * count[2] records of kPvVec float4 (at most 2^22: a float4 index stays below 2^25); points: n records of two
// float4 (position.xyz, normal.x | normal.yz, ignored, ignored); out: n float4.  The eight corners' validity weights come first - a
// corner's weight decides whether it counts -, then the records one float4 column at a time: the eight loads of a column are
// independent and issued together, the sums take them in corner order.  A corner with weight 0 leaves every sum as it is (a select,
// not a product: a NaN coefficient behind it cannot leak).  (i + stride stays below 2^31 + 2^19: no wrap.)
__global__ __launch_bounds__(kPvThreads) void k_pv_sample(PvGrid g, const float4* __restrict__ probes, const float4* __restrict__ points, uint32_t n,
                                                          float4* __restrict__ out) {
  const uint32_t stride = gridDim.x * kPvThreads;
  for (uint32_t i = blockIdx.x * kPvThreads + threadIdx.x; i < n; i += stride) {
    const float4 a = points[2 * (size_t)i], b = points[2 * (size_t)i + 1];
    uint32_t x[2], y[2], z[2];
    float fx, fy, fz;
    pv_axis(a.x, g.origin[0], g.spacing[0], g.count[0], x[0], x[1], fx);
    pv_axis(a.y, g.origin[1], g.spacing[1], g.count[1], y[0], y[1], fy);
    pv_axis(a.z, g.origin[2], g.spacing[2], g.count[2], z[0], z[1], fz);
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
    uint32_t q[8];
    float4 last[8];
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {                  // dz outer, dy, dx inner
      q[c] = ((z[c >> 2] * g.count[1] + y[(c >> 1) & 1u]) * g.count[0] + x[c & 1u]) * kPvVec;
      last[c] = probes[q[c] + (kPvVec - 1u)];
    }
    float w[8], wsum = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {
      w[c] = ((wx[c & 1u] * wy[(c >> 1) & 1u]) * wz[c >> 2]) * last[c].w;
      wsum = (w[c] == 0.0f) ? wsum : wsum + w[c];
    }
    float acc[28];
#pragma unroll
    for (uint32_t m = 0; m < kPvVec; m++) {
      float4 v[8];
#pragma unroll
      for (uint32_t c = 0; c < 8u; c++) v[c] = (m + 1u < kPvVec) ? probes[q[c] + m] : last[c];
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
      for (uint32_t c = 0; c < 8u; c++) {
        const bool on = w[c] != 0.0f;
        s0 = on ? s0 + v[c].x * w[c] : s0;
        s1 = on ? s1 + v[c].y * w[c] : s1;
        s2 = on ? s2 + v[c].z * w[c] : s2;
        s3 = on ? s3 + v[c].w * w[c] : s3;             // (of the last column: the validity's own sum, not used)
      }
      acc[4 * m] = s0; acc[4 * m + 1] = s1; acc[4 * m + 2] = s2; acc[4 * m + 3] = s3;
    }
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(wsum == 0.0f)) {
      float Y[9];
      sh9_basis(normalize3(V(a.w, b.x, b.y)), Y);
      float e[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (uint32_t j = 0; j < 9u; j++) {
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) e[c] = e[c] + (acc[3 * j + c] / wsum) * Y[j];
      }
      o = make_float4(e[0], e[1], e[2], wsum);
    }
    out[i] = o;
  }
}
#endif  // HJ_PROBES_NO_SAMPLE_KERNEL

}  // namespace hj
