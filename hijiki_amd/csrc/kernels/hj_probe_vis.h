// Probe visibility ("Probe volumes"): per probe an octahedral map of the mean distance and the mean squared distance to
// the nearest surface, and the look-up of a probe volume that weights each of the eight probes about a point by a back-face factor
// and by Chebyshev's bound on the share of the probe's rays that reach as far as the point - the light-leak weights of Majercik et
// al. 2019.  include/hijiki_hip.h (hj_bake_probe_visibility, hj_sample_probes_visible) spells the arithmetic out; every operation
// here is float32, one rounding each, uncontracted, in that order.  Beside this header hj_probes.h (pv_axis, PvGrid: the one text of
// the clamp), hj_sh9.h and hj_num.h alone: the path kernels' machine code does not depend on this unit.
//   pvv_position    a probe's position from its index: k_pv_points' expression
//   pvv_oct_decode  a point of the octahedral square [-1, 1]^2 to its (unnormalised) direction;  pvv_oct_encode: the way back
//   pvv_border_source  THE text of the border: the interior texel an atlas texel copies;  pvv_moments: THE text of a texel's two moments
//   pvv_ray         THE text of a bake ray: sample r of probe p from a given origin (k_pvv_rays; hj_probe_place.h's k_pp_rays)
//   pvv_corner_fetch  THE text of a corner's Chebyshev loads (k_pvv_sample; hj_probe_place.h's k_pp_sample)
//   (the kernels are left out under HJ_PROBE_VIS_NO_KERNELS: a unit that wants the functions above alone)
//   k_pvv_rays      one thread per ray: hj_trace_rays' record of sample k of a texel of a probe
//   k_pvv_reduce    one thread per atlas texel, border included: the two moments of its s distances, summed in ascending k
//   k_pvv_sample    a grid-stride loop over the points: hj_probes.h's k_pv_sample with the two factors in each corner's weight
// Ordinary loads and stores, no LDS, no atomics and no inline assembly.  No index is formed from a value that has not been clamped:
// whatever points, probes and atlas hold - NaN, infinities - every load stays inside the volume and its atlas.
#pragma once
#define HJ_PROBES_NO_SAMPLE_KERNEL   // pv_axis, PvGrid and the constants of hj_probes.h; k_pv_sample stays api/probe_volume.hip's
#include "hj_probes.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kPvvThreads = 256u;          // threads of a k_pvv_* workgroup (4 waves)
constexpr uint32_t kPvvSlabRays = 1u << 19;     // HJ_PROBE_VIS_SLAB_RAYS: the most rays of one slab of the bake

struct PvvMap {
  uint32_t res, s;          // interior texels per side (4, 8, 16), rays per texel (bake)
  float max_distance, normal_bias;
  uint32_t flags;           // HJ_PROBE_VIS_*
};

HJ_DEV float pvv_sg(float x) { return (x >= 0.0f) ? 1.0f : -1.0f; }

HJ_DEV v3 pvv_position(const PvGrid& g, uint32_t x, uint32_t y, uint32_t z) {
  return V(g.origin[0] + (float)x * g.spacing[0], g.origin[1] + (float)y * g.spacing[1], g.origin[2] + (float)z * g.spacing[2]);
}
HJ_DEV v3 pvv_position(const PvGrid& g, uint32_t p) {
  const uint32_t x = p % g.count[0], yz = p / g.count[0];
  return pvv_position(g, x, yz % g.count[1], yz / g.count[1]);
}

HJ_DEV v3 pvv_oct_decode(float ex, float ey) {
  const float ax = __builtin_fabsf(ex), ay = __builtin_fabsf(ey);
  const float az = (1.0f - ax) - ay;
  if (az >= 0.0f) return V(ex, ey, az);
  return V((1.0f - ay) * pvv_sg(ex), (1.0f - ax) * pvv_sg(ey), az);
}

HJ_DEV void pvv_oct_encode(v3 e, float& px, float& py) {
  const float l1 = (__builtin_fabsf(e.x) + __builtin_fabsf(e.y)) + __builtin_fabsf(e.z);
  px = e.x / l1;
  py = e.y / l1;
  if (e.z < 0.0f) {
    const float ox = px, oy = py;
    px = (1.0f - __builtin_fabsf(oy)) * pvv_sg(ox);
    py = (1.0f - __builtin_fabsf(ox)) * pvv_sg(oy);
  }
}

// THE text of the border: atlas texel (bx, by) of a map of T = res + 2 texels a side -> the interior texel (tx, ty), 0-based, it
// copies (an interior texel: itself) - the octahedral wrap, so that the look-up's bilinear fetch has no special case at the edges.
HJ_DEV void pvv_border_source(uint32_t res, uint32_t bx, uint32_t by, uint32_t& tx, uint32_t& ty) {
  const uint32_t T = res + 2u, last = res - 1u;
  const bool ex = bx == 0u || bx == T - 1u, ey = by == 0u || by == T - 1u;
  if (ex && ey) {                      // a corner: the diagonally opposite interior corner
    tx = bx == 0u ? last : 0u;
    ty = by == 0u ? last : 0u;
  } else if (ey) {                     // top and bottom rows: mirrored in x
    tx = res - bx;
    ty = by == 0u ? 0u : last;
  } else if (ex) {                     // left and right columns: mirrored in y
    tx = bx == 0u ? 0u : last;
    ty = res - by;
  } else {
    tx = bx - 1u;
    ty = by - 1u;
  }
}

// THE text of the moments: h, the v.s hit records (hj_trace_rays') of one interior texel's rays -> (m1, m2), summed in ascending k.
HJ_DEV float2 pvv_moments(const PvvMap& v, const float4* __restrict__ h) {
  float a1 = 0.0f, a2 = 0.0f;
  for (uint32_t k = 0; k < v.s; k++) {
    const float4 r = h[k];
    const float dist = (__float_as_int(r.x) >= 0) ? f_min(r.y, v.max_distance) : v.max_distance;
    a1 = a1 + dist;
    a2 = a2 + dist * dist;
  }
  return make_float2(a1 / (float)v.s, a2 / (float)v.s);
}

// THE text of a bake ray: sample r of probe p (seed + p * seed_stride + r) from the origin o -> rec[0], rec[1], hj_trace_rays' record
// (origin.xyz, dir.x | dir.yz, tMin = 0, tMax = max_distance).
HJ_DEV void pvv_ray(const PvvMap& v, uint32_t seed, uint32_t seed_stride, uint32_t p, uint32_t r, v3 o, float4* __restrict__ rec) {
  const uint32_t t = r / v.s, tx = t % v.res, ty = t / v.res;
  uint32_t state = rng_seed(seed + p * seed_stride + r);
  const float u = rng_float(state), w = rng_float(state);
  const float scale = 2.0f / (float)v.res;
  const float ex = ((float)tx + u) * scale - 1.0f, ey = ((float)ty + w) * scale - 1.0f;
  const v3 d = normalize3(pvv_oct_decode(ex, ey));
  rec[0] = make_float4(o.x, o.y, o.z, d.x);
  rec[1] = make_float4(d.y, d.z, 0.0f, v.max_distance);
}

// THE text of one corner's loads for the Chebyshev factor, for k_pvv_sample and hj_probe_place.h's k_pp_sample (P: the corner's
// probe position, m: its map): whether the factor applies, rr, the bilinear weights and the four texels.  (Of the look-up's three
// per-corner pieces this is the one both kernels call: with it k_pvv_sample keeps its 228 VGPRs; the back-face factor or the bound as
// functions too gave 226 or 230 - DESIGN.md 4, "Probe placement".)
HJ_DEV void pvv_corner_fetch(v3 xb, v3 P, float fres, uint32_t T, const float2* __restrict__ m, bool& away, float& rr, float& tfx, float& tfy, float2& t00,
                             float2& t10, float2& t01, float2& t11) {
  const v3 e = xb - P;
  away = !(e.x == 0.0f && e.y == 0.0f && e.z == 0.0f);
  rr = len3(e);
  float px, py;
  pvv_oct_encode(e, px, py);
  const float ax = (px * 0.5f + 0.5f) * fres + 0.5f, ay = (py * 0.5f + 0.5f) * fres + 0.5f;
  uint32_t ix0, ix1, iy0, iy1;
  pv_axis(ax, 0.0f, 1.0f, T, ix0, ix1, tfx);
  pv_axis(ay, 0.0f, 1.0f, T, iy0, iy1, tfy);
  t00 = m[iy0 * T + ix0];
  t10 = m[iy0 * T + ix1];
  t01 = m[iy1 * T + ix0];
  t11 = m[iy1 * T + ix1];
}

#ifndef HJ_PROBE_VIS_NO_KERNELS   // (hj_probe_update.h takes the functions above and leaves the kernels to api/probe_visibility.hip)
// rays: count records of two float4 (origin.xyz, dir.x | dir.yz, tMin = 0, tMax = max_distance); ray i of the launch is ray
// r = i % (res^2 s) of probe first + i / (res^2 s).  (count <= kPvvSlabRays or a caller's window, below 2^32 either way.)
__global__ __launch_bounds__(kPvvThreads) void k_pvv_rays(PvGrid g, PvvMap v, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t count,
                                                          float4* __restrict__ rays) {
  const uint32_t i = blockIdx.x * kPvvThreads + threadIdx.x;
  if (i >= count) return;
  const uint32_t per = v.res * v.res * v.s;
  const uint32_t p = first + i / per, r = i % per;
  pvv_ray(v, seed, seed_stride, p, r, pvv_position(g, p), rays + 2 * (size_t)i);
}

// hits: hj_trace_rays' records of the slab's rays (probes * res^2 * s float4); atlas: the slab's part, probes * (res + 2)^2 float2.
// A border texel sums the rays of the interior texel it copies: the octahedral wrap, so that the look-up's bilinear fetch has no
// special case at the map's edges.
__global__ __launch_bounds__(kPvvThreads) void k_pvv_reduce(PvvMap v, const float4* __restrict__ hits, uint32_t probes, float2* __restrict__ atlas) {
  const uint32_t T = v.res + 2u, texels = T * T;
  const uint32_t i = blockIdx.x * kPvvThreads + threadIdx.x;
  if (i >= probes * texels) return;
  const uint32_t p = i / texels, b = i % texels;
  uint32_t tx, ty;
  pvv_border_source(v.res, b % T, b / T, tx, ty);
  atlas[i] = pvv_moments(v, hits + ((size_t)p * (v.res * v.res) + (ty * v.res + tx)) * v.s);
}

// probes, points, out: k_pv_sample's; atlas: (res + 2)^2 float2 per probe (not read with both NO_ flags: may be null then).  Per point
// the eight corners' validity words and, with the Chebyshev factor, their 4 x 8 atlas texels are loaded first - independent loads,
// issued together -, then the weights, then k_pv_sample's columns.
__global__ __launch_bounds__(kPvvThreads) void k_pvv_sample(PvGrid g, PvvMap v, const float4* __restrict__ probes, const float2* __restrict__ atlas,
                                                            const float4* __restrict__ points, uint32_t n, float4* __restrict__ out) {
  const uint32_t stride = gridDim.x * kPvvThreads;
  const bool backface = (v.flags & 2u) == 0u, chebyshev = (v.flags & 4u) == 0u;     // HJ_PROBE_VIS_NO_BACKFACE, _NO_CHEBYSHEV
  const uint32_t T = v.res + 2u;
  const float fres = (float)v.res;
  for (uint32_t i = blockIdx.x * kPvvThreads + threadIdx.x; i < n; i += stride) {
    const float4 a = points[2 * (size_t)i], b = points[2 * (size_t)i + 1];
    const v3 pos = V(a.x, a.y, a.z), nn = normalize3(V(a.w, b.x, b.y));
    const v3 xb = V(pos.x + nn.x * v.normal_bias, pos.y + nn.y * v.normal_bias, pos.z + nn.z * v.normal_bias);
    uint32_t x[2], y[2], z[2];
    float fx, fy, fz;
    pv_axis(a.x, g.origin[0], g.spacing[0], g.count[0], x[0], x[1], fx);
    pv_axis(a.y, g.origin[1], g.spacing[1], g.count[1], y[0], y[1], fy);
    pv_axis(a.z, g.origin[2], g.spacing[2], g.count[2], z[0], z[1], fz);
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
    uint32_t q[8];
    float4 last[8];
    float2 t00[8], t10[8], t01[8], t11[8];
    float tfx[8], tfy[8], rr[8], wb[8];
    bool away[8];                                         // the corner's probe is not where xb is: the Chebyshev factor applies
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {                  // dz outer, dy, dx inner
      const uint32_t cx = x[c & 1u], cy = y[(c >> 1) & 1u], cz = z[c >> 2];
      const uint32_t p = (cz * g.count[1] + cy) * g.count[0] + cx;
      q[c] = p * kPvVec;
      last[c] = probes[q[c] + (kPvVec - 1u)];
      const v3 P = pvv_position(g, cx, cy, cz);
      wb[c] = 1.0f;
      if (backface && !(P.x == pos.x && P.y == pos.y && P.z == pos.z)) {
        const v3 t = normalize3(P - pos);
        const float h = (dot3(t, nn) + 1.0f) * 0.5f;
        wb[c] = h * h + 0.2f;
      }
      away[c] = false;
      if (chebyshev) pvv_corner_fetch(xb, P, fres, T, atlas + (size_t)p * (T * T), away[c], rr[c], tfx[c], tfy[c], t00[c], t10[c], t01[c], t11[c]);
    }
    float w[8], wsum = 0.0f;
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {
      float wv = 1.0f;
      if (away[c]) {
        const float gx = 1.0f - tfx[c], gy = 1.0f - tfy[c];
        const float m1 = (t00[c].x * gx + t10[c].x * tfx[c]) * gy + (t01[c].x * gx + t11[c].x * tfx[c]) * tfy[c];
        const float m2 = (t00[c].y * gx + t10[c].y * tfx[c]) * gy + (t01[c].y * gx + t11[c].y * tfx[c]) * tfy[c];
        if (rr[c] > m1) {
          const float var = __builtin_fabsf(m1 * m1 - m2), dl = rr[c] - m1;
          const float k = var / (var + dl * dl);
          wv = f_max((k * k) * k, 0.05f);
        }
      }
      w[c] = ((((wx[c & 1u] * wy[(c >> 1) & 1u]) * wz[c >> 2]) * last[c].w) * wb[c]) * wv;
      wsum = (w[c] == 0.0f) ? wsum : wsum + w[c];
    }
    float acc[28];
#pragma unroll
    for (uint32_t m = 0; m < kPvVec; m++) {
      float4 r[8];
#pragma unroll
      for (uint32_t c = 0; c < 8u; c++) r[c] = (m + 1u < kPvVec) ? probes[q[c] + m] : last[c];
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
      for (uint32_t c = 0; c < 8u; c++) {
        const bool on = w[c] != 0.0f;
        s0 = on ? s0 + r[c].x * w[c] : s0;
        s1 = on ? s1 + r[c].y * w[c] : s1;
        s2 = on ? s2 + r[c].z * w[c] : s2;
        s3 = on ? s3 + r[c].w * w[c] : s3;             // (of the last column: the validity's own sum, not used)
      }
      acc[4 * m] = s0; acc[4 * m + 1] = s1; acc[4 * m + 2] = s2; acc[4 * m + 3] = s3;
    }
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(wsum == 0.0f)) {
      float Y[9];
      sh9_basis(nn, Y);
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
#endif  // HJ_PROBE_VIS_NO_KERNELS

}  // namespace hj
