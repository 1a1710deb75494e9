// Probe placement ("Probe placement"): per probe an offset from its grid point and an active / inactive state - the
// relocation and classification of Majercik et al. 2021 -, and the update and look-up kernels that read them.
// include/hijiki_hip.h (hj_place_probes and the _placed calls) spells the arithmetic out; every operation here is float32, one
// rounding each, uncontracted, in that order.  The placement array holds one float4 per probe: the offset in world units and the
// state's bits (0: active).  The fresh values, the blend, the rays and the border are the other probe headers' own texts
// (pv_resolve_record, pvv_moments, pvv_border_source, pvv_ray, pu_resolve_probe, pu_reduce_texel); none of their kernels is compiled
// here.  The compaction of the active probes is kernels/hj_compact.h's three pieces.
//   pp_position   a probe's placed position: pvv_position's product and sum, then one more sum
//   k_pp_rays     one thread per ray: pvv_ray from the placed position of probe first + i / R, or of list[i / R]
//   k_pp_reduce   ONE WAVE per probe of a slab: the counts and extremes of its R rays, the relocation step and the classification
//   k_pp_count, k_pp_scan, k_pp_scatter   the window's active probes, in order, as a list of probe indices
//   k_pp_points   one thread per listed probe: its gather point at the placed position (k_pv_points' record)
//   k_pp_resolve  one thread per listed probe: pu_resolve_probe on the record the point's word 7 names
//   k_pp_blend    one thread per interior texel of a slab's listed probes: pu_reduce_texel on the listed probe's map
//   k_pp_sample   the look-up with the placed P and inactive corners switched off: k_pvv_sample's loop, copied (see there)
// k_pp_reduce: a lane takes the rays lane, lane + 64, ... of its probe and keeps a count and three (dist, r) keys; the wave combines
// them by a butterfly of lane exchanges.  A key order is total - (dist, r) with r unique, and dist is never a NaN (minNum with a finite
// max_distance) -, and the count is an integer sum, so the result does not depend on the combining order.
// Ordinary loads and stores, workgroup barriers in the compaction alone, no global atomics and no inline assembly.  No index is
// formed from a value that has not been clamped or compared: a ray index comes from a lane's own loop counter, a probe index from
// the list the scatter wrote.
#pragma once
#define HJ_PROBE_UPDATE_NO_KERNELS   // the functions of hj_probe_update.h (and through it of hj_probe_vis.h and hj_probes.h), no kernel of theirs
#include "hj_probe_update.h"
#include "hj_compact.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kPpThreads = 256u;            // threads of a k_pp_* workgroup (4 waves): a compaction tile, four probes of k_pp_reduce
constexpr uint32_t kPpNone = 0xFFFFFFFFu;        // the ray of a key that no ray has set

struct PpStep {
  float min_front, share, max_offset;            // hj_probe_place's min_front_distance, backface_share, max_offset
  uint32_t flags;                                // HJ_PROBE_PLACE_NO_RELOCATE 1, _NO_CLASSIFY 2
};

HJ_DEV v3 pp_position(const PvGrid& g, uint32_t p, float4 pl) {
  const v3 P = pvv_position(g, p);
  return V(P.x + pl.x, P.y + pl.y, P.z + pl.z);
}

// rays: count records of two float4; ray i of the launch is ray r = i % R of probe list[i / R] (list == NULL: first + i / R), from its
// placed position.  placement: the window's part, probe `first` first (a listed probe lies in the window: the scatter wrote nothing else).
__global__ __launch_bounds__(kPpThreads) void k_pp_rays(PvGrid g, PvvMap v, uint32_t seed, uint32_t seed_stride, uint32_t first, const uint32_t* __restrict__ list,
                                                        const float4* __restrict__ placement, uint32_t count, float4* __restrict__ rays) {
  const uint32_t i = blockIdx.x * kPpThreads + threadIdx.x;
  if (i >= count) return;
  const uint32_t per = v.res * v.res * v.s;
  const uint32_t p = list ? list[i / per] : first + i / per;
  pvv_ray(v, seed, seed_stride, p, i % per, pp_position(g, p, placement[p - first]), rays + 2 * (size_t)i);
}

// (dist, r) keys: a beats b in the least-first order, ties to the lower ray; pp_far: the greatest-first order, ties to the lower ray
HJ_DEV bool pp_near(float da, uint32_t ra, float db, uint32_t rb) { return da < db || (da == db && ra < rb); }
HJ_DEV bool pp_far(float da, uint32_t ra, float db, uint32_t rb) { return da > db || (da == db && ra < rb); }

// rays, hits, surface: a slab's (probes * R records of 2, 1 and 4 float4: hj_trace_rays' with the surface record); placement: the
// slab's part, read and written.  Wave w of the launch has probe w; every lane of it ends with the same combined values, lane 0
// takes the step and writes the probe's float4.
__global__ __launch_bounds__(kPpThreads) void k_pp_reduce(PvGrid g, PvvMap v, PpStep st, const float4* __restrict__ rays, const float4* __restrict__ hits,
                                                          const float4* __restrict__ surface, uint32_t probes, float4* __restrict__ placement) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * (kPpThreads / 64u) + (threadIdx.x >> 6);
  if (p >= probes) return;                                             // (a whole wave: no barrier follows)
  const uint32_t R = v.res * v.res * v.s;
  const size_t base = (size_t)p * R;
  const float4 old = placement[p];
  const v3 O = V(old.x, old.y, old.z);
  uint32_t nb = 0u, seen = 0u;                                         // back rays; a front face inside the eight cells
  float cb = __builtin_inff(), cf = __builtin_inff(), ff = -__builtin_inff();
  uint32_t rb = kPpNone, rf = kPpNone, rq = kPpNone;
  for (uint32_t r = lane; r < R; r += 64u) {                           // ascending r: a lane's own ties keep the lower ray
    const float4 h = hits[base + r], r0 = rays[2 * (base + r)], r1 = rays[2 * (base + r) + 1];
    const float4 s0 = surface[4 * (base + r)], s1 = surface[4 * (base + r) + 1];
    const v3 d = V(r0.w, r1.x, r1.y), n = V(s0.w, s1.x, s1.y);
    const bool hit = __float_as_int(h.x) >= 0;
    const float dist = hit ? f_min(h.y, v.max_distance) : v.max_distance;
    const bool back = hit && dot3(d, n) > 0.0f;
    if (back) {
      nb++;
      if (pp_near(dist, r, cb, rb)) { cb = dist; rb = r; }
    } else {
      if (pp_near(dist, r, cf, rf)) { cf = dist; rf = r; }
      if (pp_far(dist, r, ff, rq)) { ff = dist; rq = r; }
      if (hit && __builtin_fabsf(O.x + d.x * h.y) <= g.spacing[0] && __builtin_fabsf(O.y + d.y * h.y) <= g.spacing[1] &&
          __builtin_fabsf(O.z + d.z * h.y) <= g.spacing[2])
        seen = 1u;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {                                   // the butterfly: every lane ends with the wave's values
    nb += (uint32_t)__shfl_xor((int)nb, o);
    seen |= (uint32_t)__shfl_xor((int)seen, o);
    float od = __shfl_xor(cb, o);
    uint32_t orr = (uint32_t)__shfl_xor((int)rb, o);
    if (pp_near(od, orr, cb, rb)) { cb = od; rb = orr; }
    od = __shfl_xor(cf, o);
    orr = (uint32_t)__shfl_xor((int)rf, o);
    if (pp_near(od, orr, cf, rf)) { cf = od; rf = orr; }
    od = __shfl_xor(ff, o);
    orr = (uint32_t)__shfl_xor((int)rq, o);
    if (pp_far(od, orr, ff, rq)) { ff = od; rq = orr; }
  }
  if (lane != 0u) return;
  const bool inside = (float)nb > st.share * (float)R;
  float4 out = old;
  if ((st.flags & 1u) == 0u) {                                         // relocation
    v3 cand = O;
    if (inside) {                                                      // (nb > 0: rb is a ray)
      const float4 r0 = rays[2 * (base + rb)], r1 = rays[2 * (base + rb) + 1];
      const float step = cb + st.min_front * 0.5f;
      cand = V(O.x + r0.w * step, O.y + r1.x * step, O.z + r1.y * step);
    } else if (rf != kPpNone && cf < st.min_front) {
      const float4 f0 = rays[2 * (base + rf)], f1 = rays[2 * (base + rf) + 1], q0 = rays[2 * (base + rq)], q1 = rays[2 * (base + rq) + 1];
      if (dot3(V(f0.w, f1.x, f1.y), V(q0.w, q1.x, q1.y)) <= 0.5f) {
        const float step = f_min(ff, st.min_front);
        cand = V(O.x + q0.w * step, O.y + q1.x * step, O.z + q1.y * step);
      }
    } else if (rf != kPpNone && cf > st.min_front) {
      const float L = len3(O);
      if (L > 0.0f) {
        const float back = f_min(cf - st.min_front, L);
        cand = V(O.x - (O.x / L) * back, O.y - (O.y / L) * back, O.z - (O.z / L) * back);
      }
    }
    if (__builtin_fabsf(cand.x) <= st.max_offset * g.spacing[0] && __builtin_fabsf(cand.y) <= st.max_offset * g.spacing[1] &&
        __builtin_fabsf(cand.z) <= st.max_offset * g.spacing[2]) {     // (a NaN compares false: the offset stays)
      out.x = cand.x; out.y = cand.y; out.z = cand.z;
    }
  }
  if ((st.flags & 2u) == 0u) out.w = __uint_as_float((!inside && seen != 0u) ? 0u : 1u);   // classification
  placement[p] = out;
}

// The window's active probes: placement, the window's part (n probes from probe `first`); tile b of kPpThreads probes.
HJ_DEV bool pp_active(const float4* __restrict__ placement, uint32_t n) {
  const uint32_t t = blockIdx.x * kPpThreads + threadIdx.x;
  return t < n && __float_as_uint(placement[t].w) == 0u;
}

__global__ __launch_bounds__(kPpThreads) void k_pp_count(const float4* __restrict__ placement, uint32_t n, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kPpThreads / 64u];
  (void)compact_wave_counts(pp_active(placement, n), wave_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = compact_tile_count<kPpThreads>(wave_cnt);
}

__global__ __launch_bounds__(kPpThreads) void k_pp_scan(uint32_t* __restrict__ counts, uint32_t nb) { compact_scan_tiles<kPpThreads>(counts, nb); }

// list: at rank offsets[tile] + the active probes of the tile before it the probe's index first + t, so the list ascends.
__global__ __launch_bounds__(kPpThreads) void k_pp_scatter(const float4* __restrict__ placement, uint32_t n, uint32_t first, const uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ list) {
  __shared__ uint32_t wave_cnt[kPpThreads / 64u];
  const bool keep = pp_active(placement, n);
  const unsigned long long mask = compact_wave_counts(keep, wave_cnt);
  if (!keep) return;
  HJ_COMPACT_RANK(pos, offsets[blockIdx.x], wave_cnt, mask);
  list[pos] = first + blockIdx.x * kPpThreads + threadIdx.x;
}

// points: m records, k_pv_points' of probe p = list[i] with the placed position in words 0-2.  placement: the window's part.
__global__ __launch_bounds__(kPpThreads) void k_pp_points(PvGrid g, uint32_t seed, uint32_t seed_stride, const uint32_t* __restrict__ list, uint32_t m,
                                                          uint32_t first, const float4* __restrict__ placement, float4* __restrict__ points) {
  const uint32_t i = blockIdx.x * kPpThreads + threadIdx.x;
  if (i >= m) return;
  const uint32_t p = list[i];
  const v3 P = pp_position(g, p, placement[p - first]);
  points[2 * (size_t)i] = make_float4(P.x, P.y, P.z, 0.0f);
  points[2 * (size_t)i + 1] = make_float4(0.0f, 0.0f, __uint_as_float(seed + p * seed_stride), __uint_as_float(p));
}

// records: 9 float4 per point; window: the records of the window's probes, probe `first` first.  The probe of record i is word 7 of
// point i (first <= p < first + the window's probes: the scatter wrote nothing else).
__global__ __launch_bounds__(kPpThreads) void k_pp_resolve(const float4* __restrict__ points, const float4* __restrict__ records, uint32_t m, uint32_t first,
                                                           float s, float min_distance, float h, float soft, float hard, float4* __restrict__ window) {
  const uint32_t i = blockIdx.x * kPpThreads + threadIdx.x;
  if (i >= m) return;
  const uint32_t p = __float_as_uint(points[2 * (size_t)i + 1].w);
  pu_resolve_probe(records + 9 * (size_t)i, s, min_distance, h, soft, hard, window + kPvVec * (size_t)(p - first));
}

// hits: the slab's (probes * res^2 * s float4); window: the atlas of the window's probes, probe `first` first; list: the slab's probes.
__global__ __launch_bounds__(kPpThreads) void k_pp_blend(PvvMap v, const float4* __restrict__ hits, const uint32_t* __restrict__ list, uint32_t probes,
                                                         uint32_t first, float h, float2* __restrict__ window) {
  const uint32_t per = v.res * v.res, T = v.res + 2u;
  const uint32_t i = blockIdx.x * kPpThreads + threadIdx.x;
  if (i >= probes * per) return;
  pu_reduce_texel(v, hits + (size_t)i * v.s, i % per, h, window + (size_t)(list[i / per] - first) * (T * T));
}

// k_pvv_sample with a placement: P = the placed position in both factors, and a corner whose probe is inactive has w = 0 (a select:
// its record may never have been written).  The cell indices and the trilinear weights stay the grid's.  The loop is a copy of
// k_pvv_sample's around pvv_corner_fetch, which both call: sharing the whole loop through a template moved that kernel from 228 to 240
// VGPRs, sharing the other two per-corner pieces too to 226 or 230 ("Probe placement"), so those stay in both texts;
// the lines that differ carry a comment, and a zero placement is tested against k_pvv_sample on bits.
__global__ __launch_bounds__(kPpThreads) void k_pp_sample(PvGrid g, PvvMap v, const float4* __restrict__ probes, const float2* __restrict__ atlas,
                                                          const float4* __restrict__ placement, const float4* __restrict__ points, uint32_t n,
                                                          float4* __restrict__ out) {
  const uint32_t stride = gridDim.x * kPpThreads;
  const bool backface = (v.flags & 2u) == 0u, chebyshev = (v.flags & 4u) == 0u;     // HJ_PROBE_VIS_NO_BACKFACE, _NO_CHEBYSHEV
  const uint32_t T = v.res + 2u;
  const float fres = (float)v.res;
  for (uint32_t i = blockIdx.x * kPpThreads + threadIdx.x; i < n; i += stride) {
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
    bool away[8];
    bool off[8];                                          // (placed) the corner's probe is inactive
#pragma unroll
    for (uint32_t c = 0; c < 8u; c++) {                  // dz outer, dy, dx inner
      const uint32_t cx = x[c & 1u], cy = y[(c >> 1) & 1u], cz = z[c >> 2];
      const uint32_t p = (cz * g.count[1] + cy) * g.count[0] + cx;
      q[c] = p * kPvVec;
      last[c] = probes[q[c] + (kPvVec - 1u)];
      const float4 pl = placement[p];                     // (placed)
      off[c] = __float_as_uint(pl.w) != 0u;
      const v3 G = pvv_position(g, cx, cy, cz);
      const v3 P = V(G.x + pl.x, G.y + pl.y, G.z + pl.z);   // (placed) one more sum per axis
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
      if (off[c]) w[c] = 0.0f;                            // (placed) a select, not a product: a NaN behind it cannot leak
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
        s3 = on ? s3 + r[c].w * w[c] : s3;
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

}  // namespace hj
