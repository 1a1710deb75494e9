// Probe updates ("Probe updates"): a window of a probe volume, or of its visibility atlas, re-baked under a frame's seeds
// and folded into the values the caller holds - the hysteresis of Majercik et al. 2019.  include/hijiki_hip.h (hj_update_probes,
// hj_update_probe_visibility) spells the arithmetic out; every operation here is float32, one rounding each, uncontracted, in that
// order.  The fresh values are the bakes' own texts: pv_resolve_record (hj_probes.h), pvv_moments and pvv_border_source
// (hj_probe_vis.h); neither header's kernels are compiled here.
//   pu_blend      THE text of one blend: old * hh + fresh * (1 - hh), the fresh value itself at hh == 0
//   pu_resolve_probe, pu_reduce_texel  THE texts of the two kernels' threads, for them and for hj_probe_place.h's placed kernels, which
//                 find their probe through a list (the kernels are left out under HJ_PROBE_UPDATE_NO_KERNELS)
//   k_pu_resolve  one thread per probe of the window: the gather's record resolved and blended into the probe's record in place
//   k_pu_reduce   one thread per INTERIOR texel of a slab's probes: its rays' moments blended into the texel in place, and the result
//                 written to every border texel that copies it
// The in-place hazard of k_pu_reduce: a border texel's new value is the new value of an interior texel, which needs that texel's OLD
// value, and the interior texel is overwritten in the same launch.  Chosen here: the thread of an interior texel is the only one that
// reads or writes that texel and the only one that writes its border copies (an edge texel has one, a corner texel three), so no
// value is read after another thread wrote it and no barrier is needed.  k_pu_resolve has no such hazard: a thread reads and writes
// its own probe's record.
// Ordinary loads and stores, no LDS, no atomics and no inline assembly.
#pragma once
#define HJ_PROBE_VIS_NO_KERNELS      // the functions of hj_probe_vis.h (and through it of hj_probes.h, without k_pv_sample)
#include "hj_probe_vis.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kPuThreads = 256u;   // threads of a k_pu_* workgroup (4 waves)

// hh == 0: the fresh value whatever the old one holds (a NaN included); g = 1.0f - hh, formed once by the caller.
HJ_DEV float pu_blend(float o, float f, float hh, float g) { return (hh == 0.0f) ? f : o * hh + f * g; }

// records: 9 float4 per probe of the window, hj_trace_irradiance's with HJ_GATHER_SH9; probes: the window's records, kPvVec float4
// each, read and written.  F = pv_resolve_record; O the old record.  keep = O[27] > 0 && F[27] > 0 (a NaN compares false); without
// it hh = 0.  Otherwise d = max |F[c] - O[c]| and m = max |O[c]| over the constant band's three channels, hh = h, 0 if d > hard * m,
// else max(h - 0.15f, 0) if d > soft * m.  Word k < 27: pu_blend(O[k], F[k], hh); word 27: F[27].
// (THE text of a thread: record, the probe's 9 float4 of the gather; rec, its kPvVec float4 in the volume.)
HJ_DEV void pu_resolve_probe(const float4* __restrict__ record, float s, float min_distance, float h, float soft, float hard, float4* __restrict__ rec) {
  float o[28], f[28];
#pragma unroll
  for (uint32_t m = 0; m < kPvVec; m++) {
    const float4 t = rec[m];
    o[4 * m] = t.x; o[4 * m + 1] = t.y; o[4 * m + 2] = t.z; o[4 * m + 3] = t.w;
  }
  pv_resolve_record(record, s, min_distance, f);
  float hh = 0.0f;
  if (o[27] > 0.0f && f[27] > 0.0f) {
    const float d = f_max(f_max(__builtin_fabsf(f[0] - o[0]), __builtin_fabsf(f[1] - o[1])), __builtin_fabsf(f[2] - o[2]));
    const float m = f_max(f_max(__builtin_fabsf(o[0]), __builtin_fabsf(o[1])), __builtin_fabsf(o[2]));
    hh = h;
    if (d > hard * m) hh = 0.0f;
    else if (d > soft * m) hh = f_max(h - 0.15f, 0.0f);
  }
  const float g = 1.0f - hh;
#pragma unroll
  for (uint32_t k = 0; k < 27u; k++) f[k] = pu_blend(o[k], f[k], hh, g);
#pragma unroll
  for (uint32_t m = 0; m < kPvVec; m++) rec[m] = make_float4(f[4 * m], f[4 * m + 1], f[4 * m + 2], f[4 * m + 3]);
}

// hits: hj_trace_rays' records of the slab's rays (probes * res^2 * s float4); atlas: the slab's part, probes * (res + 2)^2 float2,
// read and written.  Thread i: interior texel t = i % res^2 of probe i / res^2.  Its border copies are the inverse of
// pvv_border_source: row 0 mirrors interior row 0 in x and row T - 1 the last row (border x = res - tx), column 0 mirrors interior
// column 0 in y and column T - 1 the last column (border y = res - ty), a corner is the diagonally opposite interior corner.
// (THE text of a thread: h4, the v.s hit records of interior texel t's rays; map, the probe's (res + 2)^2 float2.)
HJ_DEV void pu_reduce_texel(const PvvMap& v, const float4* __restrict__ h4, uint32_t t, float h, float2* __restrict__ map) {
  const uint32_t res = v.res, T = res + 2u, last = res - 1u;
  const uint32_t tx = t % res, ty = t / res;
  const float2 fr = pvv_moments(v, h4);
  const float2 old = map[(ty + 1u) * T + (tx + 1u)];
  const float g = 1.0f - h;
  const float2 nv = make_float2(pu_blend(old.x, fr.x, h, g), pu_blend(old.y, fr.y, h, g));
  map[(ty + 1u) * T + (tx + 1u)] = nv;
  const bool x0 = tx == 0u, x1 = tx == last, y0 = ty == 0u, y1 = ty == last;
  if (y0) map[res - tx] = nv;                                   // border (res - tx, 0)
  if (y1) map[(T - 1u) * T + (res - tx)] = nv;                  // border (res - tx, T - 1)
  if (x0) map[(res - ty) * T] = nv;                             // border (0, res - ty)
  if (x1) map[(res - ty) * T + (T - 1u)] = nv;                  // border (T - 1, res - ty)
  if ((x0 || x1) && (y0 || y1)) map[(y0 ? T - 1u : 0u) * T + (x0 ? T - 1u : 0u)] = nv;   // the diagonally opposite corner of the border
}

#ifndef HJ_PROBE_UPDATE_NO_KERNELS   // (hj_probe_place.h takes the functions above and leaves the kernels to api/probe_update.hip)
__global__ __launch_bounds__(kPuThreads) void k_pu_resolve(const float4* __restrict__ records, uint32_t n, float s, float min_distance, float h, float soft,
                                                          float hard, float4* __restrict__ probes) {
  const uint32_t i = blockIdx.x * kPuThreads + threadIdx.x;
  if (i >= n) return;
  pu_resolve_probe(records + 9 * (size_t)i, s, min_distance, h, soft, hard, probes + kPvVec * (size_t)i);
}

__global__ __launch_bounds__(kPuThreads) void k_pu_reduce(PvvMap v, const float4* __restrict__ hits, uint32_t probes, float h, float2* __restrict__ atlas) {
  const uint32_t per = v.res * v.res, T = v.res + 2u;
  const uint32_t i = blockIdx.x * kPuThreads + threadIdx.x;
  if (i >= probes * per) return;
  pu_reduce_texel(v, hits + (size_t)i * v.s, i % per, h, atlas + (size_t)(i / per) * (T * T));
}
#endif  // HJ_PROBE_UPDATE_NO_KERNELS

}  // namespace hj
