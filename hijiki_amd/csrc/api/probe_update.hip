// hj_update_probes, hj_update_probe_visibility: a window of a probe volume, or of its visibility atlas, re-baked from the uploaded
// scene under a frame's seeds and folded into the values the caller holds ("Probe updates").
//
// The kernels are kernels/hj_probe_update.h's (beside it the functions of hj_probe_vis.h and hj_probes.h without their kernels, and
// hj_num.h alone, so the path kernels' machine code does not depend on this unit).  The points, the rays and the desc checks are
// api/probe_volume.hip's and api/probe_visibility.hip's own (probe_points_enqueue, probe_vis_rays_enqueue, probe_desc_check,
// probe_vis_bake_check); the gather and the trace are hj_trace_irradiance and hj_trace_rays themselves, called with device arrays.
//   probes:      k_pv_points over the window  ->  hj_trace_irradiance (sphere, SH9)  ->  k_pu_resolve (resolve and blend, in place)
//   visibility:  per slab of the window  k_pvv_rays  ->  hj_trace_rays  ->  k_pu_reduce (moments, blend and border, in place)
// Host arrays: the window's part alone (visibility: a slab's) is staged in, updated and copied back.
#include "hj_internal.h"
#include "../kernels/hj_probe_update.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {   // for api/probe_place.hip too (hj_internal.h)
// What both entry points - and api/probe_place.hip's placed ones - refuse of an update, without a device, behind the descs' refusals
// (fn: the entry point's name; n: the volume's probes)
int probe_update_check(hj_context* ctx, const char* fn, const hj_probe_update* u, uint32_t n) {
  if (!u) return set_error(ctx, HJ_ERR_INVALID, "%s: null update", fn);
  if (u->flags != 0u) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown update flag bits 0x%x", fn, u->flags);
  if ((uint64_t)u->first_probe + u->num_probes > n)
    return set_error(ctx, HJ_ERR_INVALID, "%s: probes %u ... %llu of %u", fn, u->first_probe, (unsigned long long)u->first_probe + u->num_probes, n);
  if (!(u->hysteresis >= 0.0f && u->hysteresis < 1.0f)) return set_error(ctx, HJ_ERR_INVALID, "%s: hysteresis %g outside [0, 1)", fn, (double)u->hysteresis);
  if (!(u->change_soft >= 0.0f)) return set_error(ctx, HJ_ERR_INVALID, "%s: change_soft %g: >= 0 is needed", fn, (double)u->change_soft);
  if (!(u->change_hard >= 0.0f)) return set_error(ctx, HJ_ERR_INVALID, "%s: change_hard %g: >= 0 is needed", fn, (double)u->change_hard);
  return HJ_OK;
}
}  // namespace hjapi

namespace {

dim3 per_item(uint32_t n) { return dim3((n + hj::kPuThreads - 1u) / hj::kPuThreads); }

}  // namespace

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_bake_probes' order and style).
int hj_update_probes(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_update* upd, uint32_t spp, const hj_render_opts* opts, float* probes,
                     hj_render_stats* stats) {
  if (!desc || !probes) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probes: null %s", !desc ? "desc" : "probes");
  hj::PvGrid g{};
  uint32_t n = 0;
  HJ_TRY(probe_desc_check(ctx, __func__, desc, g, n));
  HJ_TRY(probe_update_check(ctx, __func__, upd, n));
  const bool on_device = (desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0;
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probes: spp %u outside [1, 65536]", spp);
  if (on_device && misaligned(probes)) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probes: device arrays must be 16-byte aligned");
  hj_render_opts o;
  HJ_TRY(query_render_opts(ctx, __func__, opts, o));
  HJ_TRY(query_gate(ctx, __func__));
  const uint32_t first = upd->first_probe, cnt = upd->num_probes;
  if (cnt == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::Probes& pv = ctx->probes;
  HJ_TRY(dev_alloc(ctx, pv.points, sizeof(float4) * 2 * (size_t)cnt));
  HJ_TRY(dev_alloc(ctx, pv.records, sizeof(float4) * 9 * (size_t)cnt));
  float* here = probes + HJ_PROBE_WORDS * (size_t)first;             // the window's records
  const size_t bytes = sizeof(float4) * hj::kPvVec * (size_t)cnt;
  float4* d_window = reinterpret_cast<float4*>(here);
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, pv.volume, bytes));
    d_window = static_cast<float4*>(pv.volume.p);
    if (const hipError_t e = hipMemcpyAsync(d_window, here, bytes, hipMemcpyHostToDevice, ctx->stream); e != hipSuccess) return drain(ctx, __func__, e);
  }
  // 1. the window's points under this frame's seed, 2. the gather: the same stream; it returns with its records complete
  const uint32_t seed = desc->seed + upd->frame * upd->frame_stride;
  float4 *d_points = static_cast<float4*>(pv.points.p), *d_records = static_cast<float4*>(pv.records.p);
  probe_points_enqueue(ctx, g, seed, desc->seed_stride, first, cnt, d_points);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
  const int rc = hj_trace_irradiance(ctx, reinterpret_cast<const float*>(d_points), cnt, spp, &o, probe_gather_flags(desc),
                                     reinterpret_cast<float*>(d_records), stats);
  if (rc != HJ_OK) return drain(ctx, __func__, rc);                   // (a host window's copy in: nothing of the call stays in flight)
  // 3. resolve and blend in one pass, in place
  const float s = 12.5663706f / (float)spp;
  hipLaunchKernelGGL(hj::k_pu_resolve, per_item(cnt), dim3(hj::kPuThreads), 0, ctx->stream, static_cast<const float4*>(d_records), cnt, s, desc->min_distance,
                     upd->hysteresis, upd->change_soft, upd->change_hard, d_window);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(here, d_window, bytes, hipMemcpyDeviceToHost, ctx->stream);
  return drain(ctx, __func__, e);
}

int hj_update_probe_visibility(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const hj_probe_update* upd, float* atlas) {
  if (!desc || !vis || !atlas) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probe_visibility: null %s", !desc ? "desc" : !vis ? "vis" : "atlas");
  hj::PvGrid g{};
  hj::PvvMap v{};
  uint32_t n = 0;
  HJ_TRY(probe_vis_bake_check(ctx, __func__, desc, vis, g, n, v));
  HJ_TRY(probe_update_check(ctx, __func__, upd, n));
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(atlas)) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probe_visibility: device arrays must be 16-byte aligned");
  HJ_TRY(query_gate(ctx, __func__));
  const uint32_t first = upd->first_probe, num = upd->num_probes;
  if (num == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::ProbeVis& pv = ctx->probe_vis;
  // whole probes of a slab: at most kPvvSlabRays rays (res^2 s <= 16384: at least 32 probes)
  const uint32_t per = v.res * v.res * v.s, texels = (v.res + 2u) * (v.res + 2u), slab = std::min(hj::kPvvSlabRays / per, num);
  HJ_TRY(dev_alloc(ctx, pv.rays, sizeof(float4) * 2 * (size_t)slab * per));
  HJ_TRY(dev_alloc(ctx, pv.hits, sizeof(float4) * (size_t)slab * per));
  if (!on_device) HJ_TRY(dev_alloc(ctx, pv.atlas, sizeof(float2) * (size_t)slab * texels));
  float4 *d_rays = static_cast<float4*>(pv.rays.p), *d_hits = static_cast<float4*>(pv.hits.p);
  const uint32_t seed = desc->seed + upd->frame * upd->frame_stride;
  for (uint32_t at = 0; at < num; at += slab) {
    const uint32_t cnt = std::min(slab, num - at);
    float* here = atlas + 2 * (size_t)(first + at) * texels;          // the slab's part of the atlas
    const size_t bytes = sizeof(float2) * (size_t)cnt * texels;
    float2* d_atlas = on_device ? reinterpret_cast<float2*>(here) : static_cast<float2*>(pv.atlas.p);
    // (a host-side atlas: through one slab's staging, which the previous slab's copy out has left - the same stream)
    if (!on_device)
      if (const hipError_t e = hipMemcpyAsync(d_atlas, here, bytes, hipMemcpyHostToDevice, ctx->stream); e != hipSuccess) return drain(ctx, __func__, e);
    // 1. the rays under this frame's seed, 2. the trace: the same stream; it returns with its hits complete
    probe_vis_rays_enqueue(ctx, g, v, seed, desc->seed_stride, first + at, cnt, d_rays);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
    const int rc = hj_trace_rays(ctx, reinterpret_cast<const float*>(d_rays), (size_t)cnt * per, HJ_TRACE_DEVICE_ARRAYS, reinterpret_cast<float*>(d_hits), nullptr);
    if (rc != HJ_OK) return drain(ctx, __func__, rc);
    // 3. moments, blend and border in one pass, in place
    hipLaunchKernelGGL(hj::k_pu_reduce, per_item(cnt * v.res * v.res), dim3(hj::kPuThreads), 0, ctx->stream, v, static_cast<const float4*>(d_hits), cnt,
                       upd->hysteresis, d_atlas);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(here, d_atlas, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return drain(ctx, __func__, e);
  }
  return drain(ctx, __func__, hipSuccess);
}

}  // extern "C"
