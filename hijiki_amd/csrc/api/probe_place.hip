// hj_place_probes, hj_update_probes_placed, hj_update_probe_visibility_placed, hj_sample_probes_visible_placed: per probe an offset
// from its grid point and an active / inactive state, found from the uploaded scene, and the updates and the look-up that read them
// ("Probe placement").
//
// The kernels are kernels/hj_probe_place.h's (beside it the functions of hj_probe_update.h, hj_probe_vis.h and hj_probes.h without
// their kernels, hj_compact.h and hj_num.h alone, so the path kernels' machine code does not depend on this unit).  The desc checks are
// api/probe_volume.hip's and api/probe_visibility.hip's own (probe_desc_check, probe_vis_bake_check), the update's api/probe_update.hip's
// (probe_update_check); the gather and the trace are
// hj_trace_irradiance and hj_trace_rays themselves, called with device arrays.
//   place:       per slab of the window  k_pp_rays  ->  hj_trace_rays (closest hit, with the surface)  ->  k_pp_reduce (in place)
//   probes:      k_pp_count -> k_pp_scan -> (the count to the host) -> k_pp_scatter -> k_pp_points  ->  hj_trace_irradiance  ->  k_pp_resolve
//   visibility:  the same list, then per slab of it  k_pp_rays  ->  hj_trace_rays  ->  k_pp_blend
//   sample:      hj_sample_probes_visible's host side (probe_vis_sample) with k_pp_sample
// Host arrays: the window's part (the look-up: the whole) of the placement, the volume or the atlas is staged in, updated and copied back.
#include "hj_internal.h"
#include "../kernels/hj_probe_place.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

constexpr uint32_t kPlaceWords = HJ_PROBE_PLACE_WORDS;

dim3 per_item(uint32_t n) { return dim3((n + hj::kPpThreads - 1u) / hj::kPpThreads); }

// The window's part of the placement on the device: the caller's own (device arrays) or a staged copy, enqueued -> d_place
int stage_placement(hj_context* ctx, const char* fn, const float* placement, uint32_t first, uint32_t num, bool on_device, const float4*& d_place) {
  const float* here = placement + kPlaceWords * (size_t)first;
  d_place = reinterpret_cast<const float4*>(here);
  if (on_device) return HJ_OK;
  HJ_TRY(dev_alloc(ctx, ctx->probe_place.placement, sizeof(float4) * (size_t)num));
  d_place = static_cast<const float4*>(ctx->probe_place.placement.p);
  if (const hipError_t e = hipMemcpyAsync(ctx->probe_place.placement.p, here, sizeof(float4) * (size_t)num, hipMemcpyHostToDevice, ctx->stream); e != hipSuccess)
    return drain(ctx, fn, e);
  return HJ_OK;
}

// The window's active probes in order -> d_list (in a buffer the context keeps) and their number, which comes to the host: it sizes
// the gather and the slabs.  One synchronisation.
int active_list(hj_context* ctx, const char* fn, const float4* d_place, uint32_t first, uint32_t num, const uint32_t*& d_list, uint32_t& active) {
  hj_context::ProbePlace& pp = ctx->probe_place;
  const uint32_t nb = (num + hj::kPpThreads - 1u) / hj::kPpThreads;
  HJ_TRY(dev_alloc(ctx, pp.counts, sizeof(uint32_t) * ((size_t)nb + 1u)));
  HJ_TRY(dev_alloc(ctx, pp.list, sizeof(uint32_t) * (size_t)num));
  uint32_t *d_counts = static_cast<uint32_t*>(pp.counts.p), *list = static_cast<uint32_t*>(pp.list.p);
  hipLaunchKernelGGL(hj::k_pp_count, dim3(nb), dim3(hj::kPpThreads), 0, ctx->stream, d_place, num, d_counts);
  hipLaunchKernelGGL(hj::k_pp_scan, dim3(1), dim3(hj::kPpThreads), 0, ctx->stream, d_counts, nb);
  hipLaunchKernelGGL(hj::k_pp_scatter, dim3(nb), dim3(hj::kPpThreads), 0, ctx->stream, d_place, num, first, static_cast<const uint32_t*>(d_counts), list);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&active, d_counts + nb, sizeof active, hipMemcpyDeviceToHost, ctx->stream);
  HJ_TRY(drain(ctx, fn, e));
  d_list = list;
  return HJ_OK;
}

// hj_sample_probes_visible_placed's kernel, for the look-up's shared host side
void launch_placed_sample(hipStream_t s, uint32_t blocks, const hj::PvGrid& g, const hj::PvvMap& v, const float4* d_probes, const float2* d_atlas,
                          const float4* d_place, const float4* d_points, uint32_t m, float4* d_out) {
  static_assert(hj::kPpThreads == hj::kPvvThreads, "the look-up's host side sizes the launch for both kernels");
  hipLaunchKernelGGL(hj::k_pp_sample, dim3(blocks), dim3(hj::kPpThreads), 0, s, g, v, d_probes, d_atlas, d_place, d_points, m, d_out);
}

}  // namespace

namespace hjapi {   // for api/probe_lit.hip (hj_internal.h)
void probe_place_sample_launch(hipStream_t s, uint32_t blocks, const hj::PvGrid& g, const hj::PvvMap& v, const float4* d_probes, const float2* d_atlas,
                               const float4* d_place, const float4* d_points, uint32_t m, float4* d_out) {
  launch_placed_sample(s, blocks, g, v, d_probes, d_atlas, d_place, d_points, m, d_out);
}
}  // namespace hjapi

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_update_probe_visibility's order and style).
int hj_place_probes(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const hj_probe_place* place, float* placement) {
  if (!desc || !vis || !placement) return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: null %s", !desc ? "desc" : !vis ? "vis" : "placement");
  hj::PvGrid g{};
  hj::PvvMap v{};
  uint32_t n = 0;
  HJ_TRY(probe_vis_bake_check(ctx, __func__, desc, vis, g, n, v));
  if (!place) return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: null place");
  if (place->flags & ~(uint32_t)(HJ_PROBE_PLACE_NO_RELOCATE | HJ_PROBE_PLACE_NO_CLASSIFY))
    return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: unknown place flag bits 0x%x", place->flags);
  if ((uint64_t)place->first_probe + place->num_probes > n)
    return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: probes %u ... %llu of %u", place->first_probe,
                     (unsigned long long)place->first_probe + place->num_probes, n);
  if (!std::isfinite(place->min_front_distance) || !(place->min_front_distance > 0.0f))
    return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: min_front_distance %g: finite and > 0 is needed", (double)place->min_front_distance);
  if (!(place->backface_share >= 0.0f && place->backface_share <= 1.0f))
    return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: backface_share %g outside [0, 1]", (double)place->backface_share);
  if (!(place->max_offset >= 0.0f && place->max_offset < 0.5f))
    return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: max_offset %g outside [0, 0.5)", (double)place->max_offset);
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(placement)) return set_error(ctx, HJ_ERR_INVALID, "hj_place_probes: device arrays must be 16-byte aligned");
  const uint32_t first = place->first_probe, num = place->num_probes;
  if (!on_device) HJ_TRY(probe_place_check_offsets(ctx, __func__, placement, first, num));
  HJ_TRY(query_gate(ctx, __func__));
  if (num == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::ProbeVis& pv = ctx->probe_vis;
  // whole probes of a slab: at most kPvvSlabRays rays (res^2 s <= 16384: at least 32 probes)
  const uint32_t per = v.res * v.res * v.s, slab = std::min(hj::kPvvSlabRays / per, num);
  HJ_TRY(dev_alloc(ctx, pv.rays, sizeof(float4) * 2 * (size_t)slab * per));
  HJ_TRY(dev_alloc(ctx, pv.hits, sizeof(float4) * (size_t)slab * per));
  HJ_TRY(dev_alloc(ctx, ctx->probe_place.surface, sizeof(float4) * 4 * (size_t)slab * per));
  if (!on_device) HJ_TRY(dev_alloc(ctx, ctx->probe_place.placement, sizeof(float4) * (size_t)slab));
  float4 *d_rays = static_cast<float4*>(pv.rays.p), *d_hits = static_cast<float4*>(pv.hits.p), *d_surface = static_cast<float4*>(ctx->probe_place.surface.p);
  const uint32_t seed = desc->seed + place->frame * place->frame_stride;
  const hj::PpStep st{place->min_front_distance, place->backface_share, place->max_offset, place->flags};
  for (uint32_t at = 0; at < num; at += slab) {
    const uint32_t cnt = std::min(slab, num - at);
    float* here = placement + kPlaceWords * (size_t)(first + at);        // the slab's part of the placement
    const size_t bytes = sizeof(float4) * (size_t)cnt;
    float4* d_place = on_device ? reinterpret_cast<float4*>(here) : static_cast<float4*>(ctx->probe_place.placement.p);
    if (!on_device)
      if (const hipError_t e = hipMemcpyAsync(d_place, here, bytes, hipMemcpyHostToDevice, ctx->stream); e != hipSuccess) return drain(ctx, __func__, e);
    // 1. the rays from the placed positions under this frame's seed, 2. the trace: the same stream; it returns with its records complete
    hipLaunchKernelGGL(hj::k_pp_rays, per_item(cnt * per), dim3(hj::kPpThreads), 0, ctx->stream, g, v, seed, desc->seed_stride, first + at,
                       static_cast<const uint32_t*>(nullptr), static_cast<const float4*>(d_place), cnt * per, d_rays);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
    const int rc = hj_trace_rays(ctx, reinterpret_cast<const float*>(d_rays), (size_t)cnt * per, HJ_TRACE_DEVICE_ARRAYS, reinterpret_cast<float*>(d_hits),
                                 reinterpret_cast<float*>(d_surface));
    if (rc != HJ_OK) return drain(ctx, __func__, rc);
    // 3. one wave per probe: the reductions, the step and the state, in place
    hipLaunchKernelGGL(hj::k_pp_reduce, dim3((cnt + hj::kPpThreads / 64u - 1u) / (hj::kPpThreads / 64u)), dim3(hj::kPpThreads), 0, ctx->stream, g, v, st,
                       static_cast<const float4*>(d_rays), static_cast<const float4*>(d_hits), static_cast<const float4*>(d_surface), cnt, d_place);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(here, d_place, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return drain(ctx, __func__, e);
  }
  return drain(ctx, __func__, hipSuccess);
}

int hj_update_probes_placed(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_update* upd, uint32_t spp, const hj_render_opts* opts,
                            const float* placement, float* probes, hj_render_stats* stats) {
  if (!desc || !placement || !probes)
    return set_error(ctx, HJ_ERR_INVALID, "hj_update_probes_placed: null %s", !desc ? "desc" : !placement ? "placement" : "probes");
  hj::PvGrid g{};
  uint32_t n = 0;
  HJ_TRY(probe_desc_check(ctx, __func__, desc, g, n));
  HJ_TRY(probe_update_check(ctx, __func__, upd, n));
  const bool on_device = (desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0;
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probes_placed: spp %u outside [1, 65536]", spp);
  if (on_device && misaligned(probes, placement)) return set_error(ctx, HJ_ERR_INVALID, "hj_update_probes_placed: device arrays must be 16-byte aligned");
  hj_render_opts o;
  HJ_TRY(query_render_opts(ctx, __func__, opts, o));
  const uint32_t first = upd->first_probe, cnt = upd->num_probes;
  if (!on_device) HJ_TRY(probe_place_check_offsets(ctx, __func__, placement, first, cnt));
  HJ_TRY(query_gate(ctx, __func__));
  if (cnt == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  // 1. the window's active probes; their number sizes everything behind it
  const float4* d_place = nullptr;
  const uint32_t* d_list = nullptr;
  uint32_t m = 0;
  HJ_TRY(stage_placement(ctx, __func__, placement, first, cnt, on_device, d_place));
  HJ_TRY(active_list(ctx, __func__, d_place, first, cnt, d_list, m));
  if (m == 0) return HJ_OK;                                            // every probe of the window is inactive: nothing is traced or written
  hj_context::Probes& pv = ctx->probes;
  HJ_TRY(dev_alloc(ctx, pv.points, sizeof(float4) * 2 * (size_t)m));
  HJ_TRY(dev_alloc(ctx, pv.records, sizeof(float4) * 9 * (size_t)m));
  float* here = probes + HJ_PROBE_WORDS * (size_t)first;             // the window's records
  const size_t bytes = sizeof(float4) * hj::kPvVec * (size_t)cnt;
  float4* d_window = reinterpret_cast<float4*>(here);
  if (!on_device) {                                                    // (an inactive probe's record travels in and out untouched)
    HJ_TRY(dev_alloc(ctx, pv.volume, bytes));
    d_window = static_cast<float4*>(pv.volume.p);
    if (const hipError_t e = hipMemcpyAsync(d_window, here, bytes, hipMemcpyHostToDevice, ctx->stream); e != hipSuccess) return drain(ctx, __func__, e);
  }
  // 2. the active probes' points at their placed positions under this frame's seed, 3. the gather over them
  const uint32_t seed = desc->seed + upd->frame * upd->frame_stride;
  float4 *d_points = static_cast<float4*>(pv.points.p), *d_records = static_cast<float4*>(pv.records.p);
  hipLaunchKernelGGL(hj::k_pp_points, per_item(m), dim3(hj::kPpThreads), 0, ctx->stream, g, seed, desc->seed_stride, d_list, m, first, d_place, d_points);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
  const int rc = hj_trace_irradiance(ctx, reinterpret_cast<const float*>(d_points), m, spp, &o, probe_gather_flags(desc),
                                     reinterpret_cast<float*>(d_records), stats);
  if (rc != HJ_OK) return drain(ctx, __func__, rc);
  // 4. resolve and blend in one pass, in place: the record of point i is the one its word 7 names
  const float s = 12.5663706f / (float)spp;
  hipLaunchKernelGGL(hj::k_pp_resolve, per_item(m), dim3(hj::kPpThreads), 0, ctx->stream, static_cast<const float4*>(d_points),
                     static_cast<const float4*>(d_records), m, first, s, desc->min_distance, upd->hysteresis, upd->change_soft, upd->change_hard, d_window);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(here, d_window, bytes, hipMemcpyDeviceToHost, ctx->stream);
  return drain(ctx, __func__, e);
}

int hj_update_probe_visibility_placed(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const hj_probe_update* upd,
                                      const float* placement, float* atlas) {
  if (!desc || !vis || !placement || !atlas)
    return set_error(ctx, HJ_ERR_INVALID, "hj_update_probe_visibility_placed: null %s", !desc ? "desc" : !vis ? "vis" : !placement ? "placement" : "atlas");
  hj::PvGrid g{};
  hj::PvvMap v{};
  uint32_t n = 0;
  HJ_TRY(probe_vis_bake_check(ctx, __func__, desc, vis, g, n, v));
  HJ_TRY(probe_update_check(ctx, __func__, upd, n));
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(atlas, placement))
    return set_error(ctx, HJ_ERR_INVALID, "hj_update_probe_visibility_placed: device arrays must be 16-byte aligned");
  const uint32_t first = upd->first_probe, num = upd->num_probes;
  if (!on_device) HJ_TRY(probe_place_check_offsets(ctx, __func__, placement, first, num));
  HJ_TRY(query_gate(ctx, __func__));
  if (num == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const float4* d_place = nullptr;
  const uint32_t* d_list = nullptr;
  uint32_t m = 0;
  HJ_TRY(stage_placement(ctx, __func__, placement, first, num, on_device, d_place));
  HJ_TRY(active_list(ctx, __func__, d_place, first, num, d_list, m));
  if (m == 0) return HJ_OK;
  hj_context::ProbeVis& pv = ctx->probe_vis;
  // whole probes of a slab, cut from the list: at most kPvvSlabRays rays
  const uint32_t per = v.res * v.res * v.s, texels = (v.res + 2u) * (v.res + 2u), slab = std::min(hj::kPvvSlabRays / per, m);
  HJ_TRY(dev_alloc(ctx, pv.rays, sizeof(float4) * 2 * (size_t)slab * per));
  HJ_TRY(dev_alloc(ctx, pv.hits, sizeof(float4) * (size_t)slab * per));
  float* here = atlas + 2 * (size_t)first * texels;                   // the window's part of the atlas
  const size_t bytes = sizeof(float2) * (size_t)num * texels;
  float2* d_window = reinterpret_cast<float2*>(here);
  if (!on_device) {                                                    // (a slab's listed probes lie anywhere in the window: it is staged whole)
    HJ_TRY(dev_alloc(ctx, pv.atlas, bytes));
    d_window = static_cast<float2*>(pv.atlas.p);
    if (const hipError_t e = hipMemcpyAsync(d_window, here, bytes, hipMemcpyHostToDevice, ctx->stream); e != hipSuccess) return drain(ctx, __func__, e);
  }
  float4 *d_rays = static_cast<float4*>(pv.rays.p), *d_hits = static_cast<float4*>(pv.hits.p);
  const uint32_t seed = desc->seed + upd->frame * upd->frame_stride;
  for (uint32_t at = 0; at < m; at += slab) {
    const uint32_t cnt = std::min(slab, m - at);
    hipLaunchKernelGGL(hj::k_pp_rays, per_item(cnt * per), dim3(hj::kPpThreads), 0, ctx->stream, g, v, seed, desc->seed_stride, first, d_list + at, d_place,
                       cnt * per, d_rays);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
    const int rc = hj_trace_rays(ctx, reinterpret_cast<const float*>(d_rays), (size_t)cnt * per, HJ_TRACE_DEVICE_ARRAYS, reinterpret_cast<float*>(d_hits), nullptr);
    if (rc != HJ_OK) return drain(ctx, __func__, rc);
    hipLaunchKernelGGL(hj::k_pp_blend, per_item(cnt * v.res * v.res), dim3(hj::kPpThreads), 0, ctx->stream, v, static_cast<const float4*>(d_hits), d_list + at, cnt,
                       first, upd->hysteresis, d_window);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
  }
  hipError_t e = hipSuccess;
  if (!on_device) e = hipMemcpyAsync(here, d_window, bytes, hipMemcpyDeviceToHost, ctx->stream);
  return drain(ctx, __func__, e);
}

int hj_sample_probes_visible_placed(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes, const float* atlas,
                                    const float* points, size_t m, const float* placement, float* out) {
  // hj_sample_probes_visible's own host side (api/probe_visibility.hip), with the placement's checks and staging and this unit's kernel
  return probe_vis_sample(ctx, __func__, desc, vis, probes, atlas, points, m, out, placement, launch_placed_sample);
}

}  // extern "C"
