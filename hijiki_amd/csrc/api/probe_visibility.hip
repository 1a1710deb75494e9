// hj_probe_visibility_rays, hj_bake_probe_visibility, hj_sample_probes_visible: per probe of a volume an octahedral atlas of the mean
// and the mean squared distance to the nearest surface, and the look-up of a volume with the back-face and Chebyshev weights against
// light leaks ("Probe volumes").
//
// The kernels are kernels/hj_probe_vis.h's (beside it hj_probes.h, hj_sh9.h and hj_num.h alone, so the path kernels' machine code
// does not depend on this unit).  The trace of the bake is hj_trace_rays itself, called with device arrays as api/probe_volume.hip
// calls hj_trace_irradiance: nothing of its walk is restated here.
//   rays:    k_pvv_rays, a slab at a time
//   bake:    per slab  k_pvv_rays  ->  hj_trace_rays (closest hit; it returns with its hits complete)  ->  k_pvv_reduce
//   sample:  k_pvv_sample
#include "hj_internal.h"
#include "../kernels/hj_probe_vis.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

enum class Call { kRays, kBake, kSample };

// What the three entry points refuse of the two descs, without a device (fn: the entry point's name) -> g, n = the probes, v
int check_descs(hj_context* ctx, const char* fn, Call call, const hj_probe_desc* d, const hj_probe_vis_desc* vis, hj::PvGrid& g, uint32_t& n, hj::PvvMap& v) {
  HJ_TRY(probe_desc_check(ctx, fn, d, g, n));
  if (vis->flags & ~(uint32_t)(HJ_PROBE_VIS_DEVICE_ARRAYS | HJ_PROBE_VIS_NO_BACKFACE | HJ_PROBE_VIS_NO_CHEBYSHEV))
    return set_error(ctx, HJ_ERR_INVALID, "%s: unknown visibility flag bits 0x%x", fn, vis->flags);
  if (((d->flags & HJ_PROBES_DEVICE_ARRAYS) != 0) != ((vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0))
    return set_error(ctx, HJ_ERR_INVALID, "%s: HJ_PROBES_DEVICE_ARRAYS and HJ_PROBE_VIS_DEVICE_ARRAYS must agree", fn);
  if (vis->res != 4u && vis->res != 8u && vis->res != 16u) return set_error(ctx, HJ_ERR_INVALID, "%s: res %u: 4, 8 or 16 is needed", fn, vis->res);
  if (call != Call::kSample) {
    if (vis->rays_per_texel == 0 || vis->rays_per_texel > 64u)
      return set_error(ctx, HJ_ERR_INVALID, "%s: rays_per_texel %u outside [1, 64]", fn, vis->rays_per_texel);
    if (!std::isfinite(vis->max_distance) || !(vis->max_distance > 0.0f) || vis->max_distance > 1e18f)
      return set_error(ctx, HJ_ERR_INVALID, "%s: max_distance %g: finite, > 0 and at most 1e18 is needed", fn, (double)vis->max_distance);
  } else if (!std::isfinite(vis->normal_bias) || vis->normal_bias < 0.0f) {
    return set_error(ctx, HJ_ERR_INVALID, "%s: normal_bias %g: finite and >= 0 is needed", fn, (double)vis->normal_bias);
  }
  v.res = vis->res;
  v.s = vis->rays_per_texel;
  v.max_distance = vis->max_distance;
  v.normal_bias = vis->normal_bias;
  v.flags = vis->flags;
  return HJ_OK;
}

dim3 per_item(uint32_t n) { return dim3((n + hj::kPvvThreads - 1u) / hj::kPvvThreads); }

// whole probes of a slab: at most kPvvSlabRays rays (res^2 s <= 16384: at least 32 probes)
uint32_t slab_probes(const hj::PvvMap& v) { return hj::kPvvSlabRays / (v.res * v.res * v.s); }

// the rays of the probes first ... first + probes - 1 (at most a slab's) under `seed`, on the context's stream
void enqueue_rays(hj_context* ctx, const hj::PvGrid& g, const hj::PvvMap& v, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t probes, float4* d_rays) {
  const uint32_t count = probes * (v.res * v.res * v.s);
  hipLaunchKernelGGL(hj::k_pvv_rays, per_item(count), dim3(hj::kPvvThreads), 0, ctx->stream, g, v, seed, seed_stride, first, count, d_rays);
}

}  // namespace

namespace hjapi {   // for api/probe_update.hip and api/probe_place.hip (hj_internal.h)
int probe_vis_bake_check(hj_context* ctx, const char* fn, const hj_probe_desc* d, const hj_probe_vis_desc* vis, hj::PvGrid& g, uint32_t& n, hj::PvvMap& v) {
  return check_descs(ctx, fn, Call::kBake, d, vis, g, n, v);
}
void probe_vis_rays_enqueue(hj_context* ctx, const hj::PvGrid& g, const hj::PvvMap& v, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t probes,
                            float4* d_rays) {
  enqueue_rays(ctx, g, v, seed, seed_stride, first, probes, d_rays);
}
// A host-side placement: the offsets of the probes first ... first + num - 1 must be finite
int probe_place_check_offsets(hj_context* ctx, const char* fn, const float* placement, uint32_t first, uint32_t num) {
  for (uint32_t p = first; p < first + num; p++)
    for (int a = 0; a < 3; a++)
      if (!std::isfinite(placement[HJ_PROBE_PLACE_WORDS * (size_t)p + a])) return set_error(ctx, HJ_ERR_INVALID, "%s: probe %u has a non-finite offset", fn, p);
  return HJ_OK;
}

// k_pvv_sample - or through `placed` k_pp_sample - over m (> 0) device points: enough workgroups to fill the device, no more than the
// points need; the kernel strides over the rest
void probe_vis_sample_enqueue(hj_context* ctx, const hj::PvGrid& g, const hj::PvvMap& v, const float4* d_probes, const float2* d_atlas, const float4* d_place,
                              const float4* d_points, uint32_t m, float4* d_out, ProbeVisSampleLaunch placed) {
  const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)m + hj::kPvvThreads - 1u) / hj::kPvvThreads, (size_t)ctx->num_cus * 8u);
  if (placed) placed(ctx->stream, blocks, g, v, d_probes, d_atlas, d_place, d_points, m, d_out);
  else hipLaunchKernelGGL(hj::k_pvv_sample, dim3(blocks), dim3(hj::kPvvThreads), 0, ctx->stream, g, v, d_probes, d_atlas, d_points, m, d_out);
}

// probe_vis_sample's refusals of the volume alone, in its order, for hj_render_probe_lit (api/probe_lit.hip), which brings the points itself
int probe_vis_volume_check(hj_context* ctx, const char* fn, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes, const float* atlas,
                           const float* placement, bool placed, bool any, hj::PvGrid& g, uint32_t& n, hj::PvvMap& v, bool& reads_atlas) {
  const uint32_t both_off = HJ_PROBE_VIS_NO_BACKFACE | HJ_PROBE_VIS_NO_CHEBYSHEV;
  reads_atlas = vis && (vis->flags & both_off) != both_off;
  const bool no_place = placed && !placement;
  if (!desc || !vis || no_place || (any && (!probes || (reads_atlas && !atlas))))
    return set_error(ctx, HJ_ERR_INVALID, "%s: null %s", fn, !desc ? "desc" : !vis ? "vis" : no_place ? "placement" : !probes ? "probes" : "atlas");
  HJ_TRY(check_descs(ctx, fn, Call::kSample, desc, vis, g, n, v));
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && any && (misaligned(probes, reads_atlas ? atlas : nullptr) || (placed && misaligned(placement))))
    return set_error(ctx, HJ_ERR_INVALID, "%s: device arrays must be 16-byte aligned", fn);
  if (!on_device && placed && any) HJ_TRY(probe_place_check_offsets(ctx, fn, placement, 0u, n));
  return HJ_OK;
}

// The host side of hj_sample_probes_visible and, with a launch of its kernel, of hj_sample_probes_visible_placed (api/probe_place.hip):
// one text of the refusals, the staging and the launch shape.  placed == nullptr: no placement (the argument is not looked at).
int probe_vis_sample(hj_context* ctx, const char* fn, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes, const float* atlas,
                     const float* points, size_t m, float* out, const float* placement, ProbeVisSampleLaunch placed) {
  const uint32_t both_off = HJ_PROBE_VIS_NO_BACKFACE | HJ_PROBE_VIS_NO_CHEBYSHEV;
  const bool reads_atlas = vis && (vis->flags & both_off) != both_off;
  const bool no_place = placed && !placement;            // (a null placement is refused whatever m is)
  if (!desc || !vis || no_place || (m != 0 && (!probes || (reads_atlas && !atlas) || !points || !out)))
    return set_error(ctx, HJ_ERR_INVALID, "%s: null %s", fn,
                     !desc ? "desc" : !vis ? "vis" : no_place ? "placement" : !probes ? "probes" : (reads_atlas && !atlas) ? "atlas" : !points ? "points" : "out");
  hj::PvGrid g{};
  hj::PvvMap v{};
  uint32_t np = 0;
  HJ_TRY(check_descs(ctx, fn, Call::kSample, desc, vis, g, np, v));
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && m != 0 && (misaligned(probes, reads_atlas ? atlas : nullptr, points, out) || (placed && misaligned(placement))))
    return set_error(ctx, HJ_ERR_INVALID, "%s: device arrays must be 16-byte aligned", fn);
  if (m > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "%s: %zu points, at most 2^31 - 1 a call", fn, m);
  if (!on_device) {                            // (device arrays: the caller's contract; the kernel clamps whatever it is given)
    for (size_t i = 0; i < m; i++) {
      const float* p = points + 8 * i;
      for (int k = 0; k < 6; k++)
        if (!std::isfinite(p[k]))
          return set_error(ctx, HJ_ERR_INVALID, "%s: point %zu has a non-finite %s", fn, i, k < 3 ? "position" : "normal");
      if (p[3] == 0.f && p[4] == 0.f && p[5] == 0.f) return set_error(ctx, HJ_ERR_INVALID, "%s: point %zu has an all-zero normal", fn, i);
    }
    if (placed && m != 0) HJ_TRY(probe_place_check_offsets(ctx, fn, placement, 0u, np));
  }
  HJ_TRY(context_gate(ctx, fn));
  if (m == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const float4 *d_probes = reinterpret_cast<const float4*>(probes), *d_points = reinterpret_cast<const float4*>(points);
  const float2* d_atlas = reads_atlas ? reinterpret_cast<const float2*>(atlas) : nullptr;
  const float4* d_place = reinterpret_cast<const float4*>(placement);
  float4* d_out = reinterpret_cast<float4*>(out);
  if (!on_device) {
    hj_context::ProbeVis& pv = ctx->probe_vis;
    const size_t atlas_bytes = sizeof(float) * HJ_PROBE_VIS_WORDS(v.res) * (size_t)np;
    HJ_TRY(dev_alloc(ctx, pv.volume, sizeof(float4) * hj::kPvVec * (size_t)np));
    if (reads_atlas) HJ_TRY(dev_alloc(ctx, pv.atlas, atlas_bytes));
    HJ_TRY(dev_alloc(ctx, pv.in_points, sizeof(float4) * 2 * m));
    HJ_TRY(dev_alloc(ctx, pv.out, sizeof(float4) * m));
    if (placed) HJ_TRY(dev_alloc(ctx, ctx->probe_place.placement, sizeof(float4) * (size_t)np));   // (the placement whole, 16 bytes a probe)
    hipError_t e = hipMemcpyAsync(pv.volume.p, probes, sizeof(float4) * hj::kPvVec * (size_t)np, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && reads_atlas) e = hipMemcpyAsync(pv.atlas.p, atlas, atlas_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pv.in_points.p, points, sizeof(float4) * 2 * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && placed) {
      e = hipMemcpyAsync(ctx->probe_place.placement.p, placement, sizeof(float4) * (size_t)np, hipMemcpyHostToDevice, s);
      d_place = static_cast<const float4*>(ctx->probe_place.placement.p);
    }
    if (e != hipSuccess) return drain(ctx, fn, e);
    d_probes = static_cast<const float4*>(pv.volume.p);
    d_atlas = reads_atlas ? static_cast<const float2*>(pv.atlas.p) : nullptr;
    d_points = static_cast<const float4*>(pv.in_points.p);
    d_out = static_cast<float4*>(pv.out.p);
  }
  probe_vis_sample_enqueue(ctx, g, v, d_probes, d_atlas, d_place, d_points, (uint32_t)m, d_out, placed);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out, d_out, sizeof(float4) * m, hipMemcpyDeviceToHost, s);
  return drain(ctx, fn, e);
}
}  // namespace hjapi

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_probe_points' order and style).
int hj_probe_visibility_rays(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, uint32_t first_probe, uint32_t num_probes, float* rays) {
  if (!desc || !vis || (num_probes != 0 && !rays))
    return set_error(ctx, HJ_ERR_INVALID, "hj_probe_visibility_rays: null %s", !desc ? "desc" : !vis ? "vis" : "rays");
  hj::PvGrid g{};
  hj::PvvMap v{};
  uint32_t n = 0;
  HJ_TRY(check_descs(ctx, __func__, Call::kRays, desc, vis, g, n, v));
  if ((uint64_t)first_probe + num_probes > n)
    return set_error(ctx, HJ_ERR_INVALID, "hj_probe_visibility_rays: probes %u ... %llu of %u", first_probe, (unsigned long long)first_probe + num_probes, n);
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && num_probes != 0 && misaligned(rays)) return set_error(ctx, HJ_ERR_INVALID, "hj_probe_visibility_rays: device arrays must be 16-byte aligned");
  HJ_TRY(context_gate(ctx, __func__));
  if (num_probes == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t per = v.res * v.res * v.s, slab = slab_probes(v);
  if (!on_device) HJ_TRY(dev_alloc(ctx, ctx->probe_vis.rays, sizeof(float4) * 2 * (size_t)std::min(slab, num_probes) * per));
  hipError_t e = hipSuccess;
  for (uint32_t at = 0; at < num_probes && e == hipSuccess; at += slab) {
    const uint32_t cnt = std::min(slab, num_probes - at);
    float* here = rays + 8 * (size_t)at * per;
    float4* d_rays = on_device ? reinterpret_cast<float4*>(here) : static_cast<float4*>(ctx->probe_vis.rays.p);
    enqueue_rays(ctx, g, v, desc->seed, desc->seed_stride, first_probe + at, cnt, d_rays);
    e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(here, d_rays, sizeof(float4) * 2 * (size_t)cnt * per, hipMemcpyDeviceToHost, ctx->stream);
  }
  return drain(ctx, __func__, e);
}

int hj_bake_probe_visibility(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, float* atlas) {
  if (!desc || !vis || !atlas) return set_error(ctx, HJ_ERR_INVALID, "hj_bake_probe_visibility: null %s", !desc ? "desc" : !vis ? "vis" : "atlas");
  hj::PvGrid g{};
  hj::PvvMap v{};
  uint32_t n = 0;
  HJ_TRY(check_descs(ctx, __func__, Call::kBake, desc, vis, g, n, v));
  const bool on_device = (vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(atlas)) return set_error(ctx, HJ_ERR_INVALID, "hj_bake_probe_visibility: device arrays must be 16-byte aligned");
  HJ_TRY(query_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::ProbeVis& pv = ctx->probe_vis;
  const uint32_t per = v.res * v.res * v.s, texels = (v.res + 2u) * (v.res + 2u), slab = std::min(slab_probes(v), n);
  HJ_TRY(dev_alloc(ctx, pv.rays, sizeof(float4) * 2 * (size_t)slab * per));
  HJ_TRY(dev_alloc(ctx, pv.hits, sizeof(float4) * (size_t)slab * per));
  if (!on_device) HJ_TRY(dev_alloc(ctx, pv.atlas, sizeof(float2) * (size_t)slab * texels));
  float4 *d_rays = static_cast<float4*>(pv.rays.p), *d_hits = static_cast<float4*>(pv.hits.p);
  for (uint32_t at = 0; at < n; at += slab) {
    const uint32_t cnt = std::min(slab, n - at);
    // 1. the rays, 2. the trace: the same stream, so it runs behind the rays; it returns with its hits complete
    enqueue_rays(ctx, g, v, desc->seed, desc->seed_stride, at, cnt, d_rays);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
    HJ_TRY(hj_trace_rays(ctx, reinterpret_cast<const float*>(d_rays), (size_t)cnt * per, HJ_TRACE_DEVICE_ARRAYS, reinterpret_cast<float*>(d_hits), nullptr));
    // 3. the moments, border included (a host-side atlas: through one slab's staging, which the copy leaves before the next slab writes it)
    float* here = atlas + 2 * (size_t)at * texels;
    float2* d_atlas = on_device ? reinterpret_cast<float2*>(here) : static_cast<float2*>(pv.atlas.p);
    hipLaunchKernelGGL(hj::k_pvv_reduce, per_item(cnt * texels), dim3(hj::kPvvThreads), 0, ctx->stream, v, static_cast<const float4*>(d_hits), cnt, d_atlas);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(here, d_atlas, sizeof(float2) * (size_t)cnt * texels, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return drain(ctx, __func__, e);
  }
  return drain(ctx, __func__, hipSuccess);
}

int hj_sample_probes_visible(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes, const float* atlas,
                             const float* points, size_t m, float* out) {
  return probe_vis_sample(ctx, __func__, desc, vis, probes, atlas, points, m, out, nullptr, nullptr);
}

}  // extern "C"
