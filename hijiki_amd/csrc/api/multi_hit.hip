// hj_trace_rays_all, hj_points_inside: every hit along caller-given rays - the K nearest in order, their number, the signed sum of
// their crossings - and containment of points by that sum ("All-hit queries").
//
// The kernels are kernels/hj_multihit.h's (beside it hj_intersect.h for the shape tests and the scene's records, and hj_num.h): this
// unit includes the existing kernel headers and edits none, and no other unit's machine code depends on it.
//   rays:    k_mh_walk<LIST>, one lane per ray, over the second copy of the uploaded tree; LIST = (max_hits > 0)
//   points:  k_mh_inside<PARITY>, one lane per point, three counting walks and the vote
// Host arrays are staged in chunks of HJ_TRACE_CHUNK through hj_context::AllHits; device arrays are used in place.
#include "hj_internal.h"
#include "../kernels/hj_multihit.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

dim3 per_lane(uint32_t n) { return dim3((n + hj::kBlockThreads - 1u) / hj::kBlockThreads); }

}  // namespace

extern "C" {

// The argument checks come first, in hj_trace_rays' style, and need neither a device nor a context's state; then the queries' gate.
int hj_trace_rays_all(hj_context* ctx, const float* rays, size_t n, uint32_t max_hits, uint32_t flags, uint32_t* counts, float* hits) {
  if (n != 0 && (!rays || !counts)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: null %s", !rays ? "rays" : "counts");
  if (n != 0 && max_hits != 0 && !hits) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: null hits with max_hits %u", max_hits);
  if (max_hits > HJ_ALLHITS_MAX_HITS) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: max_hits %u, at most %u", max_hits, HJ_ALLHITS_MAX_HITS);
  if (flags & ~(uint32_t)HJ_ALLHITS_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_ALLHITS_DEVICE_ARRAYS) != 0;
  if (n != 0) {
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: %zu rays, at most 2^31 - 1 a call", n);
    if (on_device && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(counts) | (max_hits ? reinterpret_cast<uintptr_t>(hits) : 0u)) & 15u) != 0)
      return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const size_t chunk = (size_t)ctx->tuning.trace_chunk, most = std::min(n, chunk), f4 = sizeof(float4), K = max_hits;
  hj_context::AllHits& q = ctx->allhits;
  float4 *d_rays = nullptr, *d_hits = nullptr;
  uint2* d_counts = nullptr;
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, q.rays, most * 2 * f4));
    HJ_TRY(dev_alloc(ctx, q.counts, most * sizeof(uint2)));
    if (K) HJ_TRY(dev_alloc(ctx, q.hits, most * K * f4));
    d_rays = static_cast<float4*>(q.rays.p); d_counts = static_cast<uint2*>(q.counts.p);
    d_hits = K ? static_cast<float4*>(q.hits.p) : nullptr;
  }
  const dim3 blk(hj::kBlockThreads);
  hipError_t e = hipSuccess;
  for (size_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t cnt = (uint32_t)std::min(chunk, n - at);
    if (on_device) {
      d_rays = reinterpret_cast<float4*>(const_cast<float*>(rays)) + 2 * at;
      d_counts = reinterpret_cast<uint2*>(counts) + at;
      d_hits = K ? reinterpret_cast<float4*>(hits) + K * at : nullptr;
    } else {
      e = hipMemcpyAsync(d_rays, rays + 8 * at, cnt * 2 * f4, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) break;
    }
    if (K) hipLaunchKernelGGL(hj::k_mh_walk<true>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, static_cast<const float4*>(d_rays), cnt, max_hits, d_counts, d_hits);
    else hipLaunchKernelGGL(hj::k_mh_walk<false>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, static_cast<const float4*>(d_rays), cnt, 0u, d_counts, d_hits);
    e = hipGetLastError();
    if (!on_device) {
      if (e == hipSuccess) e = hipMemcpyAsync(counts + 2 * at, d_counts, cnt * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && K) e = hipMemcpyAsync(hits + 4 * K * at, d_hits, cnt * K * f4, hipMemcpyDeviceToHost, ctx->stream);
    }
  }
  return drain(ctx, __func__, e);
}

int hj_points_inside(hj_context* ctx, const float* points, size_t n, uint32_t flags, uint32_t* out) {
  if (n != 0 && (!points || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: null %s", !points ? "points" : "out");
  if (flags & ~(uint32_t)(HJ_INSIDE_DEVICE_ARRAYS | HJ_INSIDE_PARITY)) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_INSIDE_DEVICE_ARRAYS) != 0, parity = (flags & HJ_INSIDE_PARITY) != 0;
  if (n != 0) {
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: %zu points, at most 2^31 - 1 a call", n);
    if (on_device && ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0)
      return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const size_t chunk = (size_t)ctx->tuning.trace_chunk, most = std::min(n, chunk), f4 = sizeof(float4);
  hj_context::AllHits& q = ctx->allhits;
  float4* d_points = nullptr;
  uint2* d_out = nullptr;
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, q.rays, most * f4));
    HJ_TRY(dev_alloc(ctx, q.counts, most * sizeof(uint2)));
    d_points = static_cast<float4*>(q.rays.p); d_out = static_cast<uint2*>(q.counts.p);
  }
  const dim3 blk(hj::kBlockThreads);
  hipError_t e = hipSuccess;
  for (size_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t cnt = (uint32_t)std::min(chunk, n - at);
    if (on_device) {
      d_points = reinterpret_cast<float4*>(const_cast<float*>(points)) + at;
      d_out = reinterpret_cast<uint2*>(out) + at;
    } else {
      e = hipMemcpyAsync(d_points, points + 4 * at, cnt * f4, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) break;
    }
    if (parity) hipLaunchKernelGGL(hj::k_mh_inside<true>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, static_cast<const float4*>(d_points), cnt, d_out);
    else hipLaunchKernelGGL(hj::k_mh_inside<false>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, static_cast<const float4*>(d_points), cnt, d_out);
    e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out + 2 * at, d_out, cnt * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream);
  }
  return drain(ctx, __func__, e);
}

}  // extern "C"
