// hj_trace_rays_all, hj_points_inside: every hit along caller-given rays - the K nearest in order, their number, the signed sum of
// their crossings - and containment of points by that sum ("All-hit queries").
//
// The kernels are kernels/hj_multihit.h's (beside it hj_intersect.h for the shape tests and the scene's records, and hj_num.h): this
// unit includes the existing kernel headers and edits none, and no other unit's machine code depends on it.
//   rays:    k_mh_walk<LIST>, one lane per ray, over the second copy of the uploaded tree; LIST = (max_hits > 0)
//   points:  k_mh_inside<PARITY>, one lane per point, three counting walks and the vote
// The chunks and the staging of host arrays through hj_context::AllHits are chunked_query's (api/hj_internal.h).
#include "hj_internal.h"
#include "../kernels/hj_multihit.h"

#pragma clang fp contract(off)

using namespace hjapi;

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
    if (on_device && misaligned(rays, counts, max_hits ? hits : nullptr))
      return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays_all: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  hj_context::AllHits& q = ctx->allhits;
  const size_t f4 = sizeof(float4);
  const QueryArray arrays[] = {{rays, &q.rays, 2 * f4, false}, {counts, &q.counts, sizeof(uint2), true}, {hits, &q.hits, max_hits * f4, true}};
  return chunked_query(ctx, __func__, n, on_device, arrays, [&](void* const d[], uint32_t cnt, size_t) {
    const dim3 blk(hj::kBlockThreads);
    const float4* d_rays = static_cast<const float4*>(d[0]);
    uint2* d_counts = static_cast<uint2*>(d[1]);
    float4* d_hits = static_cast<float4*>(d[2]);                           // (max_hits == 0: null)
    if (max_hits) hipLaunchKernelGGL(hj::k_mh_walk<true>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, d_rays, cnt, max_hits, d_counts, d_hits);
    else hipLaunchKernelGGL(hj::k_mh_walk<false>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, d_rays, cnt, 0u, d_counts, d_hits);
    return hipGetLastError();
  });
}

// (its points and its count pairs borrow AllHits::rays and AllHits::counts)
int hj_points_inside(hj_context* ctx, const float* points, size_t n, uint32_t flags, uint32_t* out) {
  if (n != 0 && (!points || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: null %s", !points ? "points" : "out");
  if (flags & ~(uint32_t)(HJ_INSIDE_DEVICE_ARRAYS | HJ_INSIDE_PARITY)) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_INSIDE_DEVICE_ARRAYS) != 0, parity = (flags & HJ_INSIDE_PARITY) != 0;
  if (n != 0) {
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: %zu points, at most 2^31 - 1 a call", n);
    if (on_device && misaligned(points, out)) return set_error(ctx, HJ_ERR_INVALID, "hj_points_inside: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  hj_context::AllHits& q = ctx->allhits;
  const QueryArray arrays[] = {{points, &q.rays, sizeof(float4), false}, {out, &q.counts, sizeof(uint2), true}};
  return chunked_query(ctx, __func__, n, on_device, arrays, [&](void* const d[], uint32_t cnt, size_t) {
    const dim3 blk(hj::kBlockThreads);
    const float4* d_points = static_cast<const float4*>(d[0]);
    uint2* d_out = static_cast<uint2*>(d[1]);
    if (parity) hipLaunchKernelGGL(hj::k_mh_inside<true>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, d_points, cnt, d_out);
    else hipLaunchKernelGGL(hj::k_mh_inside<false>, per_lane(cnt), blk, 0, ctx->stream, ctx->scene, d_points, cnt, d_out);
    return hipGetLastError();
  });
}

}  // extern "C"
