// hj_closest_points, hj_distance_field: the nearest surface point of the uploaded scene to caller-given points - the public distance
// query ("Distance queries").
//
// The kernels are kernels/hj_closest.h's (beside it hj_intersect.h for the scene's records and hj_num.h; of hj_probes.h the grid
// struct alone): this unit includes the existing kernel headers and edits none, and no other unit's machine code depends on it.
//   query:   k_cq_walk<STATS, ORDERED>, one lane per point, over the second copy of the uploaded tree (HJ_CLOSEST_ORDERED picks the form)
//   field:   k_pv_points (api/probe_volume.hip, through probe_points_enqueue)  ->  k_cq_pack  ->  k_cq_walk  ->  k_cq_resolve
// The query's chunks and the staging of host arrays through hj_context::ClosestQuery are chunked_query's (api/hj_internal.h).
#include "hj_internal.h"
#define HJ_PROBES_NO_SAMPLE_KERNEL
#include "../kernels/hj_probes.h"
#include "../kernels/hj_closest.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

// one launch: points [0, n) at d_points -> d_out, all on the device; d_partial (null: no statistics): two uint64 per workgroup
void launch_closest(hj_context* ctx, const float4* d_points, uint32_t n, float4* d_out, unsigned long long* d_partial) {
  const dim3 grid = per_lane(n), blk(hj::kBlockThreads);
  const bool ordered = ctx->tuning.closest_ordered != 0;                  // HJ_CLOSEST_ORDERED: the A/B partner is the stackless walk alone
  if (d_partial && ordered) hipLaunchKernelGGL((hj::k_cq_walk<true, true>), grid, blk, 0, ctx->stream, ctx->scene, d_points, n, d_out, d_partial);
  else if (d_partial) hipLaunchKernelGGL((hj::k_cq_walk<true, false>), grid, blk, 0, ctx->stream, ctx->scene, d_points, n, d_out, d_partial);
  else if (ordered) hipLaunchKernelGGL((hj::k_cq_walk<false, true>), grid, blk, 0, ctx->stream, ctx->scene, d_points, n, d_out, d_partial);
  else hipLaunchKernelGGL((hj::k_cq_walk<false, false>), grid, blk, 0, ctx->stream, ctx->scene, d_points, n, d_out, d_partial);
}

}  // namespace

extern "C" {

// The argument checks come first, in hj_trace_rays' order and style, and need neither a device nor a context's state; then the
// queries' gate.  What `stats` points at is asked of the runtime's pointer table, which launches nothing; a process without a
// device has no device pointers.
int hj_closest_points(hj_context* ctx, const float* points, size_t n, uint32_t flags, float* out, uint64_t* stats) {
  if (n != 0 && (!points || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_closest_points: null %s", !points ? "points" : "out");
  if (flags & ~(uint32_t)HJ_CLOSEST_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_closest_points: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_CLOSEST_DEVICE_ARRAYS) != 0;
  if (n != 0) {
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_closest_points: %zu points, at most 2^31 - 1 a call", n);
    if (on_device && misaligned(points, out))
      return set_error(ctx, HJ_ERR_INVALID, "hj_closest_points: device arrays must be 16-byte aligned");
    if (on_device && stats) {
      hipPointerAttribute_t at{};
      const hipError_t pe = hipPointerGetAttributes(&at, stats);
      if (pe != hipSuccess) (void)hipGetLastError();                       // (an ordinary host pointer the runtime does not know)
      else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged)
        return set_error(ctx, HJ_ERR_INVALID, "hj_closest_points: stats is a host pointer, with device arrays too");
    }
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  hj_context::ClosestQuery& q = ctx->closest;
  // statistics: per launch two uint64 per workgroup, read back behind the launch and summed once the stream has drained
  const size_t chunk = (size_t)ctx->tuning.trace_chunk, G = per_lane((uint32_t)std::min(n, chunk)).x, launches = (n + chunk - 1) / chunk;
  std::vector<unsigned long long> h_partial;
  unsigned long long* d_partial = nullptr;
  if (stats) {
    HJ_HIP(ctx, hipSetDevice(ctx->device));                                // (this allocation comes before chunked_query's own)
    HJ_TRY(dev_alloc(ctx, q.partial, 2 * G * sizeof(unsigned long long)));
    d_partial = static_cast<unsigned long long*>(q.partial.p);
    try {
      h_partial.assign(launches * 2 * G, 0ull);
    } catch (const std::bad_alloc&) {
      return set_error(ctx, HJ_ERR_NOMEM, "hj_closest_points: out of host memory");
    }
  }
  const QueryArray arrays[] = {{points, &q.points, sizeof(float4), false}, {out, &q.out, 2 * sizeof(float4), true}};
  const int rc = chunked_query(ctx, __func__, n, on_device, arrays, [&](void* const d[], uint32_t cnt, size_t launch) {
    launch_closest(ctx, static_cast<const float4*>(d[0]), cnt, static_cast<float4*>(d[1]), d_partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !stats) return e;
    return hipMemcpyAsync(h_partial.data() + launch * 2 * G, d_partial, 2 * (size_t)per_lane(cnt).x * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          ctx->stream);
  });
  if (rc == HJ_OK && stats) {
    stats[0] = 0; stats[1] = 0;
    for (size_t k = 0; k < h_partial.size(); k += 2) { stats[0] += h_partial[k]; stats[1] += h_partial[k + 1]; }
  }
  return rc;
}

// The grid of desc (hj_probe_points' positions) through the query without leaving the device: per chunk the gather points, the
// query points with max_distance as the radius, the records, one float per point.
int hj_distance_field(hj_context* ctx, const hj_probe_desc* desc, float max_distance, uint32_t flags, float* field) {
  if (!desc || !field) return set_error(ctx, HJ_ERR_INVALID, "hj_distance_field: null %s", !desc ? "desc" : "field");
  hj::PvGrid g{};
  uint32_t n = 0;
  HJ_TRY(probe_desc_check(ctx, __func__, desc, g, n));
  if (flags & ~(uint32_t)HJ_DISTANCE_UNSIGNED) return set_error(ctx, HJ_ERR_INVALID, "hj_distance_field: unknown distance flag bits 0x%x", flags);
  if (!(max_distance >= 0.0f)) return set_error(ctx, HJ_ERR_INVALID, "hj_distance_field: max_distance %g: >= 0 is needed (+inf: no limit)", (double)max_distance);
  const bool on_device = (desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(field)) return set_error(ctx, HJ_ERR_INVALID, "hj_distance_field: device arrays must be 16-byte aligned");
  HJ_TRY(query_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t chunk = (uint32_t)std::min<size_t>((size_t)ctx->tuning.trace_chunk, n);
  const size_t f4 = sizeof(float4);
  hj_context::ClosestQuery& q = ctx->closest;
  HJ_TRY(dev_alloc(ctx, q.grid, (size_t)chunk * 2 * f4));
  HJ_TRY(dev_alloc(ctx, q.points, (size_t)chunk * f4));
  HJ_TRY(dev_alloc(ctx, q.out, (size_t)chunk * 2 * f4));
  if (!on_device) HJ_TRY(dev_alloc(ctx, q.field, (size_t)chunk * sizeof(float)));
  float4 *d_grid = static_cast<float4*>(q.grid.p), *d_points = static_cast<float4*>(q.points.p), *d_out = static_cast<float4*>(q.out.p);
  const dim3 blk(hj::kBlockThreads);
  hipError_t e = hipSuccess;
  for (uint32_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t cnt = std::min(chunk, n - at);
    float* d_field = on_device ? field + at : static_cast<float*>(q.field.p);
    probe_points_enqueue(ctx, g, desc->seed, desc->seed_stride, at, cnt, d_grid);
    hipLaunchKernelGGL(hj::k_cq_pack, per_lane(cnt), blk, 0, ctx->stream, static_cast<const float4*>(d_grid), cnt, max_distance, d_points);
    launch_closest(ctx, d_points, cnt, d_out, nullptr);
    hipLaunchKernelGGL(hj::k_cq_resolve, per_lane(cnt), blk, 0, ctx->stream, static_cast<const float4*>(d_out), cnt, max_distance,
                       (flags & HJ_DISTANCE_UNSIGNED) ? 0u : 1u, d_field);
    e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(field + at, d_field, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  }
  return drain(ctx, __func__, e);
}

}  // extern "C"
