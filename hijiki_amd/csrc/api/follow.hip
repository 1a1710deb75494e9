// hj_follow_specular, and the follow rounds of hj_render_aovs_followed / hj_render_aovs_frame_followed: what a mirror or glass shows
// ("Followed AOVs").
//
// The kernels are kernels/hj_follow.h's; that header includes kernels/hj_aov.h - and through it the kernel headers up to hj_stages.h -
// and hj_compact.h and edits none, and no other unit's machine code depends on this one.  The two frame entry points themselves, their
// checks, the runs and the camera walk are api/aov.hip's (aov_render), which enters here behind each walk launch:
//   per round   k_af_count -> k_af_scan -> (the live count to the host: it sizes the grid; none: the rounds end, nothing is launched)
//               -> k_af_scatter -> k_aov_follow over the list
//   resolve     k_aov_resolve_followed in k_aov_resolve's place for a launch that took a round
//   per record  k_follow, one lane per record; chunks and staging through hj_context::Aov are chunked_query's (api/hj_internal.h)
#include "hj_internal.h"
#include "../kernels/hj_follow.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {

// Room for the rounds over walk launches of at most `slots` sample slots: the chain state (32 bytes a slot), the tile counts and
// the list (4 bytes a slot).  Before anything of the call is enqueued.
int aov_follow_reserve(hj_context* ctx, size_t slots) {
  hj_context::Aov& q = ctx->aov;
  HJ_TRY(dev_alloc(ctx, q.state, slots * 2 * sizeof(float4)));
  HJ_TRY(dev_alloc(ctx, q.counts, (slots / hj::kAfThreads + 1u) * sizeof(uint32_t)));
  return dev_alloc(ctx, q.list, slots * sizeof(uint32_t));
}

// Behind the camera walk of nb blocks at d_blocks, whose hit records are at d_hits: at most max_follow (> 0) rounds, each over the
// chains still live.  The stream is synchronised once a round, for the live count.  -> followed: a round ran, so the chain state is
// set for every sample of the launch and its runs resolve through aov_follow_resolve.
hipError_t aov_follow_rounds(hj_context* ctx, const hj_image_block* d_blocks, uint32_t nb, float4* d_hits, uint32_t max_follow, bool& followed) {
  hj_context::Aov& q = ctx->aov;
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const uint32_t n = nb * hj::kSlotsPerBlock, tiles = n / hj::kAfThreads;
  float4* d_state = static_cast<float4*>(q.state.p);
  uint32_t *d_counts = static_cast<uint32_t*>(q.counts.p), *d_list = static_cast<uint32_t*>(q.list.p);
  const dim3 tile(hj::kAfThreads);
  followed = false;
  for (uint32_t round = 0; round < max_follow; round++) {
    const bool first = round == 0;
    if (first) hipLaunchKernelGGL(hj::k_af_count<true>, dim3(tiles), tile, 0, s, sc, static_cast<const float4*>(d_hits), static_cast<const float4*>(d_state), n, max_follow, d_counts);
    else hipLaunchKernelGGL(hj::k_af_count<false>, dim3(tiles), tile, 0, s, sc, static_cast<const float4*>(d_hits), static_cast<const float4*>(d_state), n, max_follow, d_counts);
    hipLaunchKernelGGL(hj::k_af_scan, dim3(1), tile, 0, s, d_counts, tiles);
    hipError_t e = hipGetLastError();
    uint32_t count = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_counts + tiles, sizeof count, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    if (count == 0) break;                                         // (no grid of zero workgroups is ever launched)
    if (first) hipLaunchKernelGGL(hj::k_af_scatter<true>, dim3(tiles), tile, 0, s, sc, d_blocks, nb, static_cast<const float4*>(d_hits), d_state, n, max_follow, static_cast<const uint32_t*>(d_counts), d_list);
    else hipLaunchKernelGGL(hj::k_af_scatter<false>, dim3(tiles), tile, 0, s, sc, d_blocks, nb, static_cast<const float4*>(d_hits), d_state, n, max_follow, static_cast<const uint32_t*>(d_counts), d_list);
    const uint32_t wg_rays = walk_wg_rays(ctx, count);              // list entries per workgroup: hj_trace_rays' rule
    const dim3 grid((count + wg_rays - 1u) / wg_rays);
    if (sc.has_pairs != 0) hipLaunchKernelGGL(hj::k_aov_follow<true>, grid, dim3(hj::kBlockThreads), 0, s, sc, static_cast<const uint32_t*>(d_list), count, wg_rays, d_hits, d_state);
    else hipLaunchKernelGGL(hj::k_aov_follow<false>, grid, dim3(hj::kBlockThreads), 0, s, sc, static_cast<const uint32_t*>(d_list), count, wg_rays, d_hits, d_state);
    if (e = hipGetLastError(); e != hipSuccess) return e;
    followed = true;
  }
  return hipSuccess;
}

// k_aov_resolve's launch for a run of a followed walk launch
void aov_follow_resolve(hj_context* ctx, const hj_image_block* d_blocks, uint32_t nb, uint32_t b0, uint32_t cnt, const float4* d_hits, uint32_t width,
                        uint32_t height, float4* d_aov) {
  hipLaunchKernelGGL(hj::k_aov_resolve_followed, per_lane(cnt * hj::kSlotsPerBlock), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, d_blocks, nb, b0, cnt,
                     d_hits, static_cast<const float4*>(ctx->aov.state.p), width, height, d_aov);
}

}  // namespace hjapi

extern "C" {

// The argument checks come first, in hj_eval_materials' order, and need neither a device nor a context's state; then the queries' gate.
int hj_follow_specular(hj_context* ctx, const float* rays, const float* hits, size_t n, uint32_t flags, float* out_rays) {
  if (n != 0 && (!rays || !hits || !out_rays))
    return set_error(ctx, HJ_ERR_INVALID, "hj_follow_specular: null %s", !rays ? "rays" : !hits ? "hits" : "out_rays");
  if (flags & ~(uint32_t)HJ_FOLLOW_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_follow_specular: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_FOLLOW_DEVICE_ARRAYS) != 0;
  if (n != 0) {
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_follow_specular: %zu records, at most 2^31 - 1 a call", n);
    if (on_device && misaligned(rays, hits, out_rays))
      return set_error(ctx, HJ_ERR_INVALID, "hj_follow_specular: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  hj_context::Aov& q = ctx->aov;
  const size_t f4 = sizeof(float4);
  const QueryArray arrays[] = {{rays, &q.in_rays, 2 * f4, false}, {hits, &q.in_hits, f4, false}, {out_rays, &q.out_rays, 2 * f4, true}};
  return chunked_query(ctx, __func__, n, on_device, arrays, [&](void* const d[], uint32_t cnt, size_t) {
    hipLaunchKernelGGL(hj::k_follow, per_lane(cnt), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, static_cast<const float4*>(d[0]),
                       static_cast<const float4*>(d[1]), cnt, static_cast<float4*>(d[2]));
    return hipGetLastError();
  });
}

}  // extern "C"
