// hj_render_motion_followed: hj_render_motion's record for what a mirror or glass shows ("Followed motion") - the motion
// image that composes with the followed AOVs' guides in hj_denoise_frame_temporal_motion.
//
// The kernels are kernels/hj_motion_follow.h's; that header includes kernels/hj_motion.h and kernels/hj_follow.h without their kernels
// (k_mv_walk, k_mv_resolve stay api/motion.hip's, the k_af_* and k_aov_follow api/follow.hip's) and hj_compact.h and edits none, and
// no other unit's machine code depends on this one.  The checks, the staging, the camera walk and the drain are api/motion.hip's
// (motion_render), which enters here behind k_mv_walk:
//   per round   k_mf_count -> k_mf_scan -> (the live count to the host: it sizes the grid; none: the rounds end, nothing is launched)
//               -> k_mf_scatter -> k_mf_follow over the list
//   resolve     k_mf_resolve in k_mv_resolve's place for an image that took a round
#include "hj_internal.h"
#include "../kernels/hj_motion_follow.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {

// Room for the rounds over an image of `pixels` pixels: the chain state (32 bytes a pixel), the product of the reflections (48 bytes),
// the tile counts and the list (4 bytes a pixel).  Before anything of the call is enqueued.
int motion_follow_reserve(hj_context* ctx, size_t pixels) {
  hj_context::Motion& q = ctx->motion;
  HJ_TRY(dev_alloc(ctx, q.state, pixels * 2 * sizeof(float4)));
  HJ_TRY(dev_alloc(ctx, q.mat, pixels * 3 * sizeof(float4)));
  HJ_TRY(dev_alloc(ctx, q.counts, ((pixels + hj::kMfThreads - 1u) / hj::kMfThreads + 1u) * sizeof(uint32_t)));
  return dev_alloc(ctx, q.list, pixels * sizeof(uint32_t));
}

// Behind k_mv_walk over a width x height image whose raw hits are at d_motion: at most max_follow (> 0) rounds, each over the chains
// still live.  The stream is synchronised once a round, for the live count.  -> followed: a round ran, so the chain state is set for
// every pixel and the image resolves through motion_follow_resolve.
hipError_t motion_follow_rounds(hj_context* ctx, uint32_t width, uint32_t height, float4* d_motion, uint32_t max_follow, bool& followed) {
  hj_context::Motion& q = ctx->motion;
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const uint32_t n = width * height, tiles = (n + hj::kMfThreads - 1u) / hj::kMfThreads;   // (n <= 2^28)
  float4 *d_state = static_cast<float4*>(q.state.p), *d_mat = static_cast<float4*>(q.mat.p);
  uint32_t *d_counts = static_cast<uint32_t*>(q.counts.p), *d_list = static_cast<uint32_t*>(q.list.p);
  const dim3 tile(hj::kMfThreads);
  followed = false;
  for (uint32_t round = 0; round < max_follow; round++) {
    const bool first = round == 0;
    if (first) hipLaunchKernelGGL(hj::k_mf_count<true>, dim3(tiles), tile, 0, s, sc, static_cast<const float4*>(d_motion), static_cast<const float4*>(d_state), n, max_follow, d_counts);
    else hipLaunchKernelGGL(hj::k_mf_count<false>, dim3(tiles), tile, 0, s, sc, static_cast<const float4*>(d_motion), static_cast<const float4*>(d_state), n, max_follow, d_counts);
    hipLaunchKernelGGL(hj::k_mf_scan, dim3(1), tile, 0, s, d_counts, tiles);
    hipError_t e = hipGetLastError();
    uint32_t count = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_counts + tiles, sizeof count, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    if (count == 0) break;                                         // (no grid of zero workgroups is ever launched)
    if (first) hipLaunchKernelGGL(hj::k_mf_scatter<true>, dim3(tiles), tile, 0, s, sc, width, height, static_cast<const float4*>(d_motion), d_state, d_mat, n, max_follow, static_cast<const uint32_t*>(d_counts), d_list);
    else hipLaunchKernelGGL(hj::k_mf_scatter<false>, dim3(tiles), tile, 0, s, sc, width, height, static_cast<const float4*>(d_motion), d_state, d_mat, n, max_follow, static_cast<const uint32_t*>(d_counts), d_list);
    const uint32_t wg_rays = walk_wg_rays(ctx, count);              // list entries per workgroup: hj_trace_rays' rule
    const dim3 grid((count + wg_rays - 1u) / wg_rays);
    if (sc.has_pairs != 0) hipLaunchKernelGGL(hj::k_mf_follow<true>, grid, dim3(hj::kBlockThreads), 0, s, sc, static_cast<const uint32_t*>(d_list), count, wg_rays, d_motion, d_state, d_mat);
    else hipLaunchKernelGGL(hj::k_mf_follow<false>, grid, dim3(hj::kBlockThreads), 0, s, sc, static_cast<const uint32_t*>(d_list), count, wg_rays, d_motion, d_state, d_mat);
    if (e = hipGetLastError(); e != hipSuccess) return e;
    followed = true;
  }
  return hipSuccess;
}

// k_mv_resolve's launch for an image that took a round: the uploaded arrays stand beside the previous ones
void motion_follow_resolve(hj_context* ctx, const hj::MvPrev& prev, uint32_t width, uint32_t height, float4* d_motion) {
  const hj::DeviceScene& sc = ctx->scene;
  const hj::MvPrev now{sc.spheres, sc.quads, reinterpret_cast<const float4*>(sc.vertices), prev.cam};
  hipLaunchKernelGGL(hj::k_mf_resolve, per_lane(width * height), dim3(hj::kBlockThreads), 0, ctx->stream, sc, now, prev, width, height,
                     static_cast<const float4*>(ctx->motion.state.p), static_cast<const float4*>(ctx->motion.mat.p), d_motion);
}

}  // namespace hjapi

extern "C" {

int hj_render_motion_followed(hj_context* ctx, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t max_follow, uint32_t flags, float* motion) {
  return motion_render(ctx, "hj_render_motion_followed", prev, width, height, max_follow, flags, motion);
}

}  // extern "C"
