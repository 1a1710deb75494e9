// hj_render_motion_followed: hj_render_motion's record for what a mirror or glass shows ("Followed motion") - the motion
// image that composes with the followed AOVs' guides in hj_denoise_frame_temporal_motion.
//
// The kernels are kernels/hj_motion_follow.h's; that header includes kernels/hj_motion.h and kernels/hj_chain.h without their kernels
// (k_mv_walk, k_mv_resolve stay api/motion.hip's; k_chain_count, k_chain_scan, k_af_scatter and k_aov_follow api/follow.hip's) and
// edits none.  The checks, the staging, the camera walk and the drain are api/motion.hip's (motion_render), which enters here behind
// k_mv_walk:
//   per round   (chain_rounds, api/chain_rounds.h) k_chain_count -> k_chain_scan, launched by api/follow.hip's chain_count_enqueue ->
//               (the live count to the host: it sizes the grid; none: the rounds end, nothing is launched) -> k_mf_scatter ->
//               k_mf_follow over the list
//   resolve     k_mf_resolve in k_mv_resolve's place for an image that took a round
#include "hj_internal.h"
#include "../kernels/hj_motion_follow.h"
#include "chain_rounds.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {

// Room for the rounds over an image of `pixels` pixels: the chain's buffers and the product of the reflections (48 bytes a pixel).
// Before anything of the call is enqueued.
int motion_follow_reserve(hj_context* ctx, size_t pixels) {
  HJ_TRY(chain_reserve(ctx, ctx->motion.chain, pixels));
  return dev_alloc(ctx, ctx->motion.mat, pixels * 3 * sizeof(float4));
}

// Behind k_mv_walk over a width x height image whose raw hits are at d_motion: chain_rounds over the image's pixels.  -> followed: a
// round ran, so the chain state is set for every pixel and the image resolves through motion_follow_resolve.
hipError_t motion_follow_rounds(hj_context* ctx, uint32_t width, uint32_t height, float4* d_motion, uint32_t max_follow, bool& followed) {
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const uint32_t n = width * height;                                // (<= 2^28)
  float4* d_mat = static_cast<float4*>(ctx->motion.mat.p);
  return chain_rounds(
      ctx, ctx->motion.chain, d_motion, n, max_follow,
      [&](auto first, dim3 tiles, float4* d_state, const uint32_t* d_offsets, uint32_t* d_list) {
        hipLaunchKernelGGL(hj::k_mf_scatter<decltype(first)::value>, tiles, dim3(hj::kChainThreads), 0, s, sc, width, height, static_cast<const float4*>(d_motion),
                           d_state, d_mat, n, max_follow, d_offsets, d_list);
      },
      [&](auto pairs, dim3 grid, const uint32_t* d_list, uint32_t count, uint32_t wg_rays, float4* d_state) {
        hipLaunchKernelGGL(hj::k_mf_follow<decltype(pairs)::value>, grid, dim3(hj::kBlockThreads), 0, s, sc, d_list, count, wg_rays, d_motion, d_state, d_mat);
      },
      followed);
}

// k_mv_resolve's launch for an image that took a round: the uploaded arrays stand beside the previous ones
void motion_follow_resolve(hj_context* ctx, const hj::MvPrev& prev, uint32_t width, uint32_t height, float4* d_motion) {
  const hj::DeviceScene& sc = ctx->scene;
  const hj::MvPrev now{sc.spheres, sc.quads, reinterpret_cast<const float4*>(sc.vertices), prev.cam};
  hipLaunchKernelGGL(hj::k_mf_resolve, per_lane(width * height), dim3(hj::kBlockThreads), 0, ctx->stream, sc, now, prev, width, height,
                     static_cast<const float4*>(ctx->motion.chain.state.p), static_cast<const float4*>(ctx->motion.mat.p), d_motion);
}

}  // namespace hjapi

extern "C" {

int hj_render_motion_followed(hj_context* ctx, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t max_follow, uint32_t flags, float* motion) {
  return motion_render(ctx, "hj_render_motion_followed", prev, width, height, max_follow, flags, motion);
}

}  // extern "C"
