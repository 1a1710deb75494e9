// hj_follow_specular, and the follow rounds of hj_render_aovs_followed / hj_render_aovs_frame_followed: what a mirror or glass shows
// ("Followed AOVs").
//
// The kernels are kernels/hj_follow.h's and, behind it, kernels/hj_chain.h's: the rounds' shared text, whose count and scan kernels
// this unit alone instantiates (api/motion_follow.hip launches them through chain_count_enqueue).  The two frame entry points
// themselves, their checks, the runs and the camera walk are api/aov.hip's (aov_render), which enters here behind each walk launch:
//   per round   (chain_rounds, api/chain_rounds.h) k_chain_count -> k_chain_scan -> (the live count to the host: it sizes the grid;
//               none: the rounds end, nothing is launched) -> k_af_scatter -> k_aov_follow over the list
//   resolve     k_aov_resolve_followed in k_aov_resolve's place for a launch that took a round
//   per record  k_follow, one lane per record; chunks and staging through hj_context::Aov are chunked_query's (api/hj_internal.h)
#include "hj_internal.h"
#include "../kernels/hj_follow.h"
#include "chain_rounds.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {

// The one copy of the count and scan kernels (kernels/hj_chain.h), for this unit's rounds and api/motion_follow.hip's: the live chains
// of n slots per tile of kChainThreads into d_counts, then their offsets in place and the total behind them.
void chain_count_enqueue(hj_context* ctx, bool first, const float4* d_hits, const float4* d_state, uint32_t n, uint32_t max_follow, uint32_t* d_counts) {
  const uint32_t tiles = (n + hj::kChainThreads - 1u) / hj::kChainThreads;
  const dim3 tile(hj::kChainThreads);
  if (first) hipLaunchKernelGGL(hj::k_chain_count<true>, dim3(tiles), tile, 0, ctx->stream, ctx->scene, d_hits, d_state, n, max_follow, d_counts);
  else hipLaunchKernelGGL(hj::k_chain_count<false>, dim3(tiles), tile, 0, ctx->stream, ctx->scene, d_hits, d_state, n, max_follow, d_counts);
  hipLaunchKernelGGL(hj::k_chain_scan, dim3(1), tile, 0, ctx->stream, d_counts, tiles);
}

// Room for the rounds over walk launches of at most `slots` sample slots.  Before anything of the call is enqueued.
int aov_follow_reserve(hj_context* ctx, size_t slots) { return chain_reserve(ctx, ctx->aov.chain, slots); }

// Behind the camera walk of nb blocks at d_blocks, whose hit records are at d_hits: chain_rounds over the launch's sample slots.
// -> followed: a round ran, so the chain state is set for every sample of the launch and its runs resolve through aov_follow_resolve.
hipError_t aov_follow_rounds(hj_context* ctx, const hj_image_block* d_blocks, uint32_t nb, float4* d_hits, uint32_t max_follow, bool& followed) {
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const uint32_t n = nb * hj::kSlotsPerBlock;
  return chain_rounds(
      ctx, ctx->aov.chain, d_hits, n, max_follow,
      [&](auto first, dim3 tiles, float4* d_state, const uint32_t* d_offsets, uint32_t* d_list) {
        hipLaunchKernelGGL(hj::k_af_scatter<decltype(first)::value>, tiles, dim3(hj::kChainThreads), 0, s, sc, d_blocks, nb, static_cast<const float4*>(d_hits),
                           d_state, n, max_follow, d_offsets, d_list);
      },
      [&](auto pairs, dim3 grid, const uint32_t* d_list, uint32_t count, uint32_t wg_rays, float4* d_state) {
        hipLaunchKernelGGL(hj::k_aov_follow<decltype(pairs)::value>, grid, dim3(hj::kBlockThreads), 0, s, sc, d_list, count, wg_rays, d_hits, d_state);
      },
      followed);
}

// k_aov_resolve's launch for a run of a followed walk launch
void aov_follow_resolve(hj_context* ctx, const hj_image_block* d_blocks, uint32_t nb, uint32_t b0, uint32_t cnt, const float4* d_hits, uint32_t width,
                        uint32_t height, float4* d_aov) {
  hipLaunchKernelGGL(hj::k_aov_resolve_followed, per_lane(cnt * hj::kSlotsPerBlock), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, d_blocks, nb, b0, cnt,
                     d_hits, static_cast<const float4*>(ctx->aov.chain.state.p), width, height, d_aov);
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
