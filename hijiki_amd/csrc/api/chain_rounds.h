// The host side of a specular chain's rounds, once, for the units whose kernels wrap kernels/hj_chain.h's bodies: api/follow.hip
// (the followed AOVs) and api/motion_follow.hip (the followed motion image).  The including unit has included hj_internal.h and its
// kernel header, and hands in the launches of its own scatter and round kernels; the count and the scan are launched by the unit
// that holds them (chain_count_enqueue, hj_internal.h).
#pragma once
#include <type_traits>

namespace hjapi {

// Room for the rounds over n slots: the chain state (32 bytes a slot), a count per tile and the total, the list (4 bytes a slot).
// Before anything of the call is enqueued.
inline int chain_reserve(hj_context* ctx, ChainBufs& b, size_t n) {
  HJ_TRY(dev_alloc(ctx, b.state, n * 2 * sizeof(float4)));
  HJ_TRY(dev_alloc(ctx, b.counts, ((n + hj::kChainThreads - 1u) / hj::kChainThreads + 1u) * sizeof(uint32_t)));
  return dev_alloc(ctx, b.list, n * sizeof(uint32_t));
}

// Behind the first walk over n slots, whose hit records are at d_hits: at most max_follow (> 0) rounds, each over the chains still
// live.  Per round: count -> scan -> (the live count to the host: it sizes the grid, and the stream is synchronised once a round for
// it; none: the rounds end, nothing is launched) -> scatter -> the round over the list.
//   launch_scatter(FIRST, tiles, d_state, d_offsets, d_list)          the unit's scatter kernel, one workgroup of kChainThreads a tile
//   launch_round(PAIRS, grid, d_list, count, wg_rays, d_state)        the unit's round kernel, kBlockThreads a workgroup
// FIRST, PAIRS: a std::true_type or std::false_type, the kernel's template argument as its ::value - the dispatch is here, once.
// -> followed: a round ran, so the chain state is set for every slot that has a ray.
template <class LaunchScatter, class LaunchRound>
hipError_t chain_rounds(hj_context* ctx, ChainBufs& b, float4* d_hits, uint32_t n, uint32_t max_follow, LaunchScatter launch_scatter,
                        LaunchRound launch_round, bool& followed) {
  hipStream_t s = ctx->stream;
  const uint32_t tiles = (n + hj::kChainThreads - 1u) / hj::kChainThreads;
  float4* d_state = static_cast<float4*>(b.state.p);
  uint32_t *d_counts = static_cast<uint32_t*>(b.counts.p), *d_list = static_cast<uint32_t*>(b.list.p);
  followed = false;
  for (uint32_t round = 0; round < max_follow; round++) {
    const bool first = round == 0;
    chain_count_enqueue(ctx, first, d_hits, d_state, n, max_follow, d_counts);
    hipError_t e = hipGetLastError();
    uint32_t count = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_counts + tiles, sizeof count, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    if (count == 0) break;                                         // (no grid of zero workgroups is ever launched)
    const uint32_t* d_offsets = d_counts;
    if (first) launch_scatter(std::true_type{}, dim3(tiles), d_state, d_offsets, d_list);
    else launch_scatter(std::false_type{}, dim3(tiles), d_state, d_offsets, d_list);
    const uint32_t wg_rays = walk_wg_rays(ctx, count);              // list entries per workgroup: hj_trace_rays' rule
    const dim3 grid((count + wg_rays - 1u) / wg_rays);
    const uint32_t* d_live = d_list;
    if (ctx->scene.has_pairs != 0) launch_round(std::true_type{}, grid, d_live, count, wg_rays, d_state);
    else launch_round(std::false_type{}, grid, d_live, count, wg_rays, d_state);
    if (e = hipGetLastError(); e != hipSuccess) return e;
    followed = true;
  }
  return hipSuccess;
}

}  // namespace hjapi
