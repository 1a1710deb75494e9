// hj_render_direct_lit, hj_render_direct_lit_frame: hj_render_probe_lit's frame with one traced next-event sample at each chain's last
// diffuse hit - sharp direct shadows beside the volume's indirect light ("Direct-lit frames").
//
// The kernels are kernels/hj_direct_lit.h's; that header includes kernels/hj_probe_lit.h without its kernels and edits none.  The checks
// of the blocks and the image, the runs, the camera walk and the follow rounds are api/aov.hip's (aov_check, aov_render), entered with
// an AovStage; the volume, its refusals, its staging and the points hook are api/probe_lit.hip's (probe_lit_volume.h):
//   per walk launch  (k_aov_walk, the follow rounds) -> k_pl_points and the volume's look-up (lit_points; no lighting: k_pl_points alone)
//                    -> k_dl_sample -> k_dl_count -> k_dl_scan -> (the count of wanted rays to the host: it sizes the grid; none:
//                    nothing more is launched) -> k_dl_scatter -> k_dl_shadow over the list
//   per run part     k_dl_resolve in k_pl_resolve's place
// The list and its tile counts are the chain rounds' buffers (hj_context::Aov::chain): the rounds of a launch are over before its
// shadow rays are listed.
#include "hj_internal.h"
#include "../kernels/hj_direct_lit.h"
#include "probe_lit_volume.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

// What a call's stage carries: the probe-lit stage's volume, or none
struct Direct {
  bool has_volume;
  Lit lit;
};

AovStage lit_stage_of(const AovStage& st) {
  Direct& dl = *static_cast<Direct*>(st.self);
  return AovStage{st.words, nullptr, nullptr, nullptr, dl.has_volume ? &dl.lit : nullptr};
}

int dl_reserve(hj_context* ctx, const AovStage& st, size_t slots) {
  HJ_TRY(lit_reserve(ctx, lit_stage_of(st), slots));
  HJ_TRY(dev_alloc(ctx, ctx->direct_lit.rays, slots * 3 * sizeof(float4)));
  ChainBufs& b = ctx->aov.chain;
  HJ_TRY(dev_alloc(ctx, b.counts, ((slots + hj::kDlThreads - 1u) / hj::kDlThreads + 1u) * sizeof(uint32_t)));
  return dev_alloc(ctx, b.list, slots * sizeof(uint32_t));
}

// Behind the walk and the rounds of a launch of nb blocks: the probe-lit stage's points and look-up, then the next-event sample of
// every slot, the list of the slots that want a shadow ray, and the any-hit walk over it
hipError_t dl_points(hj_context* ctx, const AovStage& st, const hj_image_block* d_blocks, uint32_t nb, const float4* d_hits, bool followed) {
  if (const hipError_t e = lit_points(ctx, lit_stage_of(st), d_blocks, nb, d_hits, followed); e != hipSuccess) return e;
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const uint32_t n = nb * hj::kSlotsPerBlock, tiles = n / hj::kDlThreads;
  const float4* d_state = followed ? static_cast<const float4*>(ctx->aov.chain.state.p) : nullptr;
  float4* d_rays = static_cast<float4*>(ctx->direct_lit.rays.p);
  uint32_t *d_counts = static_cast<uint32_t*>(ctx->aov.chain.counts.p), *d_list = static_cast<uint32_t*>(ctx->aov.chain.list.p);
  const dim3 blk(hj::kBlockThreads), tile(hj::kDlThreads);
  if (sc.env_alias != nullptr) hipLaunchKernelGGL(hj::k_dl_sample<true>, per_lane(n), blk, 0, s, sc, d_blocks, nb, d_hits, d_state, d_rays);
  else hipLaunchKernelGGL(hj::k_dl_sample<false>, per_lane(n), blk, 0, s, sc, d_blocks, nb, d_hits, d_state, d_rays);
  hipLaunchKernelGGL(hj::k_dl_count, dim3(tiles), tile, 0, s, static_cast<const float4*>(d_rays), n, d_counts);
  hipLaunchKernelGGL(hj::k_dl_scan, dim3(1), tile, 0, s, d_counts, tiles);
  hipError_t e = hipGetLastError();
  uint32_t count = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&count, d_counts + tiles, sizeof count, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess || count == 0) return e;                     // (no grid of zero workgroups is ever launched)
  hipLaunchKernelGGL(hj::k_dl_scatter, dim3(tiles), tile, 0, s, static_cast<const float4*>(d_rays), n, static_cast<const uint32_t*>(d_counts), d_list);
  const uint32_t wg_rays = walk_wg_rays(ctx, count);                // list entries per workgroup: hj_trace_rays' rule
  const dim3 grid((count + wg_rays - 1u) / wg_rays);
  if (sc.has_pairs != 0) hipLaunchKernelGGL(hj::k_dl_shadow<true>, grid, blk, 0, s, sc, static_cast<const uint32_t*>(d_list), count, wg_rays, d_rays);
  else hipLaunchKernelGGL(hj::k_dl_shadow<false>, grid, blk, 0, s, sc, static_cast<const uint32_t*>(d_list), count, wg_rays, d_rays);
  return hipGetLastError();
}

void dl_resolve(hj_context* ctx, const AovStage& st, const hj_image_block* d_blocks, uint32_t nb, uint32_t b0, uint32_t cnt, const float4* d_hits,
                bool followed, uint32_t width, uint32_t height, float4* d_image) {
  const Direct& dl = *static_cast<const Direct*>(st.self);
  hj_context::ProbeLit& q = ctx->probe_lit;
  const float4* d_state = followed ? static_cast<const float4*>(ctx->aov.chain.state.p) : nullptr;
  const float4* d_lookup = dl.has_volume ? static_cast<const float4*>(q.lookup.p) : nullptr;
  hipLaunchKernelGGL(hj::k_dl_resolve, per_lane(cnt * hj::kSlotsPerBlock), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, d_blocks, nb, b0, cnt, d_hits,
                     d_state, d_lookup, static_cast<const float4*>(q.side.p), static_cast<const float4*>(ctx->direct_lit.rays.p), width, height, d_image);
}

// hj_render_probe_lit's refusals of the lighting, a null one accepted: nothing of a volume is then checked
int dl_check(hj_context* ctx, const char* fn, const hj_probe_lighting* lighting, bool any, Direct& dl, uint32_t& np, bool& reads_atlas) {
  dl.has_volume = lighting != nullptr;
  dl.lit = Lit{};
  return dl.has_volume ? lit_check(ctx, fn, lighting, any, dl.lit, np, reads_atlas) : HJ_OK;
}

int dl_render(hj_context* ctx, const char* fn, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t max_follow,
              uint32_t flags, const hj_probe_lighting* lighting, uint32_t np, bool reads_atlas, Direct& dl, float* image) {
  if (num_blocks != 0 && dl.has_volume) HJ_TRY(lit_stage(ctx, fn, lighting, np, reads_atlas, dl.lit));
  const AovStage stage{HJ_PROBE_LIT_WORDS, dl_reserve, dl_points, dl_resolve, &dl};
  return aov_render(ctx, fn, blocks, num_blocks, width, height, flags, image, max_follow, &stage);
}

}  // namespace

extern "C" {

// The argument checks come first and need neither a device nor a context's state: hj_render_probe_lit's, in its order; then the gate.
int hj_render_direct_lit(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t max_follow,
                         uint32_t flags, const hj_probe_lighting* lighting, float* image) {
  HJ_TRY(aov_check(ctx, __func__, blocks, num_blocks, width, height, flags, image));
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", __func__, max_follow, (unsigned)HJ_AOV_MAX_FOLLOW);
  Direct dl;
  uint32_t np = 0;
  bool reads_atlas = false;
  HJ_TRY(dl_check(ctx, __func__, lighting, num_blocks != 0, dl, np, reads_atlas));
  HJ_TRY(query_gate(ctx, __func__));
  return dl_render(ctx, __func__, blocks, num_blocks, width, height, max_follow, flags, lighting, np, reads_atlas, dl, image);
}

int hj_render_direct_lit_frame(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin, uint32_t pass_end,
                               uint32_t max_follow, uint32_t flags, const hj_probe_lighting* lighting, float* image) {
  HJ_TRY(aov_check(ctx, __func__, nullptr, 0, width, height, flags, image));
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", __func__, max_follow, (unsigned)HJ_AOV_MAX_FOLLOW);
  if (pass_begin > pass_end || pass_end > spp) return set_error(ctx, HJ_ERR_INVALID, "%s: bad pass range [%u,%u) of %u", __func__, pass_begin, pass_end, spp);
  Direct dl;
  uint32_t np = 0;
  bool reads_atlas = false;
  HJ_TRY(dl_check(ctx, __func__, lighting, pass_begin != pass_end, dl, np, reads_atlas));
  HJ_TRY(query_gate(ctx, __func__));
  std::vector<hj_image_block> blocks;
  HJ_TRY(aov_frame_blocks(ctx, __func__, width, height, master_seed, pass_begin, pass_end, blocks));
  return dl_render(ctx, __func__, blocks.data(), blocks.size(), width, height, max_follow, flags, lighting, np, reads_atlas, dl, image);
}

}  // extern "C"
