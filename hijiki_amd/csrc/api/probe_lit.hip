// hj_render_probe_lit, hj_render_probe_lit_frame: the frame a probe volume is for - hj_render_aovs_followed's samples, each lit at its
// chain's last diffuse hit by the volume's look-up ("Probe-lit frames").
//
// The kernels are kernels/hj_probe_lit.h's; that header includes kernels/hj_follow.h without its kernels - and through it the kernel
// headers up to hj_stages.h - and edits none, and no other unit's machine code depends on this one.  The checks of the blocks and the
// image, the runs, the camera walk and the follow rounds are api/aov.hip's (aov_check, aov_render), entered with an AovStage:
//   per walk launch  (k_aov_walk, the follow rounds) -> k_pl_points -> the volume's look-up kernel over the launch's points, launched by
//                    the unit that holds it: k_pv_sample (api/probe_volume.hip), k_pvv_sample (api/probe_visibility.hip) or
//                    k_pp_sample (api/probe_place.hip)
//   per run part     k_pl_resolve in k_aov_resolve's / k_aov_resolve_followed's place
// A host-side volume, atlas and placement are staged once a call, before aov_render enqueues anything.
// For api/direct_lit.hip (probe_lit_volume.h): the stage's volume (Lit), its checks and staging, its reserve and its points hook -
// with no volume (a null Lit) k_pl_points alone.
#include "hj_internal.h"
#include "../kernels/hj_probe_lit.h"
#include "probe_lit_volume.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {

int lit_reserve(hj_context* ctx, const AovStage&, size_t slots) {
  hj_context::ProbeLit& q = ctx->probe_lit;
  HJ_TRY(dev_alloc(ctx, q.points, slots * 2 * sizeof(float4)));
  HJ_TRY(dev_alloc(ctx, q.lookup, slots * sizeof(float4)));
  return dev_alloc(ctx, q.side, slots * sizeof(float4));
}

// Behind the walk and the rounds of a launch of nb blocks: the points of its n sample slots, then the look-up over all n of them
// (st.self == nullptr - hj_render_direct_lit without a lighting -: the points and side records alone)
hipError_t lit_points(hj_context* ctx, const AovStage& st, const hj_image_block* d_blocks, uint32_t nb, const float4* d_hits, bool followed) {
  hj_context::ProbeLit& q = ctx->probe_lit;
  const uint32_t n = nb * hj::kSlotsPerBlock;
  float4 *d_points = static_cast<float4*>(q.points.p), *d_lookup = static_cast<float4*>(q.lookup.p);
  const float4* d_state = followed ? static_cast<const float4*>(ctx->aov.chain.state.p) : nullptr;
  hipLaunchKernelGGL(hj::k_pl_points, per_lane(n), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, d_blocks, nb, d_hits, d_state, d_points,
                     static_cast<float4*>(q.side.p));
  if (const hipError_t e = hipGetLastError(); e != hipSuccess || !st.self) return e;
  const Lit& lit = *static_cast<const Lit*>(st.self);
  if (lit.lookup == LitLookup::kPlain) probe_sample_enqueue(ctx, lit.g, lit.d_probes, d_points, n, d_lookup);
  else probe_vis_sample_enqueue(ctx, lit.g, lit.v, lit.d_probes, lit.d_atlas, lit.d_place, d_points, n, d_lookup,
                                lit.lookup == LitLookup::kPlaced ? probe_place_sample_launch : nullptr);
  return hipGetLastError();
}

}  // namespace hjapi

namespace {

void lit_resolve(hj_context* ctx, const AovStage&, const hj_image_block* d_blocks, uint32_t nb, uint32_t b0, uint32_t cnt, const float4* d_hits,
                 bool followed, uint32_t width, uint32_t height, float4* d_image) {
  hj_context::ProbeLit& q = ctx->probe_lit;
  const float4* d_state = followed ? static_cast<const float4*>(ctx->aov.chain.state.p) : nullptr;
  hipLaunchKernelGGL(hj::k_pl_resolve, per_lane(cnt * hj::kSlotsPerBlock), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, d_blocks, nb, b0, cnt, d_hits,
                     d_state, static_cast<const float4*>(q.lookup.p), static_cast<const float4*>(q.side.p), width, height, d_image);
}

}  // namespace

namespace hjapi {

// The volume's refusals, without a device: a null lighting, a placement without vis, then those of the look-up `lighting` selects in that
// call's order (the points and the results are this call's own).  any: the call has blocks -> lit's look-up, grid and map; np
int lit_check(hj_context* ctx, const char* fn, const hj_probe_lighting* l, bool any, Lit& lit, uint32_t& np, bool& reads_atlas) {
  if (!l) return set_error(ctx, HJ_ERR_INVALID, "%s: null lighting", fn);
  if (l->placement && !l->vis) return set_error(ctx, HJ_ERR_INVALID, "%s: a placement needs vis", fn);
  lit = Lit{};
  reads_atlas = false;
  if (!l->vis) {                                                    // hj_sample_probes
    lit.lookup = LitLookup::kPlain;
    if (!l->desc || (any && !l->probes)) return set_error(ctx, HJ_ERR_INVALID, "%s: null %s", fn, !l->desc ? "desc" : "probes");
    HJ_TRY(probe_desc_check(ctx, fn, l->desc, lit.g, np));
    if ((l->desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0 && any && misaligned(l->probes))
      return set_error(ctx, HJ_ERR_INVALID, "%s: device arrays must be 16-byte aligned", fn);
    return HJ_OK;
  }
  lit.lookup = l->placement ? LitLookup::kPlaced : LitLookup::kVisible;  // hj_sample_probes_visible, hj_sample_probes_visible_placed
  return probe_vis_volume_check(ctx, fn, l->desc, l->vis, l->probes, l->atlas, l->placement, l->placement != nullptr, any, lit.g, np, lit.v, reads_atlas);
}

// Behind the gate: the volume's device arrays - the caller's own, or staged copies enqueued on the context's stream, once a call
int lit_stage(hj_context* ctx, const char* fn, const hj_probe_lighting* l, uint32_t np, bool reads_atlas, Lit& lit) {
  const bool on_device = ((l->vis ? l->vis->flags & HJ_PROBE_VIS_DEVICE_ARRAYS : l->desc->flags & HJ_PROBES_DEVICE_ARRAYS)) != 0;
  lit.d_probes = reinterpret_cast<const float4*>(l->probes);
  lit.d_atlas = reads_atlas ? reinterpret_cast<const float2*>(l->atlas) : nullptr;
  lit.d_place = reinterpret_cast<const float4*>(l->placement);
  if (on_device) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::ProbeLit& q = ctx->probe_lit;
  const size_t probe_bytes = sizeof(float4) * hj::kPvVec * (size_t)np, place_bytes = sizeof(float4) * (size_t)np;
  const size_t atlas_bytes = reads_atlas ? sizeof(float) * HJ_PROBE_VIS_WORDS(lit.v.res) * (size_t)np : 0;
  HJ_TRY(dev_alloc(ctx, q.volume, probe_bytes));
  if (reads_atlas) HJ_TRY(dev_alloc(ctx, q.atlas, atlas_bytes));
  if (l->placement) HJ_TRY(dev_alloc(ctx, q.placement, place_bytes));
  hipError_t e = hipMemcpyAsync(q.volume.p, l->probes, probe_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && reads_atlas) e = hipMemcpyAsync(q.atlas.p, l->atlas, atlas_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && l->placement) e = hipMemcpyAsync(q.placement.p, l->placement, place_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return drain(ctx, fn, e);
  lit.d_probes = static_cast<const float4*>(q.volume.p);
  lit.d_atlas = reads_atlas ? static_cast<const float2*>(q.atlas.p) : nullptr;
  lit.d_place = l->placement ? static_cast<const float4*>(q.placement.p) : nullptr;
  return HJ_OK;
}

}  // namespace hjapi

namespace {

int lit_render(hj_context* ctx, const char* fn, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t max_follow,
               uint32_t flags, const hj_probe_lighting* lighting, uint32_t np, bool reads_atlas, Lit& lit, float* image) {
  if (num_blocks != 0) HJ_TRY(lit_stage(ctx, fn, lighting, np, reads_atlas, lit));
  const AovStage stage{HJ_PROBE_LIT_WORDS, lit_reserve, lit_points, lit_resolve, &lit};
  return aov_render(ctx, fn, blocks, num_blocks, width, height, flags, image, max_follow, &stage);
}

}  // namespace

extern "C" {

// The argument checks come first and need neither a device nor a context's state: aov_check's, max_follow, the volume's; then the
// queries' gate.
int hj_render_probe_lit(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t max_follow,
                        uint32_t flags, const hj_probe_lighting* lighting, float* image) {
  HJ_TRY(aov_check(ctx, __func__, blocks, num_blocks, width, height, flags, image));
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", __func__, max_follow, (unsigned)HJ_AOV_MAX_FOLLOW);
  Lit lit;
  uint32_t np = 0;
  bool reads_atlas = false;
  HJ_TRY(lit_check(ctx, __func__, lighting, num_blocks != 0, lit, np, reads_atlas));
  HJ_TRY(query_gate(ctx, __func__));
  return lit_render(ctx, __func__, blocks, num_blocks, width, height, max_follow, flags, lighting, np, reads_atlas, lit, image);
}

int hj_render_probe_lit_frame(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin, uint32_t pass_end,
                              uint32_t max_follow, uint32_t flags, const hj_probe_lighting* lighting, float* image) {
  HJ_TRY(aov_check(ctx, __func__, nullptr, 0, width, height, flags, image));
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", __func__, max_follow, (unsigned)HJ_AOV_MAX_FOLLOW);
  if (pass_begin > pass_end || pass_end > spp) return set_error(ctx, HJ_ERR_INVALID, "%s: bad pass range [%u,%u) of %u", __func__, pass_begin, pass_end, spp);
  Lit lit;
  uint32_t np = 0;
  bool reads_atlas = false;
  HJ_TRY(lit_check(ctx, __func__, lighting, pass_begin != pass_end, lit, np, reads_atlas));
  HJ_TRY(query_gate(ctx, __func__));
  std::vector<hj_image_block> blocks;
  HJ_TRY(aov_frame_blocks(ctx, __func__, width, height, master_seed, pass_begin, pass_end, blocks));
  return lit_render(ctx, __func__, blocks.data(), blocks.size(), width, height, max_follow, flags, lighting, np, reads_atlas, lit, image);
}

}  // extern "C"
