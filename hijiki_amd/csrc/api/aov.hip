// hj_eval_materials, hj_render_aovs, hj_render_aovs_frame: what colour a surface has, and a frame's auxiliary buffers - albedo,
// normal, depth, emission, coverage - from the frame's own primary rays ("Frame AOVs and material queries").
//
// The kernels are kernels/hj_aov.h's; that header includes the kernel headers up to hj_stages.h and edits none, and no other unit's
// machine code depends on this one.
//   materials:  k_mat_eval, one lane per record; chunks and staging through hj_context::Aov are chunked_query's (api/hj_internal.h)
//   AOVs:       the ordered block list is cut into RUNS - maximal stretches of blocks with pairwise disjoint pixel rectangles (a
//               frame's pass is one) - and into walk launches of HJ_TRACE_CHUNK sample slots, rounded to whole blocks.  A walk
//               launch (k_aov_walk) may span several runs; behind it every run's part of it resolves in a launch of its own
//               (k_aov_resolve), in order on the context's stream: inside a launch no two samples share a pixel, across launches
//               the stream orders them - block order without an atomic.
//   followed:   hj_render_aovs_followed, hj_render_aovs_frame_followed: the same checks, runs and camera walk; behind each walk launch
//               the follow rounds and in k_aov_resolve's place the followed resolve, both api/follow.hip's (kernels/hj_follow.h)
//   for api/probe_lit.hip: aov_check, aov_frame_blocks and aov_render with an AovStage (hj_internal.h) - its image, its stage behind
//               the follow rounds and its resolve in the AOV resolves' place; without one aov_render enqueues what it always did
#include "hj_internal.h"
#include "../kernels/hj_aov.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

constexpr uint32_t kAovMaxSide = 16384u;

// Where each run of `blocks` ends: run k is blocks [ends[k - 1], ends[k]).  A block's pixels are origin + [0, min(dimension,
// image)) clipped to the image, as k_aov_resolve writes them (camera_ray compares the LOCAL pixel with the image size); a block
// joins the current run unless its rectangle meets one already in it.  The run's rectangles are kept per 128 x 128 cell of the
// image - a rectangle of at most 128 x 128 pixels meets at most four -, so the cut costs a few comparisons a block.
std::vector<size_t> cut_runs(const hj_image_block* blocks, size_t n, uint32_t width, uint32_t height) {
  struct Rect { uint32_t x0, y0, x1, y1; };
  const uint32_t cx = (width + HJ_BLOCK_SIZE - 1u) / HJ_BLOCK_SIZE, cy = (height + HJ_BLOCK_SIZE - 1u) / HJ_BLOCK_SIZE;
  std::vector<std::vector<Rect>> cells((size_t)cx * cy);
  std::vector<size_t> touched, ends;
  for (size_t i = 0; i < n; i++) {
    const hj_image_block& b = blocks[i];
    Rect r{b.origin[0], b.origin[1], 0u, 0u};
    const bool empty = r.x0 >= width || r.y0 >= height || b.dimension[0] == 0 || b.dimension[1] == 0;
    if (empty) continue;                                           // (writes no pixel: part of whatever run it falls into)
    r.x1 = r.x0 + std::min(std::min(b.dimension[0], width), width - r.x0);
    r.y1 = r.y0 + std::min(std::min(b.dimension[1], height), height - r.y0);
    const uint32_t c0x = r.x0 / HJ_BLOCK_SIZE, c1x = (r.x1 - 1u) / HJ_BLOCK_SIZE, c0y = r.y0 / HJ_BLOCK_SIZE, c1y = (r.y1 - 1u) / HJ_BLOCK_SIZE;
    bool meets = false;
    for (uint32_t y = c0y; y <= c1y && !meets; y++)
      for (uint32_t x = c0x; x <= c1x && !meets; x++)
        for (const Rect& o : cells[(size_t)y * cx + x])
          if (r.x0 < o.x1 && o.x0 < r.x1 && r.y0 < o.y1 && o.y0 < r.y1) { meets = true; break; }
    if (meets) {                                                   // block i starts the next run
      ends.push_back(i);
      for (size_t c : touched) cells[c].clear();
      touched.clear();
    }
    for (uint32_t y = c0y; y <= c1y; y++)
      for (uint32_t x = c0x; x <= c1x; x++) {
        cells[(size_t)y * cx + x].push_back(r);
        touched.push_back((size_t)y * cx + x);
      }
  }
  ends.push_back(n);
  return ends;
}

}  // namespace

namespace hjapi {

// What both AOV calls refuse of (blocks, image, flags, aov), without a device, in the header's order
int aov_check(hj_context* ctx, const char* fn, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t flags,
              const float* aov) {
  if (num_blocks != 0 && !blocks) return set_error(ctx, HJ_ERR_INVALID, "%s: null blocks", fn);
  if (!aov) return set_error(ctx, HJ_ERR_INVALID, "%s: null aov", fn);
  if (flags & ~(uint32_t)HJ_AOV_DEVICE_ARRAY) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown flag bits 0x%x", fn, flags);
  if (width == 0 || height == 0 || width > kAovMaxSide || height > kAovMaxSide)
    return set_error(ctx, HJ_ERR_INVALID, "%s: image %u x %u: 1 ... %u each", fn, width, height, kAovMaxSide);
  for (size_t i = 0; i < num_blocks; i++) {
    const hj_image_block& b = blocks[i];
    if (b.original_dimension[0] != width || b.original_dimension[1] != height)
      return set_error(ctx, HJ_ERR_INVALID, "%s: block %zu: original_dimension %u x %u != image %u x %u", fn, i, b.original_dimension[0],
                       b.original_dimension[1], width, height);
    if (b.dimension[0] > HJ_BLOCK_SIZE || b.dimension[1] > HJ_BLOCK_SIZE)
      return set_error(ctx, HJ_ERR_INVALID, "%s: block %zu: dimension %u x %u above %u", fn, i, b.dimension[0], b.dimension[1], (unsigned)HJ_BLOCK_SIZE);
  }
  if ((flags & HJ_AOV_DEVICE_ARRAY) && misaligned(aov))
    return set_error(ctx, HJ_ERR_INVALID, "%s: a device array must be 16-byte aligned", fn);
  return HJ_OK;
}

// Behind the checks and the gate: the image zeroed, then walk launches and their runs' resolves in list order.  max_follow > 0
// (the followed calls): behind each walk launch the follow rounds of api/follow.hip, and a launch that took one resolves through its
// resolve; max_follow == 0 enqueues exactly what it always did.  stage (api/probe_lit.hip): the image has stage->words floats a pixel,
// stage->points runs behind the rounds of each walk launch and stage->resolve takes the place of both resolves.
int aov_render(hj_context* ctx, const char* fn, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t flags,
               float* aov, uint32_t max_follow, const AovStage* stage) {
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const bool on_device = (flags & HJ_AOV_DEVICE_ARRAY) != 0;
  const size_t image_bytes = (size_t)width * height * (stage ? stage->words : (uint32_t)HJ_AOV_WORDS) * sizeof(float);
  hj_context::Aov& q = ctx->aov;
  float4* d_aov = reinterpret_cast<float4*>(aov);
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, q.image, image_bytes));
    d_aov = static_cast<float4*>(q.image.p);
  }
  // blocks of one walk launch: HJ_TRACE_CHUNK sample slots, rounded down to whole blocks, at least one
  const size_t per_launch = std::max<size_t>(1u, std::min<size_t>((size_t)ctx->tuning.trace_chunk, 0x7FFFFFFFu) / hj::kSlotsPerBlock);
  const hj_image_block* d_blocks = nullptr;
  float4* d_hits = nullptr;
  if (num_blocks != 0) {
    HJ_TRY(dev_alloc(ctx, q.blocks, num_blocks * sizeof(hj_image_block)));
    HJ_TRY(dev_alloc(ctx, q.hits, std::min(num_blocks, per_launch) * hj::kSlotsPerBlock * sizeof(float4)));
    if (max_follow != 0) HJ_TRY(aov_follow_reserve(ctx, std::min(num_blocks, per_launch) * hj::kSlotsPerBlock));
    if (stage) HJ_TRY(stage->reserve(ctx, *stage, std::min(num_blocks, per_launch) * hj::kSlotsPerBlock));
    d_blocks = static_cast<const hj_image_block*>(q.blocks.p);
    d_hits = static_cast<float4*>(q.hits.p);
  }
  const std::vector<size_t> ends = cut_runs(blocks, num_blocks, width, height);
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const dim3 blk(hj::kBlockThreads);
  hipError_t e = hipMemsetAsync(d_aov, 0, image_bytes, s);
  if (e == hipSuccess && num_blocks != 0) e = hipMemcpyAsync(q.blocks.p, blocks, num_blocks * sizeof(hj_image_block), hipMemcpyHostToDevice, s);
  size_t run = 0;
  for (size_t c0 = 0; c0 < num_blocks && e == hipSuccess; c0 += per_launch) {
    const size_t c1 = std::min(num_blocks, c0 + per_launch);
    const uint32_t nb = (uint32_t)(c1 - c0), n = nb * hj::kSlotsPerBlock;
    const uint32_t wg_rays = walk_wg_rays(ctx, n);                   // sample slots per workgroup: hj_trace_rays' rule
    const dim3 grid((n + wg_rays - 1u) / wg_rays);
    if (sc.has_pairs != 0) hipLaunchKernelGGL(hj::k_aov_walk<true>, grid, blk, 0, s, sc, d_blocks + c0, nb, wg_rays, d_hits);
    else hipLaunchKernelGGL(hj::k_aov_walk<false>, grid, blk, 0, s, sc, d_blocks + c0, nb, wg_rays, d_hits);
    e = hipGetLastError();
    bool followed = false;
    if (e == hipSuccess && max_follow != 0) e = aov_follow_rounds(ctx, d_blocks + c0, nb, d_hits, max_follow, followed);
    if (e == hipSuccess && stage) e = stage->points(ctx, *stage, d_blocks + c0, nb, d_hits, followed);
    // the parts of the runs that lie in [c0, c1), in order
    for (size_t at = c0; at < c1 && e == hipSuccess;) {
      while (ends[run] <= at) run++;
      const size_t to = std::min(c1, ends[run]);
      const uint32_t b0 = (uint32_t)(at - c0), cnt = (uint32_t)(to - at);
      if (stage) stage->resolve(ctx, *stage, d_blocks + c0, nb, b0, cnt, d_hits, followed, width, height, d_aov);
      else if (followed) aov_follow_resolve(ctx, d_blocks + c0, nb, b0, cnt, d_hits, width, height, d_aov);
      else hipLaunchKernelGGL(hj::k_aov_resolve, per_lane(cnt * hj::kSlotsPerBlock), blk, 0, s, sc, d_blocks + c0, nb, b0, cnt,
                              static_cast<const float4*>(d_hits), width, height, d_aov);
      e = hipGetLastError();
      at = to;
    }
  }
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(aov, d_aov, image_bytes, hipMemcpyDeviceToHost, s);
  return drain(ctx, fn, e);
}

// The block list of hj_render_frame for world == 1 (frame_blocks_append: one text for both), whole: 40 bytes a block.
int aov_frame_blocks(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, uint64_t master_seed, uint32_t pass_begin, uint32_t pass_end,
                     std::vector<hj_image_block>& blocks) {
  try {
    const hijiki::BlockGrid grid(width, height, HJ_BLOCK_SIZE);
    blocks.reserve((size_t)(pass_end - pass_begin) * grid.per_pass());
    frame_blocks_append(grid, master_seed, pass_begin, pass_end, 0u, 1u, false, blocks);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, HJ_ERR_NOMEM, "%s: no memory for the block list of %u passes", fn, pass_end - pass_begin);
  }
  return HJ_OK;
}

}  // namespace hjapi

extern "C" {

// The argument checks come first, in hj_trace_rays' style, and need neither a device nor a context's state; then the queries' gate.
int hj_eval_materials(hj_context* ctx, const float* hits, const float* surface, size_t n, uint32_t flags, float* out) {
  if (n != 0 && (!hits || !surface || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_eval_materials: null %s", !hits ? "hits" : !surface ? "surface" : "out");
  if (flags & ~(uint32_t)HJ_MATERIALS_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_eval_materials: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_MATERIALS_DEVICE_ARRAYS) != 0;
  if (n != 0) {
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_eval_materials: %zu records, at most 2^31 - 1 a call", n);
    if (on_device && misaligned(hits, surface, out))
      return set_error(ctx, HJ_ERR_INVALID, "hj_eval_materials: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  hj_context::Aov& q = ctx->aov;
  const size_t f4 = sizeof(float4);
  const QueryArray arrays[] = {{hits, &q.in_hits, f4, false}, {surface, &q.in_surface, 4 * f4, false}, {out, &q.out, 2 * f4, true}};
  return chunked_query(ctx, __func__, n, on_device, arrays, [&](void* const d[], uint32_t cnt, size_t) {
    hipLaunchKernelGGL(hj::k_mat_eval, per_lane(cnt), dim3(hj::kBlockThreads), 0, ctx->stream, ctx->scene, static_cast<const float4*>(d[0]),
                       static_cast<const float4*>(d[1]), cnt, static_cast<float4*>(d[2]));
    return hipGetLastError();
  });
}

int hj_render_aovs(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t flags, float* aov) {
  HJ_TRY(aov_check(ctx, __func__, blocks, num_blocks, width, height, flags, aov));
  HJ_TRY(query_gate(ctx, __func__));
  return aov_render(ctx, __func__, blocks, num_blocks, width, height, flags, aov, 0u, nullptr);
}

// hj_render_aovs with the chains followed through at most max_follow specular surfaces (api/follow.hip); 0: hj_render_aovs' launches
int hj_render_aovs_followed(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t max_follow,
                            uint32_t flags, float* aov) {
  HJ_TRY(aov_check(ctx, __func__, blocks, num_blocks, width, height, flags, aov));
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", __func__, max_follow, (unsigned)HJ_AOV_MAX_FOLLOW);
  HJ_TRY(query_gate(ctx, __func__));
  return aov_render(ctx, __func__, blocks, num_blocks, width, height, flags, aov, max_follow, nullptr);
}

static int aov_render_frame(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin,
                            uint32_t pass_end, uint32_t max_follow, uint32_t flags, float* aov) {
  HJ_TRY(aov_check(ctx, fn, nullptr, 0, width, height, flags, aov));
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", fn, max_follow, (unsigned)HJ_AOV_MAX_FOLLOW);
  if (pass_begin > pass_end || pass_end > spp) return set_error(ctx, HJ_ERR_INVALID, "%s: bad pass range [%u,%u) of %u", fn, pass_begin, pass_end, spp);
  HJ_TRY(query_gate(ctx, fn));
  std::vector<hj_image_block> blocks;
  HJ_TRY(aov_frame_blocks(ctx, fn, width, height, master_seed, pass_begin, pass_end, blocks));
  return aov_render(ctx, fn, blocks.data(), blocks.size(), width, height, flags, aov, max_follow, nullptr);
}

int hj_render_aovs_frame(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin, uint32_t pass_end,
                         uint32_t flags, float* aov) {
  return aov_render_frame(ctx, __func__, width, height, spp, master_seed, pass_begin, pass_end, 0u, flags, aov);
}

int hj_render_aovs_frame_followed(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin,
                                  uint32_t pass_end, uint32_t max_follow, uint32_t flags, float* aov) {
  return aov_render_frame(ctx, __func__, width, height, spp, master_seed, pass_begin, pass_end, max_follow, flags, aov);
}

}  // extern "C"
