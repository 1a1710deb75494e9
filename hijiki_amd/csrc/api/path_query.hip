// hj_trace_paths: path-traced radiance along caller-given rays - the public path query ("Path queries").
//
// The rounds are the fused path kernel's (kernels/hj_path_kernel.h, its loop over EXPLICIT path records): top-up, the merged walk of
// closest-hit and shadow rays, hit compaction by material tag, shade - the stages of kernels/hj_stages.h, called as that kernel calls
// them.  Nothing of the kernel headers is restated or edited: this unit includes them (as api/ray_query.hip does) and defines kernels
// of its own beside the path kernels.  The round loop is api/query_round_loop.h, the text k_gq_paths (api/gather_query.hip) includes
// too; this unit's own text is the top-up, which takes its paths from the caller's ray array instead of the camera.
//   k_pq_paths<PAIRS, ENV>  one persistent launch per chunk of samples: workgroup g owns the 64-sample groups g, g + num_wg, ...
//   k_pq_resolve            one thread per ray: the float32 sum of its spp samples in ascending order, first-hit normal and t
// The one-wave tail of the path kernel (HJ_TAIL1 there, kQueryTail here) is KEPT: a query's last long paths are as few as a batch's.
// Host code the queries share lives here too (namespace hjapi, declared in hj_internal.h): path_query_plan and path_query_pass, the
// render-opts check and the context gate of the entry points, per_lane, the statistics read-back (QueryStats), and fixed_spp_query,
// the driver of hj_trace_paths and hj_trace_irradiance.
#include "hj_internal.h"
#include <type_traits>
#include "../kernels/hj_stages.h"
#include "query_round.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

// What the kernel's argument segment holds behind (BatchState, DeviceScene).  A sample is s = ray * spp + k, k < spp; the chunk's
// samples are [0, num_samples), num_samples <= 2^31 - 1 (the sample index shares its word with kCameraFlag).
struct PathQueryArgs {
  const float4* src;      // two float4 per ray: origin.xyz, direction.x | direction.yz, seed bits, reserved
  uint32_t spp;
  uint32_t num_samples;
  uint32_t max_bounces;
  uint32_t rr_start;
};

// Top-up from the caller's rays: paths for groups [k0, k0 + ngen) of this workgroup's sample sequence, written to the path arrays of
// `parity` behind the n0 continuing paths (positions n0 + sh.n_gen...; the caller guarantees n0 + 64 * ngen <= pool).  A path starts
// as a camera path does (render.glsl:86-90,156): RNG state rng_seed(seed + k) with uint32 wrap-around, throughput 1, extinction 0,
// wasDiscrete, bounce 0, and kCameraFlag beside the sample index so that the walk gives its first segment tMin = eps.  The direction
// is used as given.  (A group index is below 2^25 and the last group's samples below 2^31 + 64: no 32-bit wrap.)
HJ_DEV void stage_gen_rays(const BatchState& st, const DeviceScene& sc, const float4* __restrict__ rays, uint32_t spp, uint32_t num_samples,
                           uint32_t g, WgShared& sh, uint32_t parity, uint32_t n0, uint32_t k0, uint32_t ngen, uint32_t waves) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t seg = g * st.pool + n0;
  for (uint32_t k = k0 + wave; k < k0 + ngen; k += waves) {
    const uint32_t s = (g + k * st.num_wg) * 64u + lane;
    const bool valid = s < num_samples;
    const uint32_t qi = lds_push(&sh.n_gen, valid);
    if (valid) {
      const uint32_t i = s / spp, j = s - i * spp;
      const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
      const uint32_t pos = seg + qi;
      // the sample index rides in origin.w, the RNG state in direction.w
      stp<false>(st.ray_o[parity], pos, make_float4(a.x, a.y, a.z, __uint_as_float(s | kCameraFlag)));
      stp<false>(st.ray_d[parity], pos, make_float4(a.w, b.x, b.y, __uint_as_float(rng_seed(__float_as_uint(b.z) + j))));
      stp<false>(st.thr[parity], pos, make_float4(1.f, 1.f, 1.f, __uint_as_float(1u)));   // wasDiscrete = true, bounce 0
      if (sc.has_extinction) stp<false>(st.ext[parity], pos, make_float4(0.f, 0.f, 0.f, 0.f));
      stp<false>(st.smp_rgb, s, make_float4(0.f, 0.f, 0.f, 1.f));
      stp<false>(st.smp_nd, s, make_float4(0.f, 0.f, 0.f, 0.f));
    }
  }
}

// ... as a CALLED function, like the other stages (kernels/hj_stages.h: own register allocation, the walk stays free of its
// registers).  The ray array's address comes in two halves, as the argument segment's does.  ENV only makes the environment
// kernels' instantiation a function of its own.
template <bool ENV>
__device__ __attribute__((noinline)) void stage_gen_rays_call(uint32_t ka_lo, uint32_t ka_hi, uint32_t rays_lo, uint32_t rays_hi, uint32_t spp,
                                                               uint32_t num_samples, uint32_t g, uint32_t sh_lds, uint32_t parity, uint32_t n0,
                                                               uint32_t k0, uint32_t ngen, uint32_t waves) {
  const StageCtx c = stage_ctx(ka_lo, ka_hi, sh_lds);
  const float4* rays = (const float4*)(((uint64_t)uni(rays_hi) << 32) | (uint64_t)uni(rays_lo));
  stage_gen_rays(c.st, c.sc, rays, uni(spp), uni(num_samples), uni(g), c.sh, uni(parity), uni(n0), uni(k0), uni(ngen), uni(waves));
}

// One persistent launch per chunk of samples: the round loop of api/query_round_loop.h with the top-up above.
template <bool PAIRS, bool ENV>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(HJ_QUERY_WAVES, 8))) void k_pq_paths(BatchState st, DeviceScene sc, PathQueryArgs q) {
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
#define HJ_QUERY_TOP_UP stage_gen_rays_call<ENV>
#include "query_round_loop.h"
#undef HJ_QUERY_TOP_UP
}

// samples: two float4 per ray = (sum of the ray's spp sample radiances in ascending k, starting from +0, in float32; (float)spp),
// (first-hit normal, first-hit t) of sample ray * spp - the same for every k: the first segment does not depend on the RNG.
__global__ __launch_bounds__(kBlockThreads) void k_pq_resolve(const float4* __restrict__ smp_rgb, const float4* __restrict__ smp_nd, uint32_t spp,
                                                              uint32_t n, float4* __restrict__ samples) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s0 = i * spp;               // (below the chunk's sample count: no wrap)
  float r = 0.f, g = 0.f, b = 0.f;
  for (uint32_t k = 0; k < spp; k++) {
    const float4 v = smp_rgb[s0 + k];
    r += v.x; g += v.y; b += v.z;
  }
  samples[2 * (size_t)i] = make_float4(r, g, b, (float)spp);
  samples[2 * (size_t)i + 1] = smp_nd[s0];
}

}  // namespace hj

namespace hjapi {

// The shape of a fixed-spp pass over at most n rays.  A launch takes whole rays: at most HJ_PATHS_CHUNK samples (one ray when spp
// alone exceeds it: spp <= 65536), dealt in 64-sample groups over at most HJ_PATHS_WGS workgroups of at most HJ_PATHS_POOL positions
// each - fewer positions when the busiest workgroup has fewer samples than that.  (G x pool <= 4096 * 2^19: a position is a uint32.)
PathQueryPlan path_query_plan(const Tuning& tn, size_t n, uint32_t spp) {
  PathQueryPlan p;
  p.chunk_rays = std::max<size_t>(1, (size_t)tn.paths_chunk / spp);
  p.most_rays = std::min(n, p.chunk_rays);
  p.most_samples = p.most_rays * spp;
  const size_t most_groups = (p.most_samples + 63) / 64;
  p.G = (uint32_t)std::min<size_t>((size_t)tn.paths_wgs, most_groups);
  const uint32_t per_wg = (uint32_t)((most_groups + p.G - 1) / p.G) * 64u;              // samples of the busiest workgroup
  p.pool = std::min(per_wg, (uint32_t)tn.paths_pool / 64u * 64u);
  return p;
}

// One launch of the path kernel: cnt rays at d_rays, spp samples each, into the sample arrays of st (num_samples = cnt * spp <=
// 2^31 - 1: HJ_PATHS_CHUNK's upper bound).  Fewer workgroups when the chunk has fewer 64-sample groups (the last chunk); the
// segments stay st.pool positions long.  st: num_wg and the statistics pointers are set for this launch (set_num_wg).
void path_query_pass(hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_rays, uint32_t cnt, uint32_t spp,
                     const hj_render_opts& o, hipStream_t s) {
  const uint32_t num_samples = cnt * spp;
  set_num_wg(st, std::min<uint32_t>(G, (num_samples + 63u) / 64u));
  hj::PathQueryArgs q{d_rays, spp, num_samples, o.max_bounces, o.rr_start};
  const dim3 grid(st.num_wg), blk(hj::kBlockThreads);
  const bool pairs = sc.has_pairs != 0, env = sc.env_alias != nullptr;
  if (pairs && env) hipLaunchKernelGGL((hj::k_pq_paths<true, true>), grid, blk, 0, s, st, sc, q);
  else if (pairs) hipLaunchKernelGGL((hj::k_pq_paths<true, false>), grid, blk, 0, s, st, sc, q);
  else if (env) hipLaunchKernelGGL((hj::k_pq_paths<false, true>), grid, blk, 0, s, st, sc, q);
  else hipLaunchKernelGGL((hj::k_pq_paths<false, false>), grid, blk, 0, s, st, sc, q);
}

// ---- what the query entry points share (declared in hj_internal.h; host code only) ----

dim3 per_lane(uint32_t n) { return dim3((n + hj::kBlockThreads - 1u) / hj::kBlockThreads); }

// opts (NULL: the defaults) into o, and the refusals every path-type query has for them
int query_render_opts(hj_context* ctx, const char* fn, const hj_render_opts* opts, hj_render_opts& o) {
  if (opts) o = *opts;
  else hj_default_render_opts(&o);
  if (o.max_bounces == 0) return set_error(ctx, HJ_ERR_INVALID, "%s: max_bounces must be >= 1", fn);
  if (o.use_bvh == 0) return set_error(ctx, HJ_ERR_UNSUPPORTED, "%s: the tree is always walked (use_bvh == 0: there is no linear-scan form)", fn);
  if (o.flags & ~(uint32_t)HJ_RENDER_NO_LIGHT_GRID)
    return set_error(ctx, HJ_ERR_INVALID, "%s: of the HJ_RENDER_* bits only HJ_RENDER_NO_LIGHT_GRID applies (flags 0x%x)", fn, o.flags);
  return HJ_OK;
}

// A process without a HIP device cannot hold a context: a call that is otherwise valid gets HJ_ERR_DEVICE there, like every entry
// point that computes.
int context_gate(hj_context* ctx, const char* fn) {
  if (!ctx) {
    if (hj_device_count() == 0) return set_error(nullptr, HJ_ERR_DEVICE, "%s: no HIP device available; this library has no CPU fallback", fn);
    return set_error(nullptr, HJ_ERR_INVALID, "%s: null context", fn);
  }
  HJ_NOT_BUSY_IN(ctx, fn);
  HJ_NOT_PIPELINED_IN(ctx, fn);
  return HJ_OK;
}

int query_gate(hj_context* ctx, const char* fn) {
  HJ_TRY(context_gate(ctx, fn));
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "%s: no scene has been uploaded", fn);
  return HJ_OK;
}

int QueryStats::reserve(hj_context* ctx, const char* fn, size_t launches, uint32_t G_) {
  G = G_;
  try {
    if (on) h_acc.assign(launches * kStatWords * G, 0u);
  } catch (const std::bad_alloc&) {
    (void)hipStreamSynchronize(ctx->stream);                      // (nothing of this call stays in flight)
    return set_error(ctx, HJ_ERR_NOMEM, "%s: out of host memory", fn);
  }
  return HJ_OK;
}

hipError_t QueryStats::enqueue(size_t launch, const hj::BatchState& st, hipStream_t s) {
  if (!on) return hipSuccess;
  return hipMemcpyAsync(h_acc.data() + launch * kStatWords * G, st.acc_closest, sizeof(uint32_t) * kStatWords * st.num_wg, hipMemcpyDeviceToHost, s);
}

void QueryStats::add(hj_render_stats& to, size_t chunk_rays, size_t len, uint32_t spp) const {
  if (!on) return;
  size_t launch = 0;
  for (size_t at = 0; at < len; at += chunk_rays, launch++) {
    const size_t cnt = std::min(chunk_rays, len - at);
    add_stat_words(to, h_acc.data() + launch * kStatWords * G, std::min<size_t>(G, (cnt * spp + 63) / 64));
  }
}

int fixed_spp_query(hj_context* ctx, const FixedSppQuery& q) {
  const size_t n = q.n, rec = q.rec;
  const uint32_t spp = q.spp;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const auto wall0 = std::chrono::steady_clock::now();

  // Sizes (path_query_plan above).  A launch takes whole rays.
  const Tuning& tn = ctx->tuning;
  const PathQueryPlan plan = path_query_plan(tn, n, spp);
  const size_t chunk_rays = plan.chunk_rays, most_rays = plan.most_rays;
  const uint32_t G = plan.G;
  const size_t f4 = sizeof(float4);
  const hj::DeviceScene sc = scene_for(ctx, q.o);

  // Per-workgroup arrays for HJ_PATHS_WGS workgroups, the most a call uses: two calls can need the same number of positions with
  // different workgroup counts.  st.capacity: the samples allocated, not this call's.
  hj_context::PathQuery& pq = ctx->paths;
  if (const int rc = ensure_path_state(ctx, pq, plan.most_samples, G, (uint32_t)tn.paths_wgs, plan.pool, sc.has_extinction != 0, sc.env_alias != nullptr)) {
    release_path_state(pq);
    return rc;
  }
  hj::BatchState st = pq.st;
  float4 *d_in = nullptr, *d_out = nullptr;
  if (!q.on_device) {
    HJ_TRY(dev_alloc(ctx, pq.in_rays, most_rays * 2 * f4));
    HJ_TRY(dev_alloc(ctx, pq.out_samples, most_rays * rec * f4));
    d_in = static_cast<float4*>(pq.in_rays.p);
    d_out = static_cast<float4*>(pq.out_samples.p);
  }
  const size_t launches = (n + chunk_rays - 1) / chunk_rays;
  QueryStats acc(q.stats != nullptr);
  HJ_TRY(acc.reserve(ctx, q.name, launches, G));

  hipError_t e = hipSuccess;
  size_t launch = 0;
  for (size_t at = 0; at < n && e == hipSuccess; at += chunk_rays, launch++) {
    const uint32_t cnt = (uint32_t)std::min(chunk_rays, n - at);
    if (q.on_device) {
      d_in = reinterpret_cast<float4*>(const_cast<float*>(q.in)) + 2 * at;
      d_out = reinterpret_cast<float4*>(q.out) + rec * at;
    } else {
      e = hipMemcpyAsync(d_in, q.in + 8 * at, cnt * 2 * f4, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) break;
    }
    q.chunk(q, st, sc, G, d_in, cnt, d_out, ctx->stream);
    e = hipGetLastError();
    if (e == hipSuccess && !q.on_device) e = hipMemcpyAsync(q.out + 4 * rec * at, d_out, cnt * rec * f4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = acc.enqueue(launch, st, ctx->stream);
  }
  HJ_TRY(drain(ctx, q.name, e));
  if (q.stats) {
    std::memset(q.stats, 0, sizeof *q.stats);
    acc.add(*q.stats, chunk_rays, n, spp);
    q.stats->paths = (uint64_t)n * spp;
    q.stats->batches = launches;
    q.stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  return HJ_OK;
}

}  // namespace hjapi

// the path launch and the resolve of one chunk (FixedSppQuery::chunk)
static void paths_chunk(const FixedSppQuery& q, hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_rays, uint32_t cnt,
                        float4* d_out, hipStream_t s) {
  path_query_pass(st, sc, G, d_rays, cnt, q.spp, q.o, s);
  hipLaunchKernelGGL(hj::k_pq_resolve, per_lane(cnt), dim3(hj::kBlockThreads), 0, s,
                     static_cast<const float4*>(st.smp_rgb), static_cast<const float4*>(st.smp_nd), q.spp, cnt, d_out);
}

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_rays' order and style).
int hj_trace_paths(hj_context* ctx, const float* rays, size_t n, uint32_t spp, const hj_render_opts* opts, uint32_t flags, float* samples,
                   hj_render_stats* stats) {
  if (n != 0 && (!rays || !samples)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: null %s", !rays ? "rays" : "samples");
  if (flags & ~(uint32_t)HJ_PATHS_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_PATHS_DEVICE_ARRAYS) != 0;
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: spp %u outside [1, 65536]", spp);
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: %zu rays, at most 2^31 - 1 a call", n);
  if (n != 0 && on_device && misaligned(rays, samples))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: device arrays must be 16-byte aligned");
  FixedSppQuery q{__func__, rays, n, spp, 2, on_device, samples, stats, {}, paths_chunk, flags};
  HJ_TRY(query_render_opts(ctx, __func__, opts, q.o));
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  return fixed_spp_query(ctx, q);
}

}  // extern "C"
