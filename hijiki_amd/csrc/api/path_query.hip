// hj_trace_paths: path-traced radiance along caller-given rays - the public path query ("Path queries").
//
// The rounds are the fused path kernel's (kernels/hj_path_kernel.h, its loop over EXPLICIT path records): top-up, the merged walk of
// closest-hit and shadow rays, hit compaction by material tag, shade - the stages of kernels/hj_stages.h, called as that kernel calls
// them.  Nothing of the kernel headers is restated or edited: this unit includes them (as api/ray_query.hip does) and defines kernels
// of its own beside the path kernels.  The one new text is the top-up, which takes its paths from the caller's ray array instead of
// the camera.
//   k_pq_paths<PAIRS, ENV>  one persistent launch per chunk of samples: workgroup g owns the 64-sample groups g, g + num_wg, ...
//   k_pq_resolve            one thread per ray: the float32 sum of its spp samples in ascending order, first-hit normal and t
// The one-wave tail of the path kernel (HJ_TAIL1 there, kPqTail here) is KEPT: a query's last long paths are as few as a batch's.
#include "hj_internal.h"
#include <type_traits>
#include "../kernels/hj_stages.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

constexpr uint32_t kPqTail = 128u;   // rays of a round at which the workgroup shrinks to one wave (the path kernel's HJ_TAIL1)
#define HJ_PQ_WAVES 7                // the path kernel's register budget (HJ_PATH_WAVES): the called stages are compiled for it

// What the kernel's argument segment holds behind (BatchState, DeviceScene).  A sample is s = ray * spp + k, k < spp; the chunk's
// samples are [0, num_samples), num_samples <= 2^31 - 1 (the sample index shares its word with kCameraFlag).
struct PathQueryArgs {
  const float4* rays;     // two float4 per ray: origin.xyz, direction.x | direction.yz, seed bits, reserved
  uint32_t spp;
  uint32_t num_samples;
  uint32_t max_bounces;
  uint32_t rr_start;
};

// 64-sample groups of workgroup g: group k of its sequence is global group g + k * num_wg (the path kernel's round-robin deal)
HJ_DEV uint32_t pq_num_groups(uint32_t num_samples, uint32_t num_wg, uint32_t g) {
  const uint32_t groups = (num_samples + 63u) / 64u;
  return groups > g ? (groups - g + num_wg - 1u) / num_wg : 0u;
}

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

// The whole life of a chunk of samples in ONE launch: the round loop of kernels/hj_path_kernel.h for explicit records (its
// non-IMPLICIT form), with the top-up above.  Path regeneration keeps about `pool` paths in flight per workgroup until its samples
// run out.  sh.cam_first stays 0xFFFFFFFF in every round: no path is implicit, so no stage reads st.blocks (null here).
// Exit condition every wave reaches, exactly as in the path kernel: the counts a round's decisions depend on (n_ray, n_gen,
// n_shadow in LDS, groups_left in every thread alike) are read by all waves between two workgroup barriers, so all waves take the
// same branch; the loop ends when there are no rays, no shadow rays and no groups left, and every path ends - a bounce ends it with
// probability >= 1 % from bounce rr_start on, and max_bounces caps it.  A wave that leaves at the one-wave tail leaves for good: the
// counts never grow again once groups_left is 0.
// No global atomic, no inline assembly; ordinary loads and stores (NT = false).  The statistics are per workgroup, summed on the host.
template <bool PAIRS, bool ENV>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(HJ_PQ_WAVES, 8))) void k_pq_paths(BatchState st, DeviceScene sc, PathQueryArgs q) {
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
  const uint32_t g = blockIdx.x;
  // (the called stages read the batch and scene descriptions from this kernel's argument segment and reach `sh` through its LDS address)
  const uint64_t ka_ = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t ka_lo = (uint32_t)ka_, ka_hi = (uint32_t)(ka_ >> 32), sh_lds = (uint32_t)(uintptr_t)(WgSharedLds)&sh;
  const uint32_t rays_lo = (uint32_t)(uintptr_t)q.rays, rays_hi = (uint32_t)((uint64_t)(uintptr_t)q.rays >> 32);
  uint32_t groups_left = pq_num_groups(q.num_samples, st.num_wg, g);
  uint32_t total_closest = 0, total_shadow = 0, total_hits = 0, total_unocc = 0, total_direct = 0;   // (thread 0's copies are published)
  if (groups_left != 0) {
    uint32_t k_next = 0;                     // next group of this workgroup's sample sequence
    if (threadIdx.x == 0) { sh.n_ray[0] = 0; sh.n_ray[1] = 0; sh.n_gen = 0; sh.n_shadow = 0; sh.n_unocc = 0; sh.n_direct = 0; sh.cam_first = 0xFFFFFFFFu; sh.cam_k0 = 0; sh.n_cam_dead = 0; }
    load_hot_nodes(sc, sh);
    uint32_t waves = blockDim.x >> 6;
    wg_sync(waves);
    for (uint32_t parity = 0;; parity ^= 1u) {
      // top-up: new paths behind the continuing ones, whole 64-sample groups while they fit
      const uint32_t n0 = uni(sh.n_ray[parity]);
      const uint32_t ngen = min(groups_left, (st.pool - n0) >> 6);
      if (ngen != 0) {
        stage_gen_rays_call<ENV>(ka_lo, ka_hi, rays_lo, rays_hi, q.spp, q.num_samples, g, sh_lds, parity, n0, k_next, ngen, waves);
        wg_sync(waves);
        k_next += ngen;
        groups_left -= ngen;
      }
      const uint32_t n = n0 + uni(sh.n_gen), ns = uni(sh.n_shadow);
      // next-event samples of the previous round's shade that the light-shaft grid answered: shadow rays of the statistics all the same
      { const uint32_t nd = uni(sh.n_direct); total_shadow += nd; total_unocc += nd; total_direct += nd; }
      if (n + ns == 0) {
        if (groups_left == 0) break;
        // (not reached with rays - every group below the chunk's count holds a sample -, kept as the path kernel has it)
        if (threadIdx.x == 0) { sh.n_ray[parity ^ 1u] = 0; sh.n_direct = 0; }
        wg_sync(waves);
        continue;
      }
      // Tail of the workgroup: one wave can hold every ray of a round and the counts never grow again.
      if (waves > 1u && groups_left == 0 && n + ns <= kPqTail) {
        wg_sync(waves);                      // (everyone has read the counts)
        if (threadIdx.x >= 64u) return;
        waves = 1u;
      }
      wg_sync(waves);                        // everyone has read the counts before they are reset
      if (threadIdx.x == 0) {
        sh.head = 0; sh.head_cam = 0; sh.n_ray[parity ^ 1u] = 0; sh.n_gen = 0; sh.n_shadow = 0; sh.n_unocc = 0; sh.n_direct = 0;
        sh.cam_first = 0xFFFFFFFFu; sh.cam_k0 = 0; sh.n_cam_dead = 0;
      }
      if (threadIdx.x < kNumTags) sh.cnt_hit[threadIdx.x] = 0;
      wg_sync(waves);
      stage_trace_merged<true, PAIRS, false>(st, sc, g, parity, n, ns, sh);
      compact_hits_call<false, 4u, ENV>(ka_lo, ka_hi, g, n, sh_lds, waves);
      wg_sync(waves);
      if (n != 0) {
        stage_shade_call<false, ENV>(ka_lo, ka_hi, g, parity, q.max_bounces, q.rr_start, sh_lds, waves);
      }
      total_closest += n;
      total_shadow += ns;
      for (uint32_t k = 0; k < kNumTags; k++) total_hits += uni(sh.cnt_hit[k]);
      total_unocc += uni(sh.n_unocc);
      wg_sync(waves);
    }
  }
  if (threadIdx.x == 0) {
    st.acc_closest[g] = total_closest;
    st.acc_shadow[g] = total_shadow;
    st.acc_hits[g] = total_hits;
    st.acc_unoccluded[g] = total_unocc;
    st.acc_direct[g] = total_direct;
  }
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

}  // namespace hjapi

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_rays' order and style).
int hj_trace_paths(hj_context* ctx, const float* rays, size_t n, uint32_t spp, const hj_render_opts* opts, uint32_t flags, float* samples,
                   hj_render_stats* stats) {
  if (n != 0 && (!rays || !samples)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: null %s", !rays ? "rays" : "samples");
  if (flags & ~(uint32_t)HJ_PATHS_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_PATHS_DEVICE_ARRAYS) != 0;
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: spp %u outside [1, 65536]", spp);
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: %zu rays, at most 2^31 - 1 a call", n);
  if (n != 0 && on_device && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(samples)) & 15u) != 0)
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: device arrays must be 16-byte aligned");
  hj_render_opts o;
  if (opts) o = *opts;
  else hj_default_render_opts(&o);
  if (o.max_bounces == 0) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: max_bounces must be >= 1");
  if (o.use_bvh == 0) return set_error(ctx, HJ_ERR_UNSUPPORTED, "hj_trace_paths: the tree is always walked (use_bvh == 0: there is no linear-scan form)");
  if (o.flags & ~(uint32_t)HJ_RENDER_NO_LIGHT_GRID)
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths: of the HJ_RENDER_* bits only HJ_RENDER_NO_LIGHT_GRID applies (flags 0x%x)", o.flags);
  if (!ctx) {
    if (hj_device_count() == 0) return set_error(nullptr, HJ_ERR_DEVICE, "hj_trace_paths: no HIP device available; this library has no CPU fallback");
    return set_error(nullptr, HJ_ERR_INVALID, "hj_trace_paths: null context");
  }
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "hj_trace_paths: no scene has been uploaded");
  if (n == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const auto wall0 = std::chrono::steady_clock::now();

  // Sizes (path_query_plan above).
  const Tuning& tn = ctx->tuning;
  const PathQueryPlan plan = path_query_plan(tn, n, spp);
  const size_t chunk_rays = plan.chunk_rays, most_rays = plan.most_rays, most_samples = plan.most_samples;
  const uint32_t G = plan.G, pool = plan.pool;
  const size_t f4 = sizeof(float4);
  const hj::DeviceScene sc = scene_for(ctx, o);

  // Per-workgroup arrays for HJ_PATHS_WGS workgroups, the most a call uses: two calls can need the same number of positions with
  // different workgroup counts.  st.capacity: the samples allocated, not this call's.
  hj_context::PathQuery& pq = ctx->paths;
  if (const int rc = ensure_path_state(ctx, pq, most_samples, G, (uint32_t)tn.paths_wgs, pool, sc.has_extinction != 0, sc.env_alias != nullptr)) {
    release_path_state(pq);
    return rc;
  }
  hj::BatchState st = pq.st;
  float4 *d_rays = nullptr, *d_out = nullptr;
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, pq.in_rays, most_rays * 2 * f4));
    HJ_TRY(dev_alloc(ctx, pq.out_samples, most_rays * 2 * f4));
    d_rays = static_cast<float4*>(pq.in_rays.p);
    d_out = static_cast<float4*>(pq.out_samples.p);
  }
  const size_t launches = (n + chunk_rays - 1) / chunk_rays;
  std::vector<uint32_t> h_acc;
  try {
    if (stats) h_acc.assign(launches * kStatWords * G, 0u);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, HJ_ERR_NOMEM, "hj_trace_paths: out of host memory");
  }

  hipError_t e = hipSuccess;
  size_t launch = 0;
  for (size_t at = 0; at < n && e == hipSuccess; at += chunk_rays, launch++) {
    const uint32_t cnt = (uint32_t)std::min(chunk_rays, n - at);
    if (on_device) {
      d_rays = reinterpret_cast<float4*>(const_cast<float*>(rays)) + 2 * at;
      d_out = reinterpret_cast<float4*>(samples) + 2 * at;
    } else {
      e = hipMemcpyAsync(d_rays, rays + 8 * at, cnt * 2 * f4, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) break;
    }
    path_query_pass(st, sc, G, d_rays, cnt, spp, o, ctx->stream);
    hipLaunchKernelGGL(hj::k_pq_resolve, dim3((cnt + hj::kBlockThreads - 1u) / hj::kBlockThreads), dim3(hj::kBlockThreads), 0, ctx->stream,
                       static_cast<const float4*>(st.smp_rgb), static_cast<const float4*>(st.smp_nd), spp, cnt, d_out);
    e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(samples + 8 * at, d_out, cnt * 2 * f4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && stats)
      e = hipMemcpyAsync(h_acc.data() + launch * kStatWords * G, st.acc_closest, sizeof(uint32_t) * kStatWords * st.num_wg, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);      // (also after a failed enqueue: nothing of this call stays in flight)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_error(ctx, HJ_ERR_DEVICE, "hj_trace_paths: %s", hipGetErrorString(e));
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    size_t at = 0;
    for (size_t l = 0; l < launches; l++, at += chunk_rays) {
      const size_t cnt = std::min(chunk_rays, n - at);
      add_stat_words(*stats, h_acc.data() + l * kStatWords * G, std::min<size_t>(G, (cnt * spp + 63) / 64));
    }
    stats->paths = (uint64_t)n * spp;
    stats->batches = launches;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  return HJ_OK;
}

}  // extern "C"
