// hj_trace_irradiance: the radiance gathered at caller-given points, the directions drawn on the device - the public gather query
// ("Gather queries").
//
// A gather sample is a path of hj_trace_paths whose first direction is drawn at the point: a cosine direction about the point's
// normal (the diffuse bounce of kernels/hj_stages.h) or a uniform direction of the sphere, from the RNG state the path then goes on
// with.  Nothing of the kernel headers is restated or edited: this unit includes them, as api/path_query.hip does, and defines
// kernels of its own beside the path kernels.
//   k_gq_paths<PAIRS, ENV, SPHERE>  one persistent launch per chunk of samples: workgroup g owns the 64-sample groups g, g + num_wg, ...
//   k_gq_resolve<SH9>               one thread per point: the float32 sums over its spp samples in ascending order, the first
//                                   segments' hit count and nearest hit, the nine SH-weighted sums
// The round loop of k_gq_paths is the TWIN of k_pq_paths' (api/path_query.hip): the same text with the top-up exchanged.  It is
// restated and not shared: as a device function template inlined into both kernels it moved k_pq_paths' machine code (the
// workgroup size is read with the kernel's bound only in a kernel's own body), and hj_trace_paths must not move.  A change to one
// loop is a change to the other.
#include "hj_internal.h"
#include <type_traits>
#include "../kernels/hj_stages.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

constexpr uint32_t kGqTail = 128u;   // rays of a round at which the workgroup shrinks to one wave (kPqTail of api/path_query.hip)
#define HJ_GQ_WAVES 7                // the path kernel's register budget (HJ_PATH_WAVES): the called stages are compiled for it

// What the kernel's argument segment holds behind (BatchState, DeviceScene).  A sample is s = point * spp + k, k < spp; the chunk's
// samples are [0, num_samples), num_samples <= 2^31 - 1 (the sample index shares its word with kCameraFlag).
struct GatherArgs {
  const float4* points;   // two float4 per point: position.xyz, normal.x | normal.yz, seed bits, reserved
  uint32_t spp;
  uint32_t num_samples;
  uint32_t max_bounces;
  uint32_t rr_start;
};

// 64-sample groups of workgroup g: group k of its sequence is global group g + k * num_wg (the path kernel's round-robin deal)
HJ_DEV uint32_t gq_num_groups(uint32_t num_samples, uint32_t num_wg, uint32_t g) {
  const uint32_t groups = (num_samples + 63u) / 64u;
  return groups > g ? (groups - g + num_wg - 1u) / num_wg : 0u;
}

// The direction of sample k of the point (a, b) - the ONE text of it: the top-up draws it, the SH reduction draws it again.
// rng: rng_seed(seed + k) with uint32 wrap-around, advanced by the two draws (the state the path goes on with).
//   SPHERE:      rand_uniform_sphere; the normal is not read
//   hemisphere:  rand_cos_hemisphere in populate_triangle's frame about the normal AS GIVEN (kernels/hj_shade.h; never normalised),
//                combined as the shade stage combines a diffuse bounce (kernels/hj_stages.h)
template <bool SPHERE>
HJ_DEV v3 gq_direction(float4 a, float4 b, uint32_t k, uint32_t& rng) {
  rng = rng_seed(__float_as_uint(b.z) + k);
  if (SPHERE) return rand_uniform_sphere(rng);
  const v3 l = rand_cos_hemisphere(rng);
  const v3 n = V(a.w, b.x, b.y);
  const v3 bt = (__builtin_fabsf(n.x) > __builtin_fabsf(n.y)) ? V(0.f, 1.f, 0.f) : V(1.f, 0.f, 0.f);
  const v3 t = normalize3(cross3(n, bt));
  const v3 bb = cross3(n, t);
  return (t * l.x + bb * l.y) + n * l.z;
}

// Top-up from the caller's points: paths for groups [k0, k0 + ngen) of this workgroup's sample sequence, written to the path arrays
// of `parity` behind the n0 continuing paths (positions n0 + sh.n_gen...; the caller guarantees n0 + 64 * ngen <= pool).  A path
// starts at the point as a sample of hj_trace_paths starts at its ray's origin - throughput 1, extinction 0, wasDiscrete, bounce 0,
// kCameraFlag beside the sample index so that the walk gives the first segment tMin = eps - along gq_direction, with the RNG state
// CONTINUED behind the direction's two draws.  The lanes of a group mostly share a point: its two float4 are broadcast loads.
// (A group index is below 2^25 and the last group's samples below 2^31 + 64: no 32-bit wrap.)
template <bool SPHERE>
HJ_DEV void stage_gen_points(const BatchState& st, const DeviceScene& sc, const float4* __restrict__ points, uint32_t spp, uint32_t num_samples,
                             uint32_t g, WgShared& sh, uint32_t parity, uint32_t n0, uint32_t k0, uint32_t ngen, uint32_t waves) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t seg = g * st.pool + n0;
  for (uint32_t k = k0 + wave; k < k0 + ngen; k += waves) {
    const uint32_t s = (g + k * st.num_wg) * 64u + lane;
    const bool valid = s < num_samples;
    const uint32_t qi = lds_push(&sh.n_gen, valid);
    if (valid) {
      const uint32_t i = s / spp, j = s - i * spp;
      const float4 a = points[2 * (size_t)i], b = points[2 * (size_t)i + 1];
      uint32_t rng;
      const v3 d = gq_direction<SPHERE>(a, b, j, rng);
      const uint32_t pos = seg + qi;
      // the sample index rides in origin.w, the RNG state in direction.w
      stp<false>(st.ray_o[parity], pos, make_float4(a.x, a.y, a.z, __uint_as_float(s | kCameraFlag)));
      stp<false>(st.ray_d[parity], pos, make_float4(d.x, d.y, d.z, __uint_as_float(rng)));
      stp<false>(st.thr[parity], pos, make_float4(1.f, 1.f, 1.f, __uint_as_float(1u)));   // wasDiscrete = true, bounce 0
      if (sc.has_extinction) stp<false>(st.ext[parity], pos, make_float4(0.f, 0.f, 0.f, 0.f));
      stp<false>(st.smp_rgb, s, make_float4(0.f, 0.f, 0.f, 1.f));
      stp<false>(st.smp_nd, s, make_float4(0.f, 0.f, 0.f, 0.f));
    }
  }
}

// ... as a CALLED function, like the other stages (kernels/hj_stages.h: own register allocation, the walk stays free of its
// registers).  The point array's address comes in two halves, as the argument segment's does.  ENV only makes the environment
// kernels' instantiation a function of its own.
template <bool ENV, bool SPHERE>
__device__ __attribute__((noinline)) void stage_gen_points_call(uint32_t ka_lo, uint32_t ka_hi, uint32_t pts_lo, uint32_t pts_hi, uint32_t spp,
                                                                 uint32_t num_samples, uint32_t g, uint32_t sh_lds, uint32_t parity, uint32_t n0,
                                                                 uint32_t k0, uint32_t ngen, uint32_t waves) {
  const StageCtx c = stage_ctx(ka_lo, ka_hi, sh_lds);
  const float4* points = (const float4*)(((uint64_t)uni(pts_hi) << 32) | (uint64_t)uni(pts_lo));
  stage_gen_points<SPHERE>(c.st, c.sc, points, uni(spp), uni(num_samples), uni(g), c.sh, uni(parity), uni(n0), uni(k0), uni(ngen), uni(waves));
}

// The whole life of a chunk of samples in ONE launch: the round loop of k_pq_paths (api/path_query.hip; kernels/hj_path_kernel.h's
// loop for explicit records), with the top-up above.  Path regeneration keeps about `pool` paths in flight per workgroup until its
// samples run out.  sh.cam_first stays 0xFFFFFFFF in every round: no path is implicit, so no stage reads st.blocks (null here).
// Exit condition every wave reaches, exactly as in the path kernel: the counts a round's decisions depend on (n_ray, n_gen,
// n_shadow in LDS, groups_left in every thread alike) are read by all waves between two workgroup barriers, so all waves take the
// same branch; the loop ends when there are no rays, no shadow rays and no groups left, and every path ends - a bounce ends it with
// probability >= 1 % from bounce rr_start on, and max_bounces caps it.  A wave that leaves at the one-wave tail leaves for good: the
// counts never grow again once groups_left is 0.
// No global atomic, no inline assembly; ordinary loads and stores (NT = false).  The statistics are per workgroup, summed on the host.
template <bool PAIRS, bool ENV, bool SPHERE>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(HJ_GQ_WAVES, 8))) void k_gq_paths(BatchState st, DeviceScene sc, GatherArgs q) {
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
  const uint32_t g = blockIdx.x;
  // (the called stages read the batch and scene descriptions from this kernel's argument segment and reach `sh` through its LDS address)
  const uint64_t ka_ = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t ka_lo = (uint32_t)ka_, ka_hi = (uint32_t)(ka_ >> 32), sh_lds = (uint32_t)(uintptr_t)(WgSharedLds)&sh;
  const uint32_t pts_lo = (uint32_t)(uintptr_t)q.points, pts_hi = (uint32_t)((uint64_t)(uintptr_t)q.points >> 32);
  uint32_t groups_left = gq_num_groups(q.num_samples, st.num_wg, g);
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
        stage_gen_points_call<ENV, SPHERE>(ka_lo, ka_hi, pts_lo, pts_hi, q.spp, q.num_samples, g, sh_lds, parity, n0, k_next, ngen, waves);
        wg_sync(waves);
        k_next += ngen;
        groups_left -= ngen;
      }
      const uint32_t n = n0 + uni(sh.n_gen), ns = uni(sh.n_shadow);
      // next-event samples of the previous round's shade that the light-shaft grid answered: shadow rays of the statistics all the same
      { const uint32_t nd = uni(sh.n_direct); total_shadow += nd; total_unocc += nd; total_direct += nd; }
      if (n + ns == 0) {
        if (groups_left == 0) break;
        // (not reached with points - every group below the chunk's count holds a sample -, kept as the path kernel has it)
        if (threadIdx.x == 0) { sh.n_ray[parity ^ 1u] = 0; sh.n_direct = 0; }
        wg_sync(waves);
        continue;
      }
      // Tail of the workgroup: one wave can hold every ray of a round and the counts never grow again.
      if (waves > 1u && groups_left == 0 && n + ns <= kGqTail) {
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

// The real spherical-harmonic basis of bands 0..2 at d (not renormalised), in the order and with the constants and operation
// order of include/hijiki_hip.h: 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2
HJ_DEV void gq_sh9(v3 d, float (&Y)[9]) {
  constexpr float c0 = 0x1.20dd76p-2f, c1 = 0x1.f45438p-2f, c2 = 0x1.17b142p+0f, c3 = 0x1.42f602p-2f, c4 = 0x1.17b142p-1f;
  Y[0] = c0;
  Y[1] = c1 * d.y;
  Y[2] = c1 * d.z;
  Y[3] = c1 * d.x;
  Y[4] = c2 * (d.x * d.y);
  Y[5] = c2 * (d.y * d.z);
  Y[6] = c3 * ((3.0f * d.z) * d.z - 1.0f);
  Y[7] = c2 * (d.x * d.z);
  Y[8] = c4 * (d.x * d.x - d.y * d.y);
}

// out: 2 float4 per point, 9 with SH9 - (the float32 sum of the point's spp sample radiances in ascending k, starting from +0;
// (float)spp), (the samples whose first segment hit: first-hit t > 0; the smallest such t or +inf; 0; 0), then with SH9 the 27 sums
// over ascending k of Y_j(d_k) * L_k[c] at word 8 + 3 j + c - one multiply, then one add - and a zero.  d_k: gq_direction<true> again.
template <bool SH9>
__global__ __launch_bounds__(kBlockThreads) void k_gq_resolve(const float4* __restrict__ smp_rgb, const float4* __restrict__ smp_nd,
                                                              const float4* __restrict__ points, uint32_t spp, uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s0 = i * spp;               // (below the chunk's sample count: no wrap)
  float r = 0.f, g = 0.f, b = 0.f, t_min = kInf;
  uint32_t hit = 0;
  float sh[28];
  float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pb = pa;
  if (SH9) {
#pragma unroll
    for (uint32_t j = 0; j < 28u; j++) sh[j] = 0.f;
    pa = points[2 * (size_t)i];
    pb = points[2 * (size_t)i + 1];
  }
  for (uint32_t k = 0; k < spp; k++) {
    const float4 v = smp_rgb[s0 + k];
    const float t = smp_nd[s0 + k].w;
    r += v.x; g += v.y; b += v.z;
    if (t > 0.f) {
      hit++;
      t_min = f_min(t_min, t);
    }
    if (SH9) {
      uint32_t rng;
      float Y[9];
      gq_sh9(gq_direction<true>(pa, pb, k, rng), Y);
#pragma unroll
      for (uint32_t j = 0; j < 9u; j++) {
        sh[3 * j] += Y[j] * v.x;
        sh[3 * j + 1] += Y[j] * v.y;
        sh[3 * j + 2] += Y[j] * v.z;
      }
    }
  }
  const size_t at = (SH9 ? 9 : 2) * (size_t)i;
  out[at] = make_float4(r, g, b, (float)spp);
  out[at + 1] = make_float4((float)hit, t_min, 0.f, 0.f);
  if (SH9) {
#pragma unroll
    for (uint32_t m = 0; m < 7u; m++) out[at + 2 + m] = make_float4(sh[4 * m], sh[4 * m + 1], sh[4 * m + 2], sh[4 * m + 3]);
  }
}

template <bool PAIRS, bool ENV>
static void launch_gq_paths(bool sphere, dim3 grid, dim3 blk, hipStream_t s, const BatchState& st, const DeviceScene& sc, const GatherArgs& q) {
  if (sphere) hipLaunchKernelGGL((k_gq_paths<PAIRS, ENV, true>), grid, blk, 0, s, st, sc, q);
  else hipLaunchKernelGGL((k_gq_paths<PAIRS, ENV, false>), grid, blk, 0, s, st, sc, q);
}

}  // namespace hj

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_paths' order and style).
int hj_trace_irradiance(hj_context* ctx, const float* points, size_t n, uint32_t spp, const hj_render_opts* opts, uint32_t flags, float* out,
                        hj_render_stats* stats) {
  if (n != 0 && (!points || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: null %s", !points ? "points" : "out");
  if (flags & ~(uint32_t)(HJ_GATHER_DEVICE_ARRAYS | HJ_GATHER_SPHERE | HJ_GATHER_SH9))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_GATHER_DEVICE_ARRAYS) != 0, sphere = (flags & HJ_GATHER_SPHERE) != 0, sh9 = (flags & HJ_GATHER_SH9) != 0;
  if (sh9 && !sphere) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: HJ_GATHER_SH9 only together with HJ_GATHER_SPHERE");
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: spp %u outside [1, 65536]", spp);
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: %zu points, at most 2^31 - 1 a call", n);
  if (n != 0 && on_device && ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0)
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: device arrays must be 16-byte aligned");
  hj_render_opts o;
  if (opts) o = *opts;
  else hj_default_render_opts(&o);
  if (o.max_bounces == 0) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: max_bounces must be >= 1");
  if (o.use_bvh == 0)
    return set_error(ctx, HJ_ERR_UNSUPPORTED, "hj_trace_irradiance: the tree is always walked (use_bvh == 0: there is no linear-scan form)");
  if (o.flags & ~(uint32_t)HJ_RENDER_NO_LIGHT_GRID)
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: of the HJ_RENDER_* bits only HJ_RENDER_NO_LIGHT_GRID applies (flags 0x%x)", o.flags);
  if (!sphere && !on_device) {               // (device arrays: the caller's contract)
    for (size_t i = 0; i < n; i++) {
      const float* nm = points + 8 * i + 3;
      if (!std::isfinite(nm[0]) || !std::isfinite(nm[1]) || !std::isfinite(nm[2]) || (nm[0] == 0.f && nm[1] == 0.f && nm[2] == 0.f))
        return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: point %zu has the normal (%g, %g, %g): finite and not all zero is needed", i,
                         (double)nm[0], (double)nm[1], (double)nm[2]);
    }
  }
  if (!ctx) {
    if (hj_device_count() == 0)
      return set_error(nullptr, HJ_ERR_DEVICE, "hj_trace_irradiance: no HIP device available; this library has no CPU fallback");
    return set_error(nullptr, HJ_ERR_INVALID, "hj_trace_irradiance: null context");
  }
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "hj_trace_irradiance: no scene has been uploaded");
  if (n == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const auto wall0 = std::chrono::steady_clock::now();

  // Sizes: hj_trace_paths' (path_query_plan), a point in the place of a ray.  A launch takes whole points.
  const Tuning& tn = ctx->tuning;
  const PathQueryPlan plan = path_query_plan(tn, n, spp);
  const size_t chunk_pts = plan.chunk_rays, most_pts = plan.most_rays;
  const uint32_t G = plan.G;
  const size_t f4 = sizeof(float4), rec = sh9 ? 9 : 2;                  // float4 of an output record
  const hj::DeviceScene sc = scene_for(ctx, o);

  // The path state is hj_trace_paths' (hj_context::paths), and so is the staging of host arrays.
  hj_context::PathQuery& pq = ctx->paths;
  if (const int rc = ensure_path_state(ctx, pq, plan.most_samples, G, (uint32_t)tn.paths_wgs, plan.pool, sc.has_extinction != 0, sc.env_alias != nullptr)) {
    release_path_state(pq);
    return rc;
  }
  hj::BatchState st = pq.st;
  float4 *d_pts = nullptr, *d_out = nullptr;
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, pq.in_rays, most_pts * 2 * f4));
    HJ_TRY(dev_alloc(ctx, pq.out_samples, most_pts * rec * f4));
    d_pts = static_cast<float4*>(pq.in_rays.p);
    d_out = static_cast<float4*>(pq.out_samples.p);
  }
  const size_t launches = (n + chunk_pts - 1) / chunk_pts;
  std::vector<uint32_t> h_acc;
  try {
    if (stats) h_acc.assign(launches * kStatWords * G, 0u);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, HJ_ERR_NOMEM, "hj_trace_irradiance: out of host memory");
  }

  const bool pairs = sc.has_pairs != 0, env = sc.env_alias != nullptr;
  hipError_t e = hipSuccess;
  size_t launch = 0;
  for (size_t at = 0; at < n && e == hipSuccess; at += chunk_pts, launch++) {
    const uint32_t cnt = (uint32_t)std::min(chunk_pts, n - at);
    if (on_device) {
      d_pts = reinterpret_cast<float4*>(const_cast<float*>(points)) + 2 * at;
      d_out = reinterpret_cast<float4*>(out) + rec * at;
    } else {
      e = hipMemcpyAsync(d_pts, points + 8 * at, cnt * 2 * f4, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) break;
    }
    const uint32_t num_samples = cnt * spp;    // (<= 2^31 - 1: HJ_PATHS_CHUNK's upper bound, or one point's spp)
    set_num_wg(st, std::min<uint32_t>(G, (num_samples + 63u) / 64u));
    const hj::GatherArgs q{d_pts, spp, num_samples, o.max_bounces, o.rr_start};
    const dim3 grid(st.num_wg), blk(hj::kBlockThreads);
    if (pairs && env) hj::launch_gq_paths<true, true>(sphere, grid, blk, ctx->stream, st, sc, q);
    else if (pairs) hj::launch_gq_paths<true, false>(sphere, grid, blk, ctx->stream, st, sc, q);
    else if (env) hj::launch_gq_paths<false, true>(sphere, grid, blk, ctx->stream, st, sc, q);
    else hj::launch_gq_paths<false, false>(sphere, grid, blk, ctx->stream, st, sc, q);
    const dim3 rgrid((cnt + hj::kBlockThreads - 1u) / hj::kBlockThreads);
    if (sh9)
      hipLaunchKernelGGL(hj::k_gq_resolve<true>, rgrid, blk, 0, ctx->stream, static_cast<const float4*>(st.smp_rgb),
                         static_cast<const float4*>(st.smp_nd), static_cast<const float4*>(d_pts), spp, cnt, d_out);
    else
      hipLaunchKernelGGL(hj::k_gq_resolve<false>, rgrid, blk, 0, ctx->stream, static_cast<const float4*>(st.smp_rgb),
                         static_cast<const float4*>(st.smp_nd), static_cast<const float4*>(d_pts), spp, cnt, d_out);
    e = hipGetLastError();
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out + 4 * rec * at, d_out, cnt * rec * f4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && stats)
      e = hipMemcpyAsync(h_acc.data() + launch * kStatWords * G, st.acc_closest, sizeof(uint32_t) * kStatWords * st.num_wg, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);      // (also after a failed enqueue: nothing of this call stays in flight)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_error(ctx, HJ_ERR_DEVICE, "hj_trace_irradiance: %s", hipGetErrorString(e));
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    size_t at = 0;
    for (size_t l = 0; l < launches; l++, at += chunk_pts) {
      const size_t cnt = std::min(chunk_pts, n - at);
      add_stat_words(*stats, h_acc.data() + l * kStatWords * G, std::min<size_t>(G, (cnt * spp + 63) / 64));
    }
    stats->paths = (uint64_t)n * spp;
    stats->batches = launches;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  }
  return HJ_OK;
}

}  // extern "C"
