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
// The round loop of k_gq_paths is k_pq_paths' (api/path_query.hip): ONE text, api/query_round_loop.h, included into both kernel
// bodies with the top-up named by a macro.  The host half behind the entry point's checks is fixed_spp_query (api/path_query.hip).
#include "hj_internal.h"
#include <type_traits>
#include "../kernels/hj_stages.h"
#include "../kernels/hj_sh9.h"
#include "query_round.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

// What the kernel's argument segment holds behind (BatchState, DeviceScene).  A sample is s = point * spp + k, k < spp; the chunk's
// samples are [0, num_samples), num_samples <= 2^31 - 1 (the sample index shares its word with kCameraFlag).
struct GatherArgs {
  const float4* src;      // two float4 per point: position.xyz, normal.x | normal.yz, seed bits, reserved
  uint32_t spp;
  uint32_t num_samples;
  uint32_t max_bounces;
  uint32_t rr_start;
  uint32_t start;         // the flags word a path starts with: 1u (wasDiscrete, bounce 0), or 0u with HJ_GATHER_INDIRECT
};

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
// start: GatherArgs' - with HJ_GATHER_INDIRECT wasDiscrete is clear, so the first segment's emission (an emitter it ends on, the
// environment it leaves into) is not counted; nothing else of a path differs.
// (A group index is below 2^25 and the last group's samples below 2^31 + 64: no 32-bit wrap.)
template <bool SPHERE>
HJ_DEV void stage_gen_points(const BatchState& st, const DeviceScene& sc, const float4* __restrict__ points, uint32_t spp, uint32_t num_samples,
                             uint32_t g, WgShared& sh, uint32_t parity, uint32_t n0, uint32_t k0, uint32_t ngen, uint32_t waves, uint32_t start) {
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
      stp<false>(st.thr[parity], pos, make_float4(1.f, 1.f, 1.f, __uint_as_float(start)));   // wasDiscrete = true (indirect: false), bounce 0
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
                                                                 uint32_t k0, uint32_t ngen, uint32_t waves, uint32_t start) {
  const StageCtx c = stage_ctx(ka_lo, ka_hi, sh_lds);
  const float4* points = (const float4*)(((uint64_t)uni(pts_hi) << 32) | (uint64_t)uni(pts_lo));
  stage_gen_points<SPHERE>(c.st, c.sc, points, uni(spp), uni(num_samples), uni(g), c.sh, uni(parity), uni(n0), uni(k0), uni(ngen), uni(waves), uni(start));
}

// One persistent launch per chunk of samples: the round loop of api/query_round_loop.h with the top-up above.
template <bool PAIRS, bool ENV, bool SPHERE>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(HJ_QUERY_WAVES, 8))) void k_gq_paths(BatchState st, DeviceScene sc, GatherArgs q) {
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
#define HJ_QUERY_TOP_UP(...) stage_gen_points_call<ENV, SPHERE>(__VA_ARGS__, q.start)   // (the start word: wave-uniform, from the argument segment)
#include "query_round_loop.h"
#undef HJ_QUERY_TOP_UP
}

// out: 2 float4 per point, 9 with SH9 - (the float32 sum of the point's spp sample radiances in ascending k, starting from +0;
// (float)spp), (the samples whose first segment hit: first-hit t > 0; the smallest such t or +inf; 0; 0), then with SH9 the 27 sums
// over ascending k of Y_j(d_k) * L_k[c] at word 8 + 3 j + c - one multiply, then one add - and a zero.  d_k: gq_direction<true> again;
// Y_j: kernels/hj_sh9.h's basis, which the probe look-up shares.
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
      sh9_basis(gq_direction<true>(pa, pb, k, rng), Y);
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

namespace hjapi {

// the path launch of one chunk: path_query_pass's launch shape, a point in the place of a ray (declared in hj_internal.h)
void gather_query_pass(hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_pts, uint32_t cnt, uint32_t spp, const hj_render_opts& o,
                       uint32_t flags, hipStream_t s) {
  const bool sphere = (flags & HJ_GATHER_SPHERE) != 0;
  const bool pairs = sc.has_pairs != 0, env = sc.env_alias != nullptr;
  const uint32_t num_samples = cnt * spp;                  // (<= 2^31 - 1: HJ_PATHS_CHUNK's upper bound, or one point's spp)
  set_num_wg(st, std::min<uint32_t>(G, (num_samples + 63u) / 64u));
  const hj::GatherArgs q{d_pts, spp, num_samples, o.max_bounces, o.rr_start, (flags & HJ_GATHER_INDIRECT) != 0 ? 0u : 1u};
  const dim3 grid(st.num_wg), blk(hj::kBlockThreads);
  if (pairs && env) hj::launch_gq_paths<true, true>(sphere, grid, blk, s, st, sc, q);
  else if (pairs) hj::launch_gq_paths<true, false>(sphere, grid, blk, s, st, sc, q);
  else if (env) hj::launch_gq_paths<false, true>(sphere, grid, blk, s, st, sc, q);
  else hj::launch_gq_paths<false, false>(sphere, grid, blk, s, st, sc, q);
}

// hemisphere mode, host arrays: every normal finite and not all zero, before anything is written
int gather_normals_check(hj_context* ctx, const char* fn, const float* points, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const float* nm = points + 8 * i + 3;
    if (!std::isfinite(nm[0]) || !std::isfinite(nm[1]) || !std::isfinite(nm[2]) || (nm[0] == 0.f && nm[1] == 0.f && nm[2] == 0.f))
      return set_error(ctx, HJ_ERR_INVALID, "%s: point %zu has the normal (%g, %g, %g): finite and not all zero is needed", fn, i, (double)nm[0],
                       (double)nm[1], (double)nm[2]);
  }
  return HJ_OK;
}

}  // namespace hjapi

// the path launch and the resolve of one chunk (FixedSppQuery::chunk)
static void gather_chunk(const FixedSppQuery& fq, hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_pts, uint32_t cnt,
                         float4* d_out, hipStream_t s) {
  const bool sh9 = (fq.flags & HJ_GATHER_SH9) != 0;
  const uint32_t spp = fq.spp;
  gather_query_pass(st, sc, G, d_pts, cnt, spp, fq.o, fq.flags, s);
  const dim3 blk(hj::kBlockThreads);
  const dim3 rgrid = per_lane(cnt);
  if (sh9)
    hipLaunchKernelGGL(hj::k_gq_resolve<true>, rgrid, blk, 0, s, static_cast<const float4*>(st.smp_rgb), static_cast<const float4*>(st.smp_nd),
                       d_pts, spp, cnt, d_out);
  else
    hipLaunchKernelGGL(hj::k_gq_resolve<false>, rgrid, blk, 0, s, static_cast<const float4*>(st.smp_rgb), static_cast<const float4*>(st.smp_nd),
                       d_pts, spp, cnt, d_out);
}

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_paths' order and style).  Sizes, path
// state, staging, chunking by whole points, the ONE hipStreamSynchronize and the statistics are fixed_spp_query's (api/path_query.hip).
int hj_trace_irradiance(hj_context* ctx, const float* points, size_t n, uint32_t spp, const hj_render_opts* opts, uint32_t flags, float* out,
                        hj_render_stats* stats) {
  if (n != 0 && (!points || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: null %s", !points ? "points" : "out");
  if (flags & ~(uint32_t)(HJ_GATHER_DEVICE_ARRAYS | HJ_GATHER_SPHERE | HJ_GATHER_SH9 | HJ_GATHER_INDIRECT))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_GATHER_DEVICE_ARRAYS) != 0, sphere = (flags & HJ_GATHER_SPHERE) != 0, sh9 = (flags & HJ_GATHER_SH9) != 0;
  if (sh9 && !sphere) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: HJ_GATHER_SH9 only together with HJ_GATHER_SPHERE");
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: spp %u outside [1, 65536]", spp);
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: %zu points, at most 2^31 - 1 a call", n);
  if (n != 0 && on_device && misaligned(points, out))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance: device arrays must be 16-byte aligned");
  FixedSppQuery q{__func__, points, n, spp, sh9 ? 9u : 2u, on_device, out, stats, {}, gather_chunk, flags};
  HJ_TRY(query_render_opts(ctx, __func__, opts, q.o));
  if (!sphere && !on_device) HJ_TRY(gather_normals_check(ctx, __func__, points, n));   // (device arrays: the caller's contract)
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  return fixed_spp_query(ctx, q);
}

}  // extern "C"
