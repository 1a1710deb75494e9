// hj_trace_irradiance_adaptive: gather queries whose sample count is decided per point on the device, and the scatter of
// hj_bake_lightmap_adaptive ("Adaptive gather and bake").
//
// A gather point is two float4 with the seed in word 6, as a ray is, and sample k of a point starts from rng_seed(seed + k): "point i
// after d samples" is the same point with seed_i + d.  So the rounds, the lists and their compaction are hj_trace_paths_adaptive's -
// adaptive_query and the k_pa_count / k_pa_scan / k_pa_scatter kernels of api/path_adaptive.hip, entered with this unit's pass and
// accumulate -, and a later round goes through k_gq_paths unchanged (gather_query_pass, api/gather_query.hip).  This unit includes
// hj_num.h and api/adaptive_stop.h only, so the path kernels' machine code does not depend on it:
//   k_ga_accumulate  one thread per point of a launch: k_pa_accumulate's running sums R, G, B, S1, S2 over the launch's smp_rgb
//                    records in ascending k, beside them the number of first segments that hit and the nearest such hit
//                    (smp_nd.w); the stop rule (pa_stops); the active flag; when the point stops, its record
//   k_ga_scatter     one thread per gather record of a bake: the sums scaled by 3.14159274f / (float)n_i to the texel word 7 of its
//                    point names, n_i to the sample map
// Ordinary loads and stores, no inline assembly, no global atomic.
#include "hj_internal.h"
#include "adaptive_stop.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

constexpr uint32_t kGaThreads = 256u;   // threads of a k_ga_* workgroup (4 waves)

// One launch of the gather's path kernel has written smp_rgb / smp_nd for cnt points at c samples each (sample j * c + k).  The
// launch's entries, src, first, n_before, sums, s2, flags and moments are k_pa_accumulate's (api/path_adaptive.hip).
//   state[i] = (hits as uint32 bits, the smallest first-hit t or +inf): read unless round 0, written unless the point stops
//   out[2 i] = (R, G, B, (float)n_i), out[2 i + 1] = ((float)hits, nearest hit, 0, 0) when point i stops - k_gq_resolve's record
__global__ __launch_bounds__(kGaThreads) void k_ga_accumulate(const float4* __restrict__ smp_rgb, const float4* __restrict__ smp_nd, const uint32_t* __restrict__ src,
                                                              uint32_t first, uint32_t cnt, uint32_t c, uint32_t n_before, AdaptiveArgs a,
                                                              float4* __restrict__ sums, float* __restrict__ s2, float2* __restrict__ state,
                                                              uint32_t* __restrict__ flags, float4* __restrict__ out, float4* __restrict__ moments) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  const uint32_t i = src ? src[j] : first + j;
  const uint32_t s0 = j * c;                 // (below the launch's sample count: no wrap)
  float R = 0.f, G = 0.f, B = 0.f, S1 = 0.f, S2 = 0.f, t_min = kInf;
  uint32_t hit = 0;
  if (n_before != 0u) {
    const float4 v = sums[i];
    const float2 h = state[i];
    R = v.x; G = v.y; B = v.z; S1 = v.w; S2 = s2[i];
    hit = __float_as_uint(h.x);
    t_min = h.y;
  }
  for (uint32_t k = 0; k < c; k++) {
    const float4 v = smp_rgb[s0 + k];
    const float t = smp_nd[s0 + k].w;
    R += v.x; G += v.y; B += v.z;
    const float Y = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z;
    S1 += Y;
    S2 += Y * Y;
    if (t > 0.f) {
      hit++;
      t_min = f_min(t_min, t);
    }
  }
  const uint32_t m = n_before + c;
  float sem2;
  const bool stop = pa_stops(S1, S2, m, a.spp_max, a.rel_error, a.floor, sem2);
  flags[j] = stop ? 0u : 1u;
  if (stop) {
    out[2 * (size_t)i] = make_float4(R, G, B, (float)m);
    out[2 * (size_t)i + 1] = make_float4((float)hit, t_min, 0.f, 0.f);
    if (moments) moments[i] = make_float4(S1, S2, sem2, __uint_as_float(m));
  } else {
    sums[i] = make_float4(R, G, B, S1);
    s2[i] = S2;
    state[i] = make_float2(__uint_as_float(hit), t_min);
  }
}

// One thread per gather record i: texel = word 7 of point i (below the atlas' texels: the bake's own points); the image and the
// sample map hold zeros before.  Word 3 of a record is (float)n_i, exact (n_i <= 65536); the division is correctly rounded.
__global__ __launch_bounds__(kGaThreads) void k_ga_scatter(const float4* __restrict__ points, const float4* __restrict__ records, uint32_t n,
                                                           float4* __restrict__ image, uint32_t* __restrict__ sample_map) {
  const uint32_t i = blockIdx.x * kGaThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = __float_as_uint(points[2 * (size_t)i + 1].w);
  const float4 r = records[2 * (size_t)i];
  const float scale = 3.14159274f / r.w;
  image[t] = make_float4(r.x * scale, r.y * scale, r.z * scale, 1.0f);
  if (sample_map) sample_map[t] = (uint32_t)r.w;
}

}  // namespace hj

namespace hjapi {

void lightmap_scatter_adaptive(const float4* d_points, const float4* d_records, uint32_t n, float4* d_image, uint32_t* d_sample_map, hipStream_t s) {
  hipLaunchKernelGGL(hj::k_ga_scatter, dim3((n + hj::kGaThreads - 1u) / hj::kGaThreads), dim3(hj::kGaThreads), 0, s, d_points, d_records, n, d_image,
                     d_sample_map);
}

}  // namespace hjapi

// the path launch of one chunk of a round, and its accumulate (AdaptiveQuery::pass / ::accumulate)
static void gather_pass(const AdaptiveQuery& q, hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_pts, uint32_t cnt, uint32_t c,
                        hipStream_t s) {
  gather_query_pass(st, sc, G, d_pts, cnt, c, q.o, q.flags, s);
}

static void gather_accumulate(const AdaptiveQuery&, const hj::BatchState& st, const AdaptiveLaunch& l, hipStream_t s) {
  const hj::AdaptiveArgs args{l.spp_max, l.rel_error, l.floor};
  hipLaunchKernelGGL(hj::k_ga_accumulate, dim3((l.cnt + hj::kGaThreads - 1u) / hj::kGaThreads), dim3(hj::kGaThreads), 0, s,
                     static_cast<const float4*>(st.smp_rgb), static_cast<const float4*>(st.smp_nd), l.src, l.first, l.cnt, l.c, l.n_before, args, l.sums, l.s2,
                     static_cast<float2*>(l.state), l.flags, l.out, l.moments);
}

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_irradiance's order, the adaptive opts
// where hj_trace_paths_adaptive has them).  Everything behind them is adaptive_query's (api/path_adaptive.hip).
int hj_trace_irradiance_adaptive(hj_context* ctx, const float* points, size_t n, const hj_adaptive_opts* aopts, const hj_render_opts* opts, uint32_t flags,
                                 float* out, float* moments, hj_render_stats* stats) {
  if (n != 0 && (!points || !out)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance_adaptive: null %s", !points ? "points" : "out");
  if (flags & ~(uint32_t)(HJ_GATHER_DEVICE_ARRAYS | HJ_GATHER_SPHERE | HJ_GATHER_SH9 | HJ_GATHER_INDIRECT))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance_adaptive: unknown flag bits 0x%x", flags);
  if (flags & HJ_GATHER_SH9) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance_adaptive: HJ_GATHER_SH9 is not available in the adaptive gather");
  const bool on_device = (flags & HJ_GATHER_DEVICE_ARRAYS) != 0, sphere = (flags & HJ_GATHER_SPHERE) != 0;
  AdaptiveQuery q{__func__, "points", points, n, {}, on_device, out, moments, stats, {}, gather_pass, gather_accumulate, flags, sizeof(float2)};
  HJ_TRY(adaptive_opts_check(ctx, __func__, aopts, q.a));
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance_adaptive: %zu points, at most 2^31 - 1 a call", n);
  if (n != 0 && on_device &&
      misaligned(points, out, moments))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_irradiance_adaptive: device arrays must be 16-byte aligned");
  HJ_TRY(query_render_opts(ctx, __func__, opts, q.o));
  if (!sphere && !on_device) HJ_TRY(gather_normals_check(ctx, __func__, points, n));   // (device arrays: the caller's contract)
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  return adaptive_query(ctx, q);
}

}  // extern "C"
