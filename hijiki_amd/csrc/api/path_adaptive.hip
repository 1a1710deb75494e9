// hj_trace_paths_adaptive: path queries whose sample count is decided per ray on the device ("Adaptive path queries").
//
// Sample k of a ray starts from rng_seed(seed + k), so "ray i after d samples" is the same ray with seed_i + d: a later round is a
// compacted ray array with advanced seeds, and it goes through api/path_query.hip's path kernel unchanged (path_query_pass).  This
// unit holds what runs between two rounds and includes hj_num.h only, so the path kernels' machine code does not depend on it:
//   k_pa_accumulate  one thread per ray of a launch: continues the ray's float32 running sums R, G, B, S1, S2 over the launch's
//                    smp_rgb records in ascending k, evaluates the stop rule (pa_stops), writes the active flag and, when the ray
//                    stops, its output record
//   k_pa_count       per workgroup of 256 list entries the number of active ones (wave ballot + popcount)
//   k_pa_scan        ONE workgroup: the counts become exclusive offsets, the total goes to the word the host reads
//   k_pa_scatter     the active entries, in list order, to the next round's index list and ray array (word 6 = seed_i + n_i)
// Ordinary loads and stores, no inline assembly, no global atomic, and no workgroup ever waits for another: the three compaction
// steps are three launches.
// The render-opts check, the context gate and the statistics read-back are the queries' (api/path_query.hip).  The stop rule is
// api/adaptive_stop.h's.  The round loop below (adaptive_query, declared in hj_internal.h) is the driver of both adaptive queries:
// hj_trace_irradiance_adaptive (api/gather_adaptive.hip) enters it with its own pass and accumulate.
#include "hj_internal.h"
#include "../kernels/hj_compact.h"
#include "adaptive_stop.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

constexpr uint32_t kPaThreads = 256u;   // threads of a k_pa_* workgroup = list entries of a compaction workgroup (4 waves)

// One launch of the path kernel has written smp_rgb / smp_nd for cnt rays at c samples each (sample j * c + k).  Entry j of the
// launch is entry j of the round's list behind its first `at` entries (the pointers come offset): ray src[j], or ray first + j in
// round 0, whose list is every ray (src == NULL) and whose sums start from +0.  n_before: the samples every ray of the list has
// already (they all have the same number: a ray that is still active has been in every round).
//   sums[i] = (R, G, B, S1), s2[i] = S2: read unless round 0, written unless the ray stops
//   samples[2 i] = (R, G, B, (float)n_i) when ray i stops; samples[2 i + 1] = first-hit normal and t, in round 0
//   moments[i] (may be NULL) = (S1, S2, sem2, n_i as bits) when ray i stops
__global__ __launch_bounds__(kPaThreads) void k_pa_accumulate(const float4* __restrict__ smp_rgb, const float4* __restrict__ smp_nd, const uint32_t* __restrict__ src,
                                                              uint32_t first, uint32_t cnt, uint32_t c, uint32_t n_before, AdaptiveArgs a,
                                                              float4* __restrict__ sums, float* __restrict__ s2, uint32_t* __restrict__ flags,
                                                              float4* __restrict__ samples, float4* __restrict__ moments) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  const uint32_t i = src ? src[j] : first + j;
  const uint32_t s0 = j * c;                 // (below the launch's sample count: no wrap)
  float R = 0.f, G = 0.f, B = 0.f, S1 = 0.f, S2 = 0.f;
  if (n_before != 0u) {
    const float4 v = sums[i];
    R = v.x; G = v.y; B = v.z; S1 = v.w; S2 = s2[i];
  } else {
    samples[2 * (size_t)i + 1] = smp_nd[s0];
  }
  for (uint32_t k = 0; k < c; k++) {
    const float4 v = smp_rgb[s0 + k];
    R += v.x; G += v.y; B += v.z;
    const float Y = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z;
    S1 += Y;
    S2 += Y * Y;
  }
  const uint32_t m = n_before + c;
  float sem2;
  const bool stop = pa_stops(S1, S2, m, a.spp_max, a.rel_error, a.floor, sem2);
  flags[j] = stop ? 0u : 1u;
  if (stop) {
    samples[2 * (size_t)i] = make_float4(R, G, B, (float)m);
    if (moments) moments[i] = make_float4(S1, S2, sem2, __uint_as_float(m));
  } else {
    sums[i] = make_float4(R, G, B, S1);
    s2[i] = S2;
  }
}

// The compaction is kernels/hj_compact.h's text; here: what is active (flag != 0 of an entry below len) and what an active entry becomes.
__global__ __launch_bounds__(kPaThreads) void k_pa_count(const uint32_t* __restrict__ flags, uint32_t len, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kPaThreads / 64u];
  const uint32_t j = blockIdx.x * kPaThreads + threadIdx.x;
  (void)compact_wave_counts(j < len && flags[j] != 0u, wave_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = compact_tile_count<kPaThreads>(wave_cnt);
}

// (A total is at most the list's length, below 2^31.)
__global__ __launch_bounds__(kPaThreads) void k_pa_scan(uint32_t* __restrict__ counts, uint32_t nb) { compact_scan_tiles<kPaThreads>(counts, nb); }

// Entry j of the list, if active, becomes entry offsets[workgroup] + (active entries of the workgroup before it) of the next list:
// its ray index, and the caller's ray with word 6 = seed + n_after (uint32 wrap-around).  src == NULL: the list is every ray.
__global__ __launch_bounds__(kPaThreads) void k_pa_scatter(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ src, uint32_t len,
                                                           const uint32_t* __restrict__ offsets, const float4* __restrict__ rays, uint32_t n_after,
                                                           uint32_t* __restrict__ src_out, float4* __restrict__ rays_out) {
  __shared__ uint32_t wave_cnt[kPaThreads / 64u];
  const uint32_t j = blockIdx.x * kPaThreads + threadIdx.x;
  const bool active = j < len && flags[j] != 0u;
  const unsigned long long mask = compact_wave_counts(active, wave_cnt);
  if (!active) return;
  HJ_COMPACT_RANK(pos, offsets[blockIdx.x], wave_cnt, mask);
  const uint32_t i = src ? src[j] : j;
  const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
  src_out[pos] = i;
  rays_out[2 * (size_t)pos] = a;
  rays_out[2 * (size_t)pos + 1] = make_float4(b.x, b.y, __uint_as_float(__float_as_uint(b.z) + n_after), b.w);
}

}  // namespace hj

namespace hjapi {

// What both adaptive queries refuse of their adaptive opts, without a device (fn: the entry point's name) -> a
int adaptive_opts_check(hj_context* ctx, const char* fn, const hj_adaptive_opts* aopts, hj_adaptive_opts& a) {
  if (!aopts) return set_error(ctx, HJ_ERR_INVALID, "%s: null adaptive opts", fn);
  a = *aopts;
  if (a.spp_min < 2u) return set_error(ctx, HJ_ERR_INVALID, "%s: spp_min %u below 2 (a variance needs two samples)", fn, a.spp_min);
  if (a.spp_step == 0u) return set_error(ctx, HJ_ERR_INVALID, "%s: spp_step must be >= 1", fn);
  if (a.spp_max < a.spp_min) return set_error(ctx, HJ_ERR_INVALID, "%s: spp_max %u below spp_min %u", fn, a.spp_max, a.spp_min);
  if (a.spp_max > 65536u) return set_error(ctx, HJ_ERR_INVALID, "%s: spp_max %u above 65536", fn, a.spp_max);
  if (!(a.rel_error >= 0.f) || std::isinf(a.rel_error) || !(a.floor >= 0.f) || std::isinf(a.floor))
    return set_error(ctx, HJ_ERR_INVALID, "%s: rel_error %g and floor %g must be finite and >= 0", fn, (double)a.rel_error, (double)a.floor);
  const uint32_t max_rounds = 1u + (a.spp_max - a.spp_min + a.spp_step - 1u) / a.spp_step;
  if (max_rounds > 64u)
    return set_error(ctx, HJ_ERR_INVALID, "%s: %u rounds from spp_min %u to spp_max %u in steps of %u, at most 64", fn, max_rounds, a.spp_min, a.spp_max,
                     a.spp_step);
  return HJ_OK;
}

int adaptive_query(hj_context* ctx, const AdaptiveQuery& q) {
  const size_t n = q.n;
  const hj_adaptive_opts& a = q.a;
  const bool on_device = q.on_device;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const auto wall0 = std::chrono::steady_clock::now();

  // The path state for the largest round there can be: no record stops, and a round has spp_min, spp_step or the last short round's
  // samples per record.  A round lays its launches out as hj_trace_paths lays out a query of its rays and samples (path_query_plan);
  // that layout grows with the number of rays, so a round of fewer records fits into what is allocated here.
  const Tuning& tn = ctx->tuning;
  const uint32_t n32 = (uint32_t)n;
  const uint32_t later = a.spp_max - a.spp_min;
  const uint32_t shapes[3] = {a.spp_min, std::min(a.spp_step, later), later % a.spp_step};
  size_t need_samples = 0;
  PathQueryPlan big{};
  for (const uint32_t c : shapes) {
    if (c == 0) continue;
    const PathQueryPlan p = path_query_plan(tn, n, c);
    need_samples = std::max(need_samples, p.most_samples);
    if ((size_t)p.G * p.pool > (size_t)big.G * big.pool) big = p;
  }
  const hj::DeviceScene sc = scene_for(ctx, q.o);
  hj_context::PathQuery& pq = ctx->paths;
  if (const int rc = ensure_path_state(ctx, pq, need_samples, big.G, (uint32_t)tn.paths_wgs, big.pool, sc.has_extinction != 0, sc.env_alias != nullptr)) {
    release_path_state(pq);
    return rc;
  }
  hj::BatchState st = pq.st;

  // Per record of the call: 20 B of running sums (and the query's own running state), 4 B of flags; with a second round 8 B of index
  // lists and 32 B of rays; a count per 256 records; host arrays are staged whole, once (32 B in, 32 B out, 16 B of moments).
  const size_t f4 = sizeof(float4), u4 = sizeof(uint32_t);
  const uint32_t blocks_most = (n32 + hj::kPaThreads - 1u) / hj::kPaThreads;
  HJ_TRY(dev_alloc(ctx, pq.pa_sums, n * f4));
  HJ_TRY(dev_alloc(ctx, pq.pa_s2, n * sizeof(float)));
  HJ_TRY(dev_alloc(ctx, pq.pa_flags, n * u4));
  if (q.state_bytes != 0) HJ_TRY(dev_alloc(ctx, pq.pa_state, n * q.state_bytes));
  if (later != 0) {
    HJ_TRY(dev_alloc(ctx, pq.pa_src[0], n * u4));
    HJ_TRY(dev_alloc(ctx, pq.pa_src[1], n * u4));
    HJ_TRY(dev_alloc(ctx, pq.pa_rays, n * 2 * f4));
    HJ_TRY(dev_alloc(ctx, pq.pa_counts, ((size_t)blocks_most + 1) * u4));
    HJ_HIP(ctx, pq.pa_active.reserve(1));
  }
  const float4* d_rays = reinterpret_cast<const float4*>(q.in);
  float4 *d_out = reinterpret_cast<float4*>(q.out), *d_mom = reinterpret_cast<float4*>(q.moments);
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, pq.in_rays, n * 2 * f4));
    HJ_TRY(dev_alloc(ctx, pq.out_samples, n * 2 * f4));
    if (q.moments) HJ_TRY(dev_alloc(ctx, pq.pa_moments, n * f4));
    d_rays = static_cast<const float4*>(pq.in_rays.p);
    d_out = static_cast<float4*>(pq.out_samples.p);
    d_mom = q.moments ? static_cast<float4*>(pq.pa_moments.p) : nullptr;
  }
  uint32_t* d_flags = static_cast<uint32_t*>(pq.pa_flags.p);
  uint32_t* d_counts = static_cast<uint32_t*>(pq.pa_counts.p);
  AdaptiveLaunch al{};
  al.spp_max = a.spp_max;
  al.rel_error = a.rel_error;
  al.floor = a.floor;
  al.sums = static_cast<float4*>(pq.pa_sums.p);
  al.s2 = static_cast<float*>(pq.pa_s2.p);
  al.state = q.state_bytes != 0 ? pq.pa_state.p : nullptr;
  al.out = d_out;
  al.moments = d_mom;
  QueryStats acc(q.stats != nullptr);
  hj_render_stats total{};

  hipError_t e = hipSuccess;
  if (!on_device) e = hipMemcpyAsync(pq.in_rays.p, q.in, n * 2 * f4, hipMemcpyHostToDevice, ctx->stream);
  // A round: the path launches over the list's records, chunked as hj_trace_paths chunks, each followed by its accumulate; the
  // compaction of the list; the 4-byte active count; ONE hipStreamSynchronize.  Every record of a list has n_before samples.
  const float4* list_rays = d_rays;          // round 0 reads the caller's records in place
  const uint32_t* list_src = nullptr;        // ... and its list is every record
  uint32_t active = n32, n_before = 0, side = 0;
  while (active != 0 && e == hipSuccess) {
    const uint32_t c = n_before == 0 ? a.spp_min : std::min(a.spp_step, a.spp_max - n_before);
    const uint32_t n_after = n_before + c;
    const PathQueryPlan plan = path_query_plan(tn, active, c);
    st.pool = plan.pool;
    const size_t launches = (active + plan.chunk_rays - 1) / plan.chunk_rays;
    HJ_TRY(acc.reserve(ctx, q.name, launches, plan.G));
    size_t launch = 0;
    for (size_t at = 0; at < active && e == hipSuccess; at += plan.chunk_rays, launch++) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(plan.chunk_rays, active - at);
      q.pass(q, st, sc, plan.G, list_rays + 2 * at, cnt, c, ctx->stream);
      al.src = list_src ? list_src + at : nullptr;
      al.first = (uint32_t)at;
      al.cnt = cnt;
      al.c = c;
      al.n_before = n_before;
      al.flags = d_flags + at;
      q.accumulate(q, st, al, ctx->stream);
      e = hipGetLastError();
      if (e == hipSuccess) e = acc.enqueue(launch, st, ctx->stream);
    }
    const bool last = n_after == a.spp_max;  // every record of the list stops: nothing to compact, the count is 0
    if (e == hipSuccess && !last) {
      const uint32_t nb = (active + hj::kPaThreads - 1u) / hj::kPaThreads;
      uint32_t* next_src = static_cast<uint32_t*>(pq.pa_src[side].p);
      hipLaunchKernelGGL(hj::k_pa_count, dim3(nb), dim3(hj::kPaThreads), 0, ctx->stream, d_flags, active, d_counts);
      hipLaunchKernelGGL(hj::k_pa_scan, dim3(1), dim3(hj::kPaThreads), 0, ctx->stream, d_counts, nb);
      hipLaunchKernelGGL(hj::k_pa_scatter, dim3(nb), dim3(hj::kPaThreads), 0, ctx->stream, d_flags, list_src, active, d_counts, d_rays, n_after, next_src,
                         static_cast<float4*>(pq.pa_rays.p));
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(pq.pa_active.p, d_counts + nb, u4, hipMemcpyDeviceToHost, ctx->stream);
      list_src = next_src;
      list_rays = static_cast<const float4*>(pq.pa_rays.p);
      side ^= 1u;
    }
    if (e == hipSuccess && last && !on_device) {      // the results of host arrays ride on the last possible round's synchronisation
      e = hipMemcpyAsync(q.out, d_out, n * 2 * f4, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess && q.moments) e = hipMemcpyAsync(q.moments, d_mom, n * f4, hipMemcpyDeviceToHost, ctx->stream);
    }
    HJ_TRY(drain(ctx, q.name, e));                                // (the round's ONE synchronisation)
    acc.add(total, plan.chunk_rays, active, c);
    total.paths += (uint64_t)active * c;
    total.batches += launches;
    total.bounce_rounds += 1;
    const uint32_t next = last ? 0u : *pq.pa_active.p;
    if (next > active) return set_error(ctx, HJ_ERR_DEVICE, "%s: %u active %s out of a list of %u", q.name, next, q.what, active);
    if (next == 0 && !last && !on_device) {           // the list ran out before spp_max: one more, synchronous, copy back
      e = hipMemcpy(q.out, d_out, n * 2 * f4, hipMemcpyDeviceToHost);
      if (e == hipSuccess && q.moments) e = hipMemcpy(q.moments, d_mom, n * f4, hipMemcpyDeviceToHost);
    }
    active = next;
    n_before = n_after;
  }
  if (e != hipSuccess) return drain(ctx, q.name, e);            // (the copy in, or the synchronous copy back)
  if (q.stats) {
    total.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    *q.stats = total;
  }
  return HJ_OK;
}

}  // namespace hjapi

// the path launch of one chunk of a round, and its accumulate (AdaptiveQuery::pass / ::accumulate)
static void paths_pass(const AdaptiveQuery& q, hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_rays, uint32_t cnt, uint32_t c,
                       hipStream_t s) {
  path_query_pass(st, sc, G, d_rays, cnt, c, q.o, s);
}

static void paths_accumulate(const AdaptiveQuery&, const hj::BatchState& st, const AdaptiveLaunch& l, hipStream_t s) {
  const hj::AdaptiveArgs args{l.spp_max, l.rel_error, l.floor};
  hipLaunchKernelGGL(hj::k_pa_accumulate, dim3((l.cnt + hj::kPaThreads - 1u) / hj::kPaThreads), dim3(hj::kPaThreads), 0, s,
                     static_cast<const float4*>(st.smp_rgb), static_cast<const float4*>(st.smp_nd), l.src, l.first, l.cnt, l.c, l.n_before, args, l.sums, l.s2,
                     l.flags, l.out, l.moments);
}

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_paths' order and style).  Sizes, path
// state, lists, staging, the ONE hipStreamSynchronize per round and the statistics are adaptive_query's.
int hj_trace_paths_adaptive(hj_context* ctx, const float* rays, size_t n, const hj_adaptive_opts* aopts, const hj_render_opts* opts, uint32_t flags,
                            float* samples, float* moments, hj_render_stats* stats) {
  if (n != 0 && (!rays || !samples)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths_adaptive: null %s", !rays ? "rays" : "samples");
  if (flags & ~(uint32_t)HJ_PATHS_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths_adaptive: unknown flag bits 0x%x", flags);
  const bool on_device = (flags & HJ_PATHS_DEVICE_ARRAYS) != 0;
  AdaptiveQuery q{__func__, "rays", rays, n, {}, on_device, samples, moments, stats, {}, paths_pass, paths_accumulate, flags, 0};
  HJ_TRY(adaptive_opts_check(ctx, __func__, aopts, q.a));
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths_adaptive: %zu rays, at most 2^31 - 1 a call", n);
  if (n != 0 && on_device &&
      misaligned(rays, samples, moments))
    return set_error(ctx, HJ_ERR_INVALID, "hj_trace_paths_adaptive: device arrays must be 16-byte aligned");
  HJ_TRY(query_render_opts(ctx, __func__, opts, q.o));
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  return adaptive_query(ctx, q);
}

}  // extern "C"

