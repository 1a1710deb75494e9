// hj_probe_points, hj_bake_probes, hj_sample_probes: a regular grid of irradiance probes baked from the uploaded scene, and the
// look-up of a baked volume at caller-given points ("Probe volumes").
//
// The look-up kernel is kernels/hj_probes.h's (beside it hj_sh9.h and hj_num.h alone, so the path kernels' machine code does not
// depend on this unit).  The gather of the bake is hj_trace_irradiance itself, called with device arrays as api/lightmap.hip calls
// it: nothing of its plan or its round loop is restated here.
//   points:  k_pv_points
//   bake:    k_pv_points  ->  hj_trace_irradiance (sphere, SH9; it returns with its records complete)  ->  k_pv_resolve
//   sample:  k_pv_sample
//   k_pv_points   one thread per probe of a window: its gather point
//   k_pv_resolve  one thread per probe: the gather's 27 SH sums scaled to irradiance coefficients, and the validity weight
// For api/probe_update.hip: probe_desc_check and probe_points_enqueue (hj_internal.h).
#include "hj_internal.h"
#include "../kernels/hj_probes.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

// Probe p = first + i of thread i, p = (z * count[1] + y) * count[0] + x: position origin + (float)i * spacing per axis (a product, then a
// sum), normal +0, the seed seed + p * seed_stride (uint32 wrap-around), p.  points: the n records of the window first ... first + n - 1.
__global__ __launch_bounds__(kPvThreads) void k_pv_points(PvGrid g, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t n, float4* __restrict__ points) {
  const uint32_t i = blockIdx.x * kPvThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = first + i;
  const uint32_t x = p % g.count[0], yz = p / g.count[0], y = yz % g.count[1], z = yz / g.count[1];
  const float px = g.origin[0] + (float)x * g.spacing[0], py = g.origin[1] + (float)y * g.spacing[1], pz = g.origin[2] + (float)z * g.spacing[2];
  points[2 * (size_t)i] = make_float4(px, py, pz, 0.0f);
  points[2 * (size_t)i + 1] = make_float4(0.0f, 0.0f, __uint_as_float(seed + p * seed_stride), __uint_as_float(p));
}

// records: 9 float4 per probe, hj_trace_irradiance's with HJ_GATHER_SH9; the arithmetic is pv_resolve_record's (kernels/hj_probes.h).
__global__ __launch_bounds__(kPvThreads) void k_pv_resolve(const float4* __restrict__ records, uint32_t n, float s, float min_distance, float4* __restrict__ probes) {
  const uint32_t p = blockIdx.x * kPvThreads + threadIdx.x;
  if (p >= n) return;
  float v[28];
  pv_resolve_record(records + 9 * (size_t)p, s, min_distance, v);
#pragma unroll
  for (uint32_t m = 0; m < kPvVec; m++) probes[kPvVec * (size_t)p + m] = make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
}

}  // namespace hj

namespace {

// What the three entry points refuse of a desc, without a device (fn: the entry point's name) -> g, n = the probes
int check_desc(hj_context* ctx, const char* fn, const hj_probe_desc* d, hj::PvGrid& g, uint32_t& n) {
  // (HJ_PROBES_INDIRECT_ONLY: read by the calls that gather - probe_gather_flags -, accepted and ignored by every other reader of a desc)
  if (d->flags & ~(uint32_t)(HJ_PROBES_DEVICE_ARRAYS | HJ_PROBES_INDIRECT_ONLY)) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown flag bits 0x%x", fn, d->flags);
  uint64_t total = 1;
  for (int a = 0; a < 3; a++) {
    if (d->count[a] == 0 || d->count[a] > 1024u) total = ~0ull;
    else if (total != ~0ull) total *= d->count[a];
  }
  if (total > (1ull << 22))
    return set_error(ctx, HJ_ERR_INVALID, "%s: count %u x %u x %u: 1 ... 1024 each and at most 2^22 probes", fn, d->count[0], d->count[1], d->count[2]);
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(d->origin[a])) return set_error(ctx, HJ_ERR_INVALID, "%s: origin[%d] %g is not finite", fn, a, (double)d->origin[a]);
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(d->spacing[a]) || !(d->spacing[a] > 0.0f))
      return set_error(ctx, HJ_ERR_INVALID, "%s: spacing[%d] %g: finite and > 0 is needed", fn, a, (double)d->spacing[a]);
  if (!std::isfinite(d->min_distance) || d->min_distance < 0.0f)
    return set_error(ctx, HJ_ERR_INVALID, "%s: min_distance %g: finite and >= 0 is needed", fn, (double)d->min_distance);
  for (int a = 0; a < 3; a++) {
    g.origin[a] = d->origin[a];
    g.spacing[a] = d->spacing[a];
    g.count[a] = d->count[a];
  }
  n = (uint32_t)total;
  return HJ_OK;
}

dim3 per_probe(uint32_t n) { return dim3((n + hj::kPvThreads - 1u) / hj::kPvThreads); }

// the gather points of the probes first ... first + n - 1 (n > 0) under `seed`, on the context's stream
void enqueue_points(hj_context* ctx, const hj::PvGrid& g, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t n, float4* d_points) {
  hipLaunchKernelGGL(hj::k_pv_points, per_probe(n), dim3(hj::kPvThreads), 0, ctx->stream, g, seed, seed_stride, first, n, d_points);
}

}  // namespace

namespace hjapi {
uint32_t probe_gather_flags(const hj_probe_desc* d) {
  return HJ_GATHER_SPHERE | HJ_GATHER_SH9 | HJ_GATHER_DEVICE_ARRAYS | ((d->flags & HJ_PROBES_INDIRECT_ONLY) != 0 ? (uint32_t)HJ_GATHER_INDIRECT : 0u);
}
int probe_desc_check(hj_context* ctx, const char* fn, const hj_probe_desc* d, hj::PvGrid& g, uint32_t& n) { return check_desc(ctx, fn, d, g, n); }
void probe_points_enqueue(hj_context* ctx, const hj::PvGrid& g, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t n, float4* d_points) {
  enqueue_points(ctx, g, seed, seed_stride, first, n, d_points);
}
// k_pv_sample over m (> 0) device points: enough workgroups to fill the device, no more than the points need; the kernel strides over the rest
void probe_sample_enqueue(hj_context* ctx, const hj::PvGrid& g, const float4* d_probes, const float4* d_points, uint32_t m, float4* d_out) {
  const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)m + hj::kPvThreads - 1u) / hj::kPvThreads, (size_t)ctx->num_cus * 8u);
  hipLaunchKernelGGL(hj::k_pv_sample, dim3(blocks), dim3(hj::kPvThreads), 0, ctx->stream, g, d_probes, d_points, m, d_out);
}
}  // namespace hjapi

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_lightmap_texels' order and style).
int hj_probe_points(hj_context* ctx, const hj_probe_desc* desc, float* points) {
  if (!desc || !points) return set_error(ctx, HJ_ERR_INVALID, "hj_probe_points: null %s", !desc ? "desc" : "points");
  hj::PvGrid g{};
  uint32_t n = 0;
  HJ_TRY(check_desc(ctx, __func__, desc, g, n));
  const bool on_device = (desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(points)) return set_error(ctx, HJ_ERR_INVALID, "hj_probe_points: device arrays must be 16-byte aligned");
  HJ_TRY(context_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  float4* d_points = reinterpret_cast<float4*>(points);
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, ctx->probes.points, sizeof(float4) * 2 * (size_t)n));
    d_points = static_cast<float4*>(ctx->probes.points.p);
  }
  enqueue_points(ctx, g, desc->seed, desc->seed_stride, 0u, n, d_points);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(points, d_points, sizeof(float4) * 2 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  return drain(ctx, __func__, e);
}

int hj_bake_probes(hj_context* ctx, const hj_probe_desc* desc, uint32_t spp, const hj_render_opts* opts, float* probes, hj_render_stats* stats) {
  if (!desc || !probes) return set_error(ctx, HJ_ERR_INVALID, "hj_bake_probes: null %s", !desc ? "desc" : "probes");
  hj::PvGrid g{};
  uint32_t n = 0;
  HJ_TRY(check_desc(ctx, __func__, desc, g, n));
  const bool on_device = (desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0;
  if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "hj_bake_probes: spp %u outside [1, 65536]", spp);
  if (on_device && misaligned(probes)) return set_error(ctx, HJ_ERR_INVALID, "hj_bake_probes: device arrays must be 16-byte aligned");
  hj_render_opts o;
  HJ_TRY(query_render_opts(ctx, __func__, opts, o));
  HJ_TRY(query_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::Probes& pv = ctx->probes;
  // 1. the points, 2. the gather: the same stream, so it runs behind the points; it returns with its records complete
  HJ_TRY(dev_alloc(ctx, pv.points, sizeof(float4) * 2 * (size_t)n));
  HJ_TRY(dev_alloc(ctx, pv.records, sizeof(float4) * 9 * (size_t)n));
  float4* d_probes = reinterpret_cast<float4*>(probes);
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, pv.volume, sizeof(float4) * hj::kPvVec * (size_t)n));
    d_probes = static_cast<float4*>(pv.volume.p);
  }
  float4 *d_points = static_cast<float4*>(pv.points.p), *d_records = static_cast<float4*>(pv.records.p);
  enqueue_points(ctx, g, desc->seed, desc->seed_stride, 0u, n, d_points);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, __func__, e);
  HJ_TRY(hj_trace_irradiance(ctx, reinterpret_cast<const float*>(d_points), n, spp, &o, probe_gather_flags(desc),
                             reinterpret_cast<float*>(d_records), stats));
  // 3. the resolve
  const float s = 12.5663706f / (float)spp;
  hipLaunchKernelGGL(hj::k_pv_resolve, per_probe(n), dim3(hj::kPvThreads), 0, ctx->stream, static_cast<const float4*>(d_records), n, s, desc->min_distance, d_probes);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(probes, d_probes, sizeof(float4) * hj::kPvVec * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  return drain(ctx, __func__, e);
}

int hj_sample_probes(hj_context* ctx, const hj_probe_desc* desc, const float* probes, const float* points, size_t n, float* out) {
  if (!desc || (n != 0 && (!probes || !points || !out)))
    return set_error(ctx, HJ_ERR_INVALID, "hj_sample_probes: null %s", !desc ? "desc" : !probes ? "probes" : !points ? "points" : "out");
  hj::PvGrid g{};
  uint32_t np = 0;
  HJ_TRY(check_desc(ctx, __func__, desc, g, np));
  const bool on_device = (desc->flags & HJ_PROBES_DEVICE_ARRAYS) != 0;
  if (on_device && n != 0 && misaligned(probes, points, out))
    return set_error(ctx, HJ_ERR_INVALID, "hj_sample_probes: device arrays must be 16-byte aligned");
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_sample_probes: %zu points, at most 2^31 - 1 a call", n);
  if (!on_device) {                            // (device arrays: the caller's contract; the kernel clamps whatever it is given)
    for (size_t i = 0; i < n; i++) {
      const float* p = points + 8 * i;
      for (int k = 0; k < 6; k++)
        if (!std::isfinite(p[k])) return set_error(ctx, HJ_ERR_INVALID, "hj_sample_probes: point %zu has a non-finite %s", i, k < 3 ? "position" : "normal");
      if (p[3] == 0.f && p[4] == 0.f && p[5] == 0.f) return set_error(ctx, HJ_ERR_INVALID, "hj_sample_probes: point %zu has an all-zero normal", i);
    }
  }
  HJ_TRY(context_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const float4 *d_probes = reinterpret_cast<const float4*>(probes), *d_points = reinterpret_cast<const float4*>(points);
  float4* d_out = reinterpret_cast<float4*>(out);
  if (!on_device) {
    hj_context::Probes& pv = ctx->probes;
    HJ_TRY(dev_alloc(ctx, pv.volume, sizeof(float4) * hj::kPvVec * (size_t)np));
    HJ_TRY(dev_alloc(ctx, pv.in_points, sizeof(float4) * 2 * n));
    HJ_TRY(dev_alloc(ctx, pv.out, sizeof(float4) * n));
    hipError_t e = hipMemcpyAsync(pv.volume.p, probes, sizeof(float4) * hj::kPvVec * (size_t)np, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(pv.in_points.p, points, sizeof(float4) * 2 * n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return drain(ctx, __func__, e);
    d_probes = static_cast<const float4*>(pv.volume.p);
    d_points = static_cast<const float4*>(pv.in_points.p);
    d_out = static_cast<float4*>(pv.out.p);
  }
  probe_sample_enqueue(ctx, g, d_probes, d_points, (uint32_t)n, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out, d_out, sizeof(float4) * n, hipMemcpyDeviceToHost, s);
  return drain(ctx, __func__, e);
}

}  // extern "C"
