// hj_lightmap_texels, hj_bake_lightmap, hj_bake_lightmap_filtered, hj_bake_lightmap_adaptive: the uploaded scene's triangle UVs rasterised into gather points, and the gather's records
// scattered into an atlas image ("Light-map baking").
//
// The kernels are kernels/hj_lightmap.h's (beside it hj_compact.h and hj_num.h alone, so the path kernels' machine code does not
// depend on this unit).  The gather of the bake is hj_trace_irradiance itself, called with device arrays: it
// enters fixed_spp_query with the gather's own chunk function, and nothing of its plan or its round loop is restated here.
//   texels:  owner map = 0xFFFFFFFF  ->  k_lm_owner  ->  k_lm_owner_wide  ->  k_lm_count  ->  k_lm_scan  ->  k_lm_emit
//   bake:    texels (a synchronisation: the count sizes the buffers)  ->  hj_trace_irradiance  ->  image = 0  ->  k_lm_scatter  ->
//            [the filter's iterations: api/lightmap_filter.hip]  ->  gutter x k_lm_dilate between two images
//   adaptive bake:  the same with hj_trace_irradiance_adaptive as the gather and, for k_lm_scatter, api/gather_adaptive.hip's scatter
//            (lightmap_scatter_adaptive: the scale per texel from the record's own sample count, and the sample map)
#include "hj_internal.h"
#include "../kernels/hj_lightmap.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

// What both entry points refuse of a desc, without a device (fn: the entry point's name)
int check_desc(hj_context* ctx, const char* fn, const hj_lightmap_desc* d) {
  if (d->flags & ~(uint32_t)HJ_LIGHTMAP_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown flag bits 0x%x", fn, d->flags);
  HJ_TRY(lightmap_atlas_check(ctx, fn, d->width, d->height));
  if (!std::isfinite(d->offset)) return set_error(ctx, HJ_ERR_INVALID, "%s: offset %g is not finite", fn, (double)d->offset);
  return HJ_OK;
}

// ... and with the scene at hand: the triangle range -> a.first, a.count
int check_range(hj_context* ctx, const char* fn, const hj_lightmap_desc* d, hj::LmArgs& a) {
  const uint32_t nt = ctx->scene.nt;
  if (d->first_triangle > nt || (d->num_triangles != 0 && d->num_triangles > nt - d->first_triangle))
    return set_error(ctx, HJ_ERR_INVALID, "%s: triangles [%u, %u + %u) of a scene with %u", fn, d->first_triangle, d->first_triangle, d->num_triangles, nt);
  a.tris = ctx->scene.triangles;
  a.verts = ctx->scene.vertices;
  a.first = d->first_triangle;
  a.count = d->num_triangles != 0 ? d->num_triangles : nt - d->first_triangle;
  a.W = d->width;
  a.H = d->height;
  a.lane_texels = (uint32_t)ctx->tuning.lightmap_lane_texels;
  a.seed = d->seed;
  a.seed_stride = d->seed_stride;
  a.offset = d->offset;
  return HJ_OK;
}

// Owner map, counts and scan of desc's texels on the context's stream, into the context's buffers: nothing of the caller's is touched.
// -> d_owner, d_counts (nb tile offsets, then the total).  Enqueues only.
int enqueue_owner_and_scan(hj_context* ctx, const hj::LmArgs& a, uint32_t*& d_owner, uint32_t*& d_counts, uint32_t& nb) {
  const uint32_t n = a.W * a.H;
  nb = (n + hj::kLmThreads - 1u) / hj::kLmThreads;
  hj_context::Lightmap& lm = ctx->lightmap;
  HJ_TRY(dev_alloc(ctx, lm.owner, sizeof(uint32_t) * (size_t)n));
  HJ_TRY(dev_alloc(ctx, lm.counts, sizeof(uint32_t) * ((size_t)nb + 1)));
  d_owner = static_cast<uint32_t*>(lm.owner.p);
  d_counts = static_cast<uint32_t*>(lm.counts.p);
  hipStream_t s = ctx->stream;
  HJ_HIP(ctx, hipMemsetAsync(d_owner, 0xFF, sizeof(uint32_t) * (size_t)n, s));
  if (a.count != 0) {
    // a wave takes 64 triangles at a time; enough workgroups to fill the device, no more than the triangles need
    const uint32_t groups = (uint32_t)(((uint64_t)a.count + 63u) / 64u);
    const uint32_t fill = (uint32_t)ctx->num_cus * 8u;
    const uint32_t gx = std::max(1u, std::min((groups + 3u) / 4u, fill));
    HJ_TRY(dev_alloc(ctx, lm.masks, sizeof(unsigned long long) * (size_t)groups));
    unsigned long long* d_masks = static_cast<unsigned long long*>(lm.masks.p);
    hipLaunchKernelGGL(hj::k_lm_owner, dim3(gx), dim3(hj::kLmThreads), 0, s, a, d_owner, d_masks);
    // The boxes too large for a lane: few workgroups a row - a lane reads 8 bytes per 64 triangles to find them - and as many rows as
    // fill the device (at most 256), so that one chart over the whole atlas is every row's work whether 12 triangles or a million
    // stand beside it.
    const uint32_t wx = std::max(1u, std::min((groups + 255u) / 256u, 8u));   // (a wave reads 64 groups' masks at a time)
    const uint32_t rows = (uint32_t)Tuning::pick(ctx->tuning.lightmap_slices, (int)std::max(1u, std::min(256u, fill / wx)));
    hipLaunchKernelGGL(hj::k_lm_owner_wide, dim3(wx, rows), dim3(hj::kLmThreads), 0, s, a, static_cast<const unsigned long long*>(d_masks), groups, d_owner);
  }
  hipLaunchKernelGGL(hj::k_lm_count, dim3(nb), dim3(hj::kLmThreads), 0, s, a, n, d_owner, d_counts);
  hipLaunchKernelGGL(hj::k_lm_scan, dim3(1), dim3(hj::kLmThreads), 0, s, d_counts, nb);
  HJ_HIP(ctx, hipGetLastError());
  return HJ_OK;
}

void enqueue_emit(hj_context* ctx, const hj::LmArgs& a, const uint32_t* d_owner, const uint32_t* d_counts, uint32_t nb, uint64_t capacity,
                  float4* d_points, uint32_t* d_owner_out) {
  hipLaunchKernelGGL(hj::k_lm_emit, dim3(nb), dim3(hj::kLmThreads), 0, ctx->stream, a, a.W * a.H, d_owner, d_counts, nb, capacity, d_points, d_owner_out);
}

// The three bakes (fn: the entry point's name).  filter == NULL or no iterations: hj_bake_lightmap, launch for launch.  adaptive:
// hj_bake_lightmap_adaptive - spp is not read, the gather is hj_trace_irradiance_adaptive and the scatter api/gather_adaptive.hip's,
// which also fills sample_map (may be NULL; only read with adaptive).
int bake(hj_context* ctx, const char* fn, const hj_lightmap_desc* desc, uint32_t spp, bool adaptive, const hj_adaptive_opts* aopts, uint32_t gutter,
         const hj_lightmap_filter* filter, const hj_render_opts* opts, float* image, uint32_t* sample_map, size_t* out_count, hj_render_stats* stats) {
  if (!desc || !image) return set_error(ctx, HJ_ERR_INVALID, "%s: null %s", fn, !desc ? "desc" : "image");
  HJ_TRY(check_desc(ctx, fn, desc));
  const bool on_device = (desc->flags & HJ_LIGHTMAP_DEVICE_ARRAYS) != 0;
  hj_adaptive_opts ad{};
  if (adaptive) HJ_TRY(adaptive_opts_check(ctx, fn, aopts, ad));
  else if (spp == 0 || spp > 65536u) return set_error(ctx, HJ_ERR_INVALID, "%s: spp %u outside [1, 65536]", fn, spp);
  if (gutter > HJ_LIGHTMAP_MAX_GUTTER) return set_error(ctx, HJ_ERR_INVALID, "%s: gutter %u above %u passes", fn, gutter, HJ_LIGHTMAP_MAX_GUTTER);
  if (on_device && misaligned(image))
    return set_error(ctx, HJ_ERR_INVALID, "%s: a device image must be 16-byte aligned", fn);
  if (on_device && adaptive && misaligned(sample_map))
    return set_error(ctx, HJ_ERR_INVALID, "%s: a device sample map must be 16-byte aligned", fn);
  if (filter) HJ_TRY(lightmap_filter_check(ctx, fn, filter));
  const uint32_t iterations = filter ? filter->iterations : 0u;
  hj_render_opts o;
  HJ_TRY(query_render_opts(ctx, fn, opts, o));
  HJ_TRY(query_gate(ctx, fn));
  hj::LmArgs a{};
  HJ_TRY(check_range(ctx, fn, desc, a));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = a.W * a.H;
  hj_context::Lightmap& lm = ctx->lightmap;

  // 1. the texels: the count comes to the host, because it sizes the points, the records and the gather
  uint32_t *d_owner = nullptr, *d_counts = nullptr, nb = 0, total = 0;
  int rc = enqueue_owner_and_scan(ctx, a, d_owner, d_counts, nb);
  if (rc == HJ_OK && hipMemcpyAsync(&total, d_counts + nb, sizeof total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = set_error(ctx, HJ_ERR_DEVICE, "%s: the count's copy failed", fn);
  HJ_TRY(drain(ctx, fn, rc));
  // the images: with f filter iterations and g gutter passes the scatter starts where f + g swaps end in the caller's device image (or in image[0])
  float4* img[2] = {nullptr, nullptr};
  if (on_device) img[0] = reinterpret_cast<float4*>(image);
  else {
    HJ_TRY(dev_alloc(ctx, lm.image[0], sizeof(float4) * (size_t)n));
    img[0] = static_cast<float4*>(lm.image[0].p);
  }
  if (gutter + iterations != 0) {
    HJ_TRY(dev_alloc(ctx, lm.image[1], sizeof(float4) * (size_t)n));
    img[1] = static_cast<float4*>(lm.image[1].p);
  }
  uint32_t cur = (gutter + iterations) & 1u;     // (after that many swaps: 0)
  uint32_t* d_map = nullptr;                     // the adaptive bake's sample map: the caller's device array, or staging of a host array
  if (adaptive && sample_map) {
    d_map = sample_map;
    if (!on_device) {
      HJ_TRY(dev_alloc(ctx, lm.sample_map, sizeof(uint32_t) * (size_t)n));
      d_map = static_cast<uint32_t*>(lm.sample_map.p);
    }
  }
  float4 *d_points = nullptr, *d_records = nullptr;
  if (total != 0) {
    HJ_TRY(dev_alloc(ctx, lm.points, sizeof(float4) * 2 * (size_t)total));
    HJ_TRY(dev_alloc(ctx, lm.records, sizeof(float4) * 2 * (size_t)total));
    d_points = static_cast<float4*>(lm.points.p);
    d_records = static_cast<float4*>(lm.records.p);
    enqueue_emit(ctx, a, d_owner, d_counts, nb, total, d_points, nullptr);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return drain(ctx, fn, e);
    // 2. the gather: the same stream, so it runs behind the emit; it returns with its records complete
    if (adaptive)
      HJ_TRY(hj_trace_irradiance_adaptive(ctx, reinterpret_cast<const float*>(d_points), total, &ad, &o, HJ_GATHER_DEVICE_ARRAYS,
                                          reinterpret_cast<float*>(d_records), nullptr, stats));
    else
      HJ_TRY(hj_trace_irradiance(ctx, reinterpret_cast<const float*>(d_points), total, spp, &o, HJ_GATHER_DEVICE_ARRAYS, reinterpret_cast<float*>(d_records), stats));
  } else if (stats) {
    std::memset(stats, 0, sizeof *stats);
  }
  // 3. scatter, the filter's iterations, 4. dilate
  hipStream_t s = ctx->stream;
  hipError_t e = hipMemsetAsync(img[cur], 0, sizeof(float4) * (size_t)n, s);
  if (e == hipSuccess && d_map) e = hipMemsetAsync(d_map, 0, sizeof(uint32_t) * (size_t)n, s);
  if (e == hipSuccess && total != 0 && adaptive) {
    lightmap_scatter_adaptive(d_points, d_records, total, img[cur], d_map, s);
  } else if (e == hipSuccess && total != 0) {
    const float scale = 3.14159274f / (float)spp;
    hipLaunchKernelGGL(hj::k_lm_scatter, dim3((total + hj::kLmThreads - 1u) / hj::kLmThreads), dim3(hj::kLmThreads), 0, s, d_points, d_records, total, scale,
                       img[cur]);
  }
  if (e == hipSuccess && iterations != 0) {
    if (const int frc = lightmap_filter_enqueue(ctx, *filter, a.W, a.H, d_points, total, img, cur); frc != HJ_OK) return drain(ctx, fn, frc);
  }
  for (uint32_t g = 0; g < gutter && e == hipSuccess; g++) {
    hipLaunchKernelGGL(hj::k_lm_dilate, dim3(nb), dim3(hj::kLmThreads), 0, s, static_cast<const float4*>(img[cur]), img[cur ^ 1u], a.W, a.H);
    cur ^= 1u;
  }
  if (e == hipSuccess) e = hipGetLastError();
  // 5. to the host
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(image, img[cur], sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !on_device && d_map) e = hipMemcpyAsync(sample_map, d_map, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, s);
  HJ_TRY(drain(ctx, fn, e));
  if (out_count) *out_count = total;
  return HJ_OK;
}

}  // namespace

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_trace_paths' order and style).
int hj_lightmap_texels(hj_context* ctx, const hj_lightmap_desc* desc, float* points, size_t capacity, uint32_t* owner, size_t* out_count) {
  if (!desc || !out_count) return set_error(ctx, HJ_ERR_INVALID, "hj_lightmap_texels: null %s", !desc ? "desc" : "out_count");
  HJ_TRY(check_desc(ctx, __func__, desc));
  const bool on_device = (desc->flags & HJ_LIGHTMAP_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(points, owner))
    return set_error(ctx, HJ_ERR_INVALID, "hj_lightmap_texels: device arrays must be 16-byte aligned");
  HJ_TRY(query_gate(ctx, __func__));
  hj::LmArgs a{};
  HJ_TRY(check_range(ctx, __func__, desc, a));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)a.W * a.H;
  uint32_t *d_owner = nullptr, *d_counts = nullptr, nb = 0;
  uint32_t total = 0;
  int rc = enqueue_owner_and_scan(ctx, a, d_owner, d_counts, nb);
  if (rc == HJ_OK && on_device) {
    // the device decides whether the records fit (k_lm_emit writes nothing when they do not): ONE synchronisation
    if (points || owner) enqueue_emit(ctx, a, d_owner, d_counts, nb, capacity, reinterpret_cast<float4*>(points), owner);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&total, d_counts + nb, sizeof total, hipMemcpyDeviceToHost, ctx->stream);
    HJ_TRY(drain(ctx, __func__, e));
  } else {
    // host arrays: the count first - it sizes the staging -, then the records
    if (rc == HJ_OK && hipMemcpyAsync(&total, d_counts + nb, sizeof total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      rc = set_error(ctx, HJ_ERR_DEVICE, "hj_lightmap_texels: the count's copy failed");
    HJ_TRY(drain(ctx, __func__, rc));
    if (points && capacity >= total && total != 0) {
      HJ_TRY(dev_alloc(ctx, ctx->lightmap.points, sizeof(float4) * 2 * (size_t)total));
      float4* d_points = static_cast<float4*>(ctx->lightmap.points.p);
      enqueue_emit(ctx, a, d_owner, d_counts, nb, capacity, d_points, nullptr);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(points, d_points, sizeof(float4) * 2 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
      if (e != hipSuccess) rc = set_error(ctx, HJ_ERR_DEVICE, "hj_lightmap_texels: %s", hipGetErrorString(e));
    }
    if (rc == HJ_OK && owner && !(points && capacity < total) &&
        hipMemcpyAsync(owner, d_owner, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      rc = set_error(ctx, HJ_ERR_DEVICE, "hj_lightmap_texels: the owner map's copy failed");
    HJ_TRY(drain(ctx, __func__, rc));
  }
  *out_count = total;
  if (points && capacity < total)
    return set_error(ctx, HJ_ERR_INVALID, "hj_lightmap_texels: %u owned texels, room for %zu points (nothing was written)", total, capacity);
  return HJ_OK;
}

int hj_bake_lightmap(hj_context* ctx, const hj_lightmap_desc* desc, uint32_t spp, uint32_t gutter, const hj_render_opts* opts, float* image,
                     size_t* out_count, hj_render_stats* stats) {
  return bake(ctx, __func__, desc, spp, false, nullptr, gutter, nullptr, opts, image, nullptr, out_count, stats);
}

int hj_bake_lightmap_filtered(hj_context* ctx, const hj_lightmap_desc* desc, uint32_t spp, uint32_t gutter, const hj_lightmap_filter* filter,
                              const hj_render_opts* opts, float* image, size_t* out_count, hj_render_stats* stats) {
  return bake(ctx, __func__, desc, spp, false, nullptr, gutter, filter, opts, image, nullptr, out_count, stats);
}

int hj_bake_lightmap_adaptive(hj_context* ctx, const hj_lightmap_desc* desc, const hj_adaptive_opts* adaptive, uint32_t gutter, const hj_lightmap_filter* filter,
                              const hj_render_opts* opts, float* image, uint32_t* sample_map, size_t* out_count, hj_render_stats* stats) {
  return bake(ctx, __func__, desc, 0, true, adaptive, gutter, filter, opts, image, sample_map, out_count, stats);
}

}  // extern "C"
