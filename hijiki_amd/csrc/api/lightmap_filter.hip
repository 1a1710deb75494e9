// hj_filter_lightmap: the edge-avoiding a-trous filter over a light-map atlas ("Light-map filter"), and the host half of
// the filter that hj_bake_lightmap_filtered (api/lightmap.hip) enters between its scatter and its dilation.
//
// The kernels are kernels/hj_lightmap_filter.h's (beside it hj_num.h and the light-map constants alone, so the path kernels' machine
// code does not depend on this unit).
//   guide = 0  ->  k_lm_guide  ->  iterations x (k_lm_filter_lds | k_lm_filter_direct) between two images
#include "hj_internal.h"
#include "../kernels/hj_lightmap_filter.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hjapi {

int lightmap_filter_check(hj_context* ctx, const char* fn, const hj_lightmap_filter* f) {
  if (f->flags & ~(uint32_t)HJ_LIGHTMAP_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown filter flag bits 0x%x", fn, f->flags);
  if (f->iterations > HJ_LIGHTMAP_FILTER_MAX_ITERATIONS)
    return set_error(ctx, HJ_ERR_INVALID, "%s: %u filter iterations, at most %u", fn, f->iterations, HJ_LIGHTMAP_FILTER_MAX_ITERATIONS);
  const float sigma[3] = {f->sigma_position, f->sigma_normal, f->sigma_color};
  const char* const name[3] = {"sigma_position", "sigma_normal", "sigma_color"};
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f) return set_error(ctx, HJ_ERR_INVALID, "%s: %s %g: finite and >= 0 is needed", fn, name[k], (double)sigma[k]);
  return HJ_OK;
}

static float inv_sq(float sigma) { return sigma > 0.0f ? 1.0f / (sigma * sigma) : 0.0f; }

int lightmap_filter_enqueue(hj_context* ctx, const hj_lightmap_filter& f, uint32_t W, uint32_t H, const float4* d_points, uint32_t count, float4* const img[2],
                            uint32_t& cur) {
  if (f.iterations == 0) return HJ_OK;
  const size_t n = (size_t)W * H;
  hj_context::Lightmap& lm = ctx->lightmap;
  HJ_TRY(dev_alloc(ctx, lm.guide, sizeof(float4) * 2 * n));
  float4* d_guide = static_cast<float4*>(lm.guide.p);
  hipStream_t s = ctx->stream;
  HJ_HIP(ctx, hipMemsetAsync(d_guide, 0, sizeof(float4) * 2 * n, s));
  if (count != 0)
    hipLaunchKernelGGL(hj::k_lm_guide, dim3((count + hj::kLmThreads - 1u) / hj::kLmThreads), dim3(hj::kLmThreads), 0, s, d_points, count, (uint32_t)n, d_guide);
  hj::LmFilterArgs a{d_guide, nullptr, nullptr, W, H, 1u, inv_sq(f.sigma_position), inv_sq(f.sigma_normal), inv_sq(f.sigma_color)};
  const uint32_t lds_step = (uint32_t)ctx->tuning.lightmap_filter_lds_step;    // the largest step that takes the LDS form
  const dim3 blk(hj::kLfTX * hj::kLfTY);
  for (uint32_t i = 0; i < f.iterations; i++) {
    a.s = 1u << i;
    a.in = img[cur];
    a.out = img[cur ^ 1u];
    if (a.s <= lds_step) {
      const uint32_t tiles_x = ((W + a.s - 1u) / a.s + hj::kLfTX - 1u) / hj::kLfTX, tiles_y = ((H + a.s - 1u) / a.s + hj::kLfTY - 1u) / hj::kLfTY;
      hipLaunchKernelGGL(hj::k_lm_filter_lds, dim3(a.s * tiles_x, a.s * tiles_y), blk, 0, s, a, tiles_x, tiles_y);   // (s * tiles_y <= 2048 + 127)
    } else {
      hipLaunchKernelGGL(hj::k_lm_filter_direct, dim3((W + hj::kLfTX - 1u) / hj::kLfTX, (H + hj::kLfTY - 1u) / hj::kLfTY), blk, 0, s, a);
    }
    cur ^= 1u;
    a.ic = a.ic * 4.0f;
  }
  HJ_HIP(ctx, hipGetLastError());
  return HJ_OK;
}

}  // namespace hjapi

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_lightmap_texels' order and style).
int hj_filter_lightmap(hj_context* ctx, uint32_t width, uint32_t height, const float* points, size_t count, const hj_lightmap_filter* filter, float* image) {
  if (!filter || !image || (count != 0 && !points))
    return set_error(ctx, HJ_ERR_INVALID, "hj_filter_lightmap: null %s", !filter ? "filter" : !image ? "image" : "points");
  HJ_TRY(lightmap_filter_check(ctx, __func__, filter));
  HJ_TRY(lightmap_atlas_check(ctx, __func__, width, height));
  const size_t n = (size_t)width * height;
  if (count > n) return set_error(ctx, HJ_ERR_INVALID, "hj_filter_lightmap: %zu points for %zu texels", count, n);
  const bool on_device = (filter->flags & HJ_LIGHTMAP_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(points, image))
    return set_error(ctx, HJ_ERR_INVALID, "hj_filter_lightmap: device arrays must be 16-byte aligned");
  if (!on_device) {                            // (device arrays: the caller's contract; the kernels skip what names no texel)
    for (size_t i = 0; i < count; i++) {
      const float* p = points + 8 * i;
      uint32_t t, before = 0;
      std::memcpy(&t, p + 7, sizeof t);
      if (i != 0) std::memcpy(&before, p - 1, sizeof before);
      if (t >= n || (i != 0 && t <= before))
        return set_error(ctx, HJ_ERR_INVALID, "hj_filter_lightmap: point %zu names texel %u: strictly ascending and below %zu is needed", i, t, n);
      for (int k = 0; k < 6; k++)
        if (!std::isfinite(p[k])) return set_error(ctx, HJ_ERR_INVALID, "hj_filter_lightmap: point %zu has a non-finite %s", i, k < 3 ? "position" : "normal");
    }
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (filter->iterations == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::Lightmap& lm = ctx->lightmap;
  hipStream_t s = ctx->stream;
  float4* img[2] = {nullptr, nullptr};
  const float4* d_points = reinterpret_cast<const float4*>(points);
  HJ_TRY(dev_alloc(ctx, lm.image[1], sizeof(float4) * n));
  img[1] = static_cast<float4*>(lm.image[1].p);
  if (on_device) img[0] = reinterpret_cast<float4*>(image);
  else {
    HJ_TRY(dev_alloc(ctx, lm.image[0], sizeof(float4) * n));
    img[0] = static_cast<float4*>(lm.image[0].p);
    HJ_HIP(ctx, hipMemcpyAsync(img[0], image, sizeof(float4) * n, hipMemcpyHostToDevice, s));
    if (count != 0) {
      HJ_TRY(drain(ctx, __func__, dev_alloc(ctx, lm.points, sizeof(float4) * 2 * count)));
      if (hipMemcpyAsync(lm.points.p, points, sizeof(float4) * 2 * count, hipMemcpyHostToDevice, s) != hipSuccess)
        return drain(ctx, __func__, set_error(ctx, HJ_ERR_DEVICE, "hj_filter_lightmap: the points' copy failed"));
      d_points = static_cast<const float4*>(lm.points.p);
    }
  }
  uint32_t cur = 0;
  int rc = lightmap_filter_enqueue(ctx, *filter, width, height, d_points, (uint32_t)count, img, cur);
  // the result to `image`: from whichever image the last iteration wrote (an odd number of iterations: one copy on the device route)
  if (rc == HJ_OK && (!on_device || cur != 0u) &&
      hipMemcpyAsync(image, img[cur], sizeof(float4) * n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = set_error(ctx, HJ_ERR_DEVICE, "hj_filter_lightmap: the image's copy failed");
  return drain(ctx, __func__, rc);
}

}  // extern "C"
