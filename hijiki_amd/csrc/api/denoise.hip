// hj_denoise_frame: the variance-guided a-trous filter over a frame, guided by the frame's AOVs ("Frame denoiser").
//
// The kernels are kernels/hj_denoise.h's (beside it hj_num.h alone, so no other unit's machine code depends on this one).
//   k_dn_prepare  ->  k_dn_variance  ->  iterations x (k_dn_filter_lds | k_dn_filter_direct) between two images, the last one
//   storing the remodulated result (iterations == 0: k_dn_finish)
// The checks, the buffers, the prepare stage and the iterations are ONE text for this call and hj_denoise_frame_temporal
// (api/denoise_temporal.hip; declared in hj_internal.h), which puts its own stages between them.
#include "hj_internal.h"
#include "../kernels/hj_denoise.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

float inv_sq(float sigma) { return sigma > 0.0f ? 1.0f / (sigma * sigma) : 0.0f; }

}  // namespace

namespace hjapi {

// What both entry points refuse of (opts, width, height) behind their null checks, in the header's order, without a device
int denoise_check(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, const hj_denoise_opts* opts) {
  if (opts->flags & ~(uint32_t)HJ_DENOISE_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown flag bits 0x%x", fn, opts->flags);
  if (opts->iterations > HJ_DENOISE_MAX_ITERATIONS)
    return set_error(ctx, HJ_ERR_INVALID, "%s: %u iterations, at most %u", fn, opts->iterations, HJ_DENOISE_MAX_ITERATIONS);
  const float sigma[4] = {opts->sigma_normal, opts->sigma_depth, opts->sigma_luminance, opts->sigma_albedo};
  const char* const name[4] = {"sigma_normal", "sigma_depth", "sigma_luminance", "sigma_albedo"};
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f) return set_error(ctx, HJ_ERR_INVALID, "%s: %s %g: finite and >= 0 is needed", fn, name[k], (double)sigma[k]);
  if (width == 0 || height == 0 || width > kDenoiseMaxSide || height > kDenoiseMaxSide)
    return set_error(ctx, HJ_ERR_INVALID, "%s: image %u x %u: 1 ... %u each", fn, width, height, kDenoiseMaxSide);
  return HJ_OK;
}

// Behind the argument checks: the queries' gate without its last check (no scene is needed), what beauty == NULL asks of the
// framebuffer, the context's buffers and the staging of host arrays.  On HJ_OK f holds the device arrays of the call and, in f.e,
// the first error of the copies enqueued (the caller ends in drain() whatever it is).
int denoise_begin(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, const float* beauty, const float* aov, float* out, bool on_device,
                  DenoiseFrame& f) {
  HJ_TRY(context_gate(ctx, fn));
  if (!beauty) {
    if (!ctx->accum) return set_error(ctx, HJ_ERR_STATE, "%s: null beauty and no framebuffer", fn);
    if (ctx->width != width || ctx->height != height)
      return set_error(ctx, HJ_ERR_INVALID, "%s: null beauty: the framebuffer is %u x %u, the image %u x %u", fn, ctx->width, ctx->height, width, height);
  }
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)width * height, f4 = sizeof(float4);
  hj_context::Denoise& dn = ctx->denoise;
  HJ_TRY(dev_alloc(ctx, dn.guide, 3 * f4 * n));
  HJ_TRY(dev_alloc(ctx, dn.image[0], f4 * n));
  HJ_TRY(dev_alloc(ctx, dn.image[1], f4 * n));
  f.W = width;
  f.H = height;
  f.guide = static_cast<float4*>(dn.guide.p);
  f.work[0] = static_cast<float4*>(dn.image[0].p);
  f.work[1] = static_cast<float4*>(dn.image[1].p);
  f.beauty = beauty ? reinterpret_cast<const float4*>(beauty) : ctx->accum;
  f.aov = reinterpret_cast<const float4*>(aov);
  f.out = reinterpret_cast<float4*>(out);
  f.e = hipSuccess;
  if (on_device) return HJ_OK;
  hipStream_t s = ctx->stream;
  HJ_TRY(dev_alloc(ctx, dn.in_aov, 3 * f4 * n));
  HJ_TRY(dev_alloc(ctx, dn.out, f4 * n));
  if (beauty) HJ_TRY(dev_alloc(ctx, dn.in_beauty, f4 * n));
  if (beauty) {
    f.e = hipMemcpyAsync(dn.in_beauty.p, beauty, f4 * n, hipMemcpyHostToDevice, s);
    f.beauty = static_cast<const float4*>(dn.in_beauty.p);
  }
  if (f.e == hipSuccess) f.e = hipMemcpyAsync(dn.in_aov.p, aov, 3 * f4 * n, hipMemcpyHostToDevice, s);
  f.aov = static_cast<const float4*>(dn.in_aov.p);
  f.out = static_cast<float4*>(dn.out.p);
  return HJ_OK;
}

// PREPARE: the guide's first two records and (I, 0) or (c, 0) into work[1]
void denoise_prepare_enqueue(hj_context* ctx, const DenoiseFrame& f) {
  const dim3 tile_grid((f.W + hj::kDnTX - 1u) / hj::kDnTX, (f.H + hj::kDnTY - 1u) / hj::kDnTY), blk(hj::kDnTX * hj::kDnTY);
  hipLaunchKernelGGL(hj::k_dn_prepare, tile_grid, blk, 0, ctx->stream, f.aov, f.beauty, f.W, f.H, f.guide, f.work[1]);
}

// Iterations [i0, i1) over (I, V) in work[cur], cur flipped by each.  finish: the last of them stores the remodulated result into
// f.out; with none to run (i0 == i1), the remodulation of work[cur] alone.
void denoise_filter_enqueue(hj_context* ctx, const hj_denoise_opts& o, const DenoiseFrame& f, uint32_t& cur, uint32_t i0, uint32_t i1, bool finish) {
  const uint32_t W = f.W, H = f.H, n = W * H;                          // (<= 2^28)
  hipStream_t s = ctx->stream;
  const dim3 tile_grid((W + hj::kDnTX - 1u) / hj::kDnTX, (H + hj::kDnTY - 1u) / hj::kDnTY), blk(hj::kDnTX * hj::kDnTY);
  if (finish && i0 == i1) {
    const dim3 lane_grid((n + hj::kDnThreads - 1u) / hj::kDnThreads);
    hipLaunchKernelGGL(hj::k_dn_finish, lane_grid, dim3(hj::kDnThreads), 0, s, static_cast<const float4*>(f.guide), static_cast<const float4*>(f.work[cur]), n, f.out);
    return;
  }
  hj::DnArgs a{f.guide, nullptr, nullptr, W, H, 1u, inv_sq(o.sigma_normal), o.sigma_depth, o.sigma_luminance, inv_sq(o.sigma_albedo), 0u};
  const uint32_t lds_step = (uint32_t)ctx->tuning.denoise_lds_step;    // the largest step that takes the LDS form
  for (uint32_t i = i0; i < i1; i++) {
    const bool last = finish && i + 1u == i1;
    a.s = 1u << i;
    a.in = f.work[cur];
    a.out = last ? f.out : f.work[cur ^ 1u];
    a.finish = last ? 1u : 0u;
    if (a.s <= lds_step) {
      const uint32_t tiles_x = ((W + a.s - 1u) / a.s + hj::kDnTX - 1u) / hj::kDnTX, tiles_y = ((H + a.s - 1u) / a.s + hj::kDnTY - 1u) / hj::kDnTY;
      hipLaunchKernelGGL(hj::k_dn_filter_lds, dim3(a.s * tiles_x, a.s * tiles_y), blk, 0, s, a, tiles_x, tiles_y);   // (s * tiles_y <= 2048 + 127)
    } else {
      hipLaunchKernelGGL(hj::k_dn_filter_direct, tile_grid, blk, 0, s, a);
    }
    cur ^= 1u;
  }
}

}  // namespace hjapi

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_filter_lightmap's and hj_render_aovs' order
// and style); then the queries' gate without its last check: no scene is needed, this call traces nothing.
int hj_denoise_frame(hj_context* ctx, uint32_t width, uint32_t height, const float* beauty, const float* aov, const hj_denoise_opts* opts, float* out) {
  if (!opts || !aov || !out) return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: null %s", !opts ? "opts" : !aov ? "aov" : "out");
  HJ_TRY(denoise_check(ctx, __func__, width, height, opts));
  const bool on_device = (opts->flags & HJ_DENOISE_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(beauty, aov, out))
    return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: device arrays must be 16-byte aligned");
  DenoiseFrame f;
  HJ_TRY(denoise_begin(ctx, __func__, width, height, beauty, aov, out, on_device, f));
  hipError_t e = f.e;
  if (e == hipSuccess) {
    denoise_prepare_enqueue(ctx, f);
    const dim3 tile_grid((width + hj::kDnTX - 1u) / hj::kDnTX, (height + hj::kDnTY - 1u) / hj::kDnTY), blk(hj::kDnTX * hj::kDnTY);
    hipLaunchKernelGGL(hj::k_dn_variance, tile_grid, blk, 0, ctx->stream, f.guide, static_cast<const float4*>(f.work[1]), f.work[0], width, height);
    uint32_t cur = 0;
    denoise_filter_enqueue(ctx, *opts, f, cur, 0u, opts->iterations, true);
    e = hipGetLastError();
  }
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out, f.out, sizeof(float4) * (size_t)width * height, hipMemcpyDeviceToHost, ctx->stream);
  return drain(ctx, __func__, e);
}

}  // extern "C"
