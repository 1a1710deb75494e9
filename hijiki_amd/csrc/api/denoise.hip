// hj_denoise_frame: the variance-guided a-trous filter over a frame, guided by the frame's AOVs ("Frame denoiser").
//
// The kernels are kernels/hj_denoise.h's (beside it hj_num.h alone, so no other unit's machine code depends on this one).
//   k_dn_prepare  ->  k_dn_variance  ->  iterations x (k_dn_filter_lds | k_dn_filter_direct) between two images, the last one
//   storing the remodulated result (iterations == 0: k_dn_finish)
#include "hj_internal.h"
#include "../kernels/hj_denoise.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

constexpr uint32_t kDenoiseMaxSide = 16384u;

float inv_sq(float sigma) { return sigma > 0.0f ? 1.0f / (sigma * sigma) : 0.0f; }

// Behind the checks and the gate: everything enqueued on the context's stream; the result lands in d_out.
// work[0], work[1]: the two working images; d_out may be neither.
hipError_t denoise_enqueue(hj_context* ctx, const hj_denoise_opts& o, uint32_t W, uint32_t H, const float4* d_beauty, const float4* d_aov, float4* d_guide,
                           float4* const work[2], float4* d_out) {
  const uint32_t n = W * H;                                            // (<= 2^28)
  hipStream_t s = ctx->stream;
  const dim3 tile_grid((W + hj::kDnTX - 1u) / hj::kDnTX, (H + hj::kDnTY - 1u) / hj::kDnTY), blk(hj::kDnTX * hj::kDnTY);
  const dim3 lane_grid((n + hj::kDnThreads - 1u) / hj::kDnThreads);
  hipLaunchKernelGGL(hj::k_dn_prepare, tile_grid, blk, 0, s, d_aov, d_beauty, W, H, d_guide, work[1]);
  hipLaunchKernelGGL(hj::k_dn_variance, tile_grid, blk, 0, s, d_guide, static_cast<const float4*>(work[1]), work[0], W, H);
  if (o.iterations == 0) {
    hipLaunchKernelGGL(hj::k_dn_finish, lane_grid, dim3(hj::kDnThreads), 0, s, static_cast<const float4*>(d_guide), static_cast<const float4*>(work[0]), n, d_out);
    return hipGetLastError();
  }
  hj::DnArgs a{d_guide, nullptr, nullptr, W, H, 1u, inv_sq(o.sigma_normal), o.sigma_depth, o.sigma_luminance, inv_sq(o.sigma_albedo), 0u};
  const uint32_t lds_step = (uint32_t)ctx->tuning.denoise_lds_step;    // the largest step that takes the LDS form
  uint32_t cur = 0;
  for (uint32_t i = 0; i < o.iterations; i++) {
    const bool last = i + 1u == o.iterations;
    a.s = 1u << i;
    a.in = work[cur];
    a.out = last ? d_out : work[cur ^ 1u];
    a.finish = last ? 1u : 0u;
    if (a.s <= lds_step) {
      const uint32_t tiles_x = ((W + a.s - 1u) / a.s + hj::kDnTX - 1u) / hj::kDnTX, tiles_y = ((H + a.s - 1u) / a.s + hj::kDnTY - 1u) / hj::kDnTY;
      hipLaunchKernelGGL(hj::k_dn_filter_lds, dim3(a.s * tiles_x, a.s * tiles_y), blk, 0, s, a, tiles_x, tiles_y);   // (s * tiles_y <= 2048 + 127)
    } else {
      hipLaunchKernelGGL(hj::k_dn_filter_direct, tile_grid, blk, 0, s, a);
    }
    cur ^= 1u;
  }
  return hipGetLastError();
}

}  // namespace

extern "C" {

// The argument checks come first and need neither a device nor a context's state (hj_filter_lightmap's and hj_render_aovs' order
// and style); then the queries' gate without its last check: no scene is needed, this call traces nothing.
int hj_denoise_frame(hj_context* ctx, uint32_t width, uint32_t height, const float* beauty, const float* aov, const hj_denoise_opts* opts, float* out) {
  if (!opts || !aov || !out) return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: null %s", !opts ? "opts" : !aov ? "aov" : "out");
  if (opts->flags & ~(uint32_t)HJ_DENOISE_DEVICE_ARRAYS) return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: unknown flag bits 0x%x", opts->flags);
  if (opts->iterations > HJ_DENOISE_MAX_ITERATIONS)
    return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: %u iterations, at most %u", opts->iterations, HJ_DENOISE_MAX_ITERATIONS);
  const float sigma[4] = {opts->sigma_normal, opts->sigma_depth, opts->sigma_luminance, opts->sigma_albedo};
  const char* const name[4] = {"sigma_normal", "sigma_depth", "sigma_luminance", "sigma_albedo"};
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(sigma[k]) || sigma[k] < 0.0f)
      return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: %s %g: finite and >= 0 is needed", name[k], (double)sigma[k]);
  if (width == 0 || height == 0 || width > kDenoiseMaxSide || height > kDenoiseMaxSide)
    return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: image %u x %u: 1 ... %u each", width, height, kDenoiseMaxSide);
  const bool on_device = (opts->flags & HJ_DENOISE_DEVICE_ARRAYS) != 0;
  if (on_device && ((reinterpret_cast<uintptr_t>(beauty) | reinterpret_cast<uintptr_t>(aov) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0)
    return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: device arrays must be 16-byte aligned");
  HJ_TRY(context_gate(ctx, __func__));
  if (!beauty) {
    if (!ctx->accum) return set_error(ctx, HJ_ERR_STATE, "hj_denoise_frame: null beauty and no framebuffer");
    if (ctx->width != width || ctx->height != height)
      return set_error(ctx, HJ_ERR_INVALID, "hj_denoise_frame: null beauty: the framebuffer is %u x %u, the image %u x %u", ctx->width, ctx->height, width, height);
  }
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)width * height, f4 = sizeof(float4);
  hj_context::Denoise& dn = ctx->denoise;
  HJ_TRY(dev_alloc(ctx, dn.guide, 3 * f4 * n));
  HJ_TRY(dev_alloc(ctx, dn.image[0], f4 * n));
  HJ_TRY(dev_alloc(ctx, dn.image[1], f4 * n));
  float4* const work[2] = {static_cast<float4*>(dn.image[0].p), static_cast<float4*>(dn.image[1].p)};
  const float4* d_beauty = beauty ? reinterpret_cast<const float4*>(beauty) : ctx->accum;
  const float4* d_aov = reinterpret_cast<const float4*>(aov);
  float4* d_out = reinterpret_cast<float4*>(out);
  hipStream_t s = ctx->stream;
  hipError_t e = hipSuccess;
  if (!on_device) {
    HJ_TRY(dev_alloc(ctx, dn.in_aov, 3 * f4 * n));
    HJ_TRY(dev_alloc(ctx, dn.out, f4 * n));
    if (beauty) {
      HJ_TRY(dev_alloc(ctx, dn.in_beauty, f4 * n));
      e = hipMemcpyAsync(dn.in_beauty.p, beauty, f4 * n, hipMemcpyHostToDevice, s);
      d_beauty = static_cast<const float4*>(dn.in_beauty.p);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(dn.in_aov.p, aov, 3 * f4 * n, hipMemcpyHostToDevice, s);
    d_aov = static_cast<const float4*>(dn.in_aov.p);
    d_out = static_cast<float4*>(dn.out.p);
  }
  if (e == hipSuccess) e = denoise_enqueue(ctx, *opts, width, height, d_beauty, d_aov, static_cast<float4*>(dn.guide.p), work, d_out);
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out, d_out, f4 * n, hipMemcpyDeviceToHost, s);
  return drain(ctx, __func__, e);
}

}  // extern "C"
