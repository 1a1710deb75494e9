// hj_denoise_frame_temporal: the last frame's history reprojected into this one, in front of hj_denoise_frame's filter (DESIGN.md 4,
// "Temporal accumulation").  hj_denoise_frame_temporal_motion: the same host routine, reprojecting through hj_render_motion's records
// ("Motion for the temporal denoiser").
//
// The kernels are kernels/hj_denoise_temporal.h's; prepare, the iterations and finish are api/denoise.hip's, through hj_internal.h:
//   k_dn_prepare  ->  k_dt_accumulate  ->  k_dt_variance  ->  the iterations (HJ_TEMPORAL_FEEDBACK: the first one into a working image,
//   k_dt_feedback behind it, and k_dn_finish when it was the only one)
// k_dt_accumulate<false> is this unit's; with a motion image the routine enters api/motion.hip's launch of k_dt_accumulate<true>.
#include "hj_internal.h"
#include "../kernels/hj_denoise_temporal.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return a && b && pa < pb + nb && pb < pa + na;
}

// Both entry points (kFn: which one, for the messages).  motion == nullptr: hj_denoise_frame_temporal.
int temporal(hj_context* ctx, const char* kFn, uint32_t width, uint32_t height, const float* beauty, const float* aov, const hj_denoise_opts* opts,
             const hj_temporal_opts* topts, const float* motion, const float* history_in, float* history_out, float* out) {
  if (!opts || !topts || !aov || !history_out || !out)
    return set_error(ctx, HJ_ERR_INVALID, "%s: null %s", kFn, !opts ? "opts" : !topts ? "topts" : !aov ? "aov" : !history_out ? "history_out" : "out");
  HJ_TRY(denoise_check(ctx, kFn, width, height, opts));
  const hj_temporal_opts& to = *topts;
  if (to.flags & ~(uint32_t)HJ_TEMPORAL_FEEDBACK) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown temporal flag bits 0x%x", kFn, to.flags);
  if (!(to.alpha >= 0.0f && to.alpha <= 1.0f)) return set_error(ctx, HJ_ERR_INVALID, "%s: alpha %g: 0 ... 1 is needed", kFn, (double)to.alpha);
  if (!(to.alpha_moments >= 0.0f && to.alpha_moments <= 1.0f))
    return set_error(ctx, HJ_ERR_INVALID, "%s: alpha_moments %g: 0 ... 1 is needed", kFn, (double)to.alpha_moments);
  if (!std::isfinite(to.depth_tolerance) || to.depth_tolerance < 0.0f)
    return set_error(ctx, HJ_ERR_INVALID, "%s: depth_tolerance %g: finite and >= 0 is needed", kFn, (double)to.depth_tolerance);
  if (!(to.normal_cos >= -1.0f && to.normal_cos <= 1.0f)) return set_error(ctx, HJ_ERR_INVALID, "%s: normal_cos %g: -1 ... 1 is needed", kFn, (double)to.normal_cos);
  if (to.max_history == 0 || to.max_history > 65535u) return set_error(ctx, HJ_ERR_INVALID, "%s: max_history %u: 1 ... 65535", kFn, to.max_history);
  if (!camera_ok(to.camera)) return set_error(ctx, HJ_ERR_INVALID, "%s: camera: finite position and rotation and a fov inside (0, 180) are needed", kFn);
  if (!camera_ok(to.prev_camera)) return set_error(ctx, HJ_ERR_INVALID, "%s: prev_camera: finite position and rotation and a fov inside (0, 180) are needed", kFn);
  const size_t n = (size_t)width * height, f4 = sizeof(float4);
  if (overlap(history_out, 3 * f4 * n, beauty, f4 * n) || overlap(history_out, 3 * f4 * n, aov, 3 * f4 * n) || overlap(history_out, 3 * f4 * n, history_in, 3 * f4 * n) ||
      overlap(history_out, 3 * f4 * n, out, f4 * n) || overlap(history_out, 3 * f4 * n, motion, f4 * n))
    return set_error(ctx, HJ_ERR_INVALID, "%s: history_out aliases an input or out", kFn);
  const bool on_device = (opts->flags & HJ_DENOISE_DEVICE_ARRAYS) != 0;
  if (on_device && misaligned(beauty, aov, out, history_in, history_out, motion))
    return set_error(ctx, HJ_ERR_INVALID, "%s: device arrays must be 16-byte aligned", kFn);
  DenoiseFrame f;
  HJ_TRY(denoise_begin(ctx, kFn, width, height, beauty, aov, out, on_device, f));
  hj_context::Denoise& dn = ctx->denoise;
  const float4* d_hin = reinterpret_cast<const float4*>(history_in);
  const float4* d_motion = reinterpret_cast<const float4*>(motion);
  float4* d_hout = reinterpret_cast<float4*>(history_out);
  hipStream_t s = ctx->stream;
  hipError_t e = f.e;
  if (!on_device) {
    int rc = dev_alloc(ctx, dn.out_history, 3 * f4 * n);
    if (rc == HJ_OK && history_in) rc = dev_alloc(ctx, dn.in_history, 3 * f4 * n);
    if (rc == HJ_OK && motion) rc = dev_alloc(ctx, dn.in_motion, f4 * n);
    if (rc != HJ_OK) return drain(ctx, kFn, rc);
    d_hout = static_cast<float4*>(dn.out_history.p);
    if (motion) {
      if (e == hipSuccess) e = hipMemcpyAsync(dn.in_motion.p, motion, f4 * n, hipMemcpyHostToDevice, s);
      d_motion = static_cast<const float4*>(dn.in_motion.p);
    }
    if (history_in) {
      if (e == hipSuccess) e = hipMemcpyAsync(dn.in_history.p, history_in, 3 * f4 * n, hipMemcpyHostToDevice, s);
      d_hin = static_cast<const float4*>(dn.in_history.p);
    }
  }
  if (e == hipSuccess) {
    const uint32_t W = width, H = height;
    const dim3 tile_grid((W + hj::kDnTX - 1u) / hj::kDnTX, (H + hj::kDnTY - 1u) / hj::kDnTY), blk(hj::kDnTX * hj::kDnTY);
    const dim3 lane_grid(((uint32_t)n + hj::kDnThreads - 1u) / hj::kDnThreads);
    denoise_prepare_enqueue(ctx, f);
    const hj::DtArgs a{f.guide, f.work[1], d_hin, d_motion, d_hout, W, H, hj::dt_host_camera(to.camera), hj::dt_host_camera(to.prev_camera), to.alpha,
                       to.alpha_moments, to.depth_tolerance, to.normal_cos, (float)to.max_history};
    if (motion) dt_accumulate_motion_enqueue(ctx, a);
    else hipLaunchKernelGGL(hj::k_dt_accumulate<false>, tile_grid, blk, 0, s, a);
    hipLaunchKernelGGL(hj::k_dt_variance, tile_grid, blk, 0, s, f.guide, static_cast<const float4*>(f.work[1]), f.work[0], static_cast<const float4*>(d_hout), W, H);
    uint32_t cur = 0;
    if ((to.flags & HJ_TEMPORAL_FEEDBACK) != 0 && opts->iterations >= 1u) {
      // the first iteration never remodulates: the history wants I' itself (iterations == 1: k_dn_finish behind it)
      denoise_filter_enqueue(ctx, *opts, f, cur, 0u, 1u, false);
      hipLaunchKernelGGL(hj::k_dt_feedback, lane_grid, dim3(hj::kDnThreads), 0, s, static_cast<const float4*>(f.guide), static_cast<const float4*>(f.work[cur]),
                         (uint32_t)n, d_hout);
      denoise_filter_enqueue(ctx, *opts, f, cur, 1u, opts->iterations, true);
    } else {
      denoise_filter_enqueue(ctx, *opts, f, cur, 0u, opts->iterations, true);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(out, f.out, f4 * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !on_device) e = hipMemcpyAsync(history_out, d_hout, 3 * f4 * n, hipMemcpyDeviceToHost, s);
  return drain(ctx, kFn, e);
}

}  // namespace

extern "C" {

int hj_denoise_frame_temporal(hj_context* ctx, uint32_t width, uint32_t height, const float* beauty, const float* aov, const hj_denoise_opts* opts,
                              const hj_temporal_opts* topts, const float* history_in, float* history_out, float* out) {
  return temporal(ctx, __func__, width, height, beauty, aov, opts, topts, nullptr, history_in, history_out, out);
}

int hj_denoise_frame_temporal_motion(hj_context* ctx, uint32_t width, uint32_t height, const float* beauty, const float* aov, const hj_denoise_opts* opts,
                                     const hj_temporal_opts* topts, const float* motion, const float* history_in, float* history_out, float* out) {
  return temporal(ctx, __func__, width, height, beauty, aov, opts, topts, motion, history_in, history_out, out);
}

}  // extern "C"
