// hj_render_motion: for every pixel, where the surface point its centre ray sees was in the previous frame ("Motion for
// the temporal denoiser") - what hj_denoise_frame_temporal_motion reprojects through in place of the static assumption.
//
// The kernels are kernels/hj_motion.h's; that header includes the kernel headers up to hj_stages.h and the functions of
// hj_denoise_temporal.h and edits none, and no other unit's machine code depends on this one.
//   k_mv_walk     ONE launch over the image's entries (a wave's 64 rays an 8 x 8 tile or a row run of 64: DeviceScene::group_tile), the
//                 raw hits straight into the motion image - the caller's, or the context's staging of a host array
//   k_mv_resolve  behind it on the context's stream, in place: the previous point from the previous shape arrays - the caller's device
//                 arrays, the context's staging of host arrays, or the uploaded array where a kind did not move - and its projection
// motion_render is also hj_render_motion_followed's host routine (api/motion_follow.hip: the rounds between the two launches, and the
// followed resolve in k_mv_resolve's place once a round ran).
// Also the one instantiation of k_dt_accumulate<true> (dt_accumulate_motion_enqueue, for api/denoise_temporal.hip): the temporal
// unit keeps the three kernels it had.
#include "hj_internal.h"
#include "../kernels/hj_motion.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

constexpr uint32_t kMotionMaxSide = 16384u;

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

}  // namespace

namespace hjapi {

void dt_accumulate_motion_enqueue(hj_context* ctx, const hj::DtArgs& a) {
  const dim3 grid((a.W + hj::kDnTX - 1u) / hj::kDnTX, (a.H + hj::kDnTY - 1u) / hj::kDnTY), blk(hj::kDnTX * hj::kDnTY);
  hipLaunchKernelGGL(hj::k_dt_accumulate<true>, grid, blk, 0, ctx->stream, a);
}

// hj_render_motion (max_follow == 0, its own two launches and nothing else) and hj_render_motion_followed (api/motion_follow.hip) behind
// the name kFn: one host routine, so the checks, their order and their texts are one.  The argument checks come first, in
// hj_trace_rays' style, and need neither a device nor a context's state; then the queries' gate.
int motion_render(hj_context* ctx, const char* kFn, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t max_follow, uint32_t flags,
                  float* motion) {
  if (!prev || !motion) return set_error(ctx, HJ_ERR_INVALID, "%s: null %s", kFn, !prev ? "prev" : "motion");
  if (flags & ~(uint32_t)(HJ_MOTION_DEVICE_SHAPES | HJ_MOTION_DEVICE_OUT)) return set_error(ctx, HJ_ERR_INVALID, "%s: unknown flag bits 0x%x", kFn, flags);
  if (width == 0 || height == 0 || width > kMotionMaxSide || height > kMotionMaxSide)
    return set_error(ctx, HJ_ERR_INVALID, "%s: image %u x %u: 1 ... %u each", kFn, width, height, kMotionMaxSide);
  if (!camera_ok(prev->camera)) return set_error(ctx, HJ_ERR_INVALID, "%s: prev->camera: finite position and rotation and a fov inside (0, 180) are needed", kFn);
  const bool dev_shapes = (flags & HJ_MOTION_DEVICE_SHAPES) != 0, dev_out = (flags & HJ_MOTION_DEVICE_OUT) != 0;
  if ((dev_out && misaligned(motion)) || (dev_shapes && misaligned(prev->spheres, prev->quads, prev->vertices)))
    return set_error(ctx, HJ_ERR_INVALID, "%s: a device array must be 16-byte aligned", kFn);
  if (max_follow > HJ_AOV_MAX_FOLLOW) return set_error(ctx, HJ_ERR_INVALID, "%s: max_follow %u above %u", kFn, max_follow, (uint32_t)HJ_AOV_MAX_FOLLOW);
  HJ_TRY(query_gate(ctx, kFn));
  const hj::DeviceScene& sc = ctx->scene;
  const size_t ns = sc.ns, nq = sc.nq, nv = ctx->update.num_vertices;
  if (prev->num_spheres != ns || prev->num_quads != nq || prev->num_vertices != nv)
    return set_error(ctx, HJ_ERR_INVALID, "%s: %zu spheres, %zu quads, %zu vertices; the uploaded scene has %zu, %zu, %zu", kFn, prev->num_spheres,
                     prev->num_quads, prev->num_vertices, ns, nq, nv);
  if (!dev_shapes) {
    bool ok = true;
    if (prev->spheres)
      for (size_t i = 0; i < ns && ok; i++) ok = finite3(prev->spheres[i].center) && std::isfinite(prev->spheres[i].radius);
    if (prev->quads)
      for (size_t i = 0; i < nq && ok; i++) ok = finite3(prev->quads[i].origin) && finite3(prev->quads[i].edge1) && finite3(prev->quads[i].edge2);
    if (prev->vertices)
      for (size_t i = 0; i < nv && ok; i++) ok = finite3(prev->vertices[i].pos);
    if (!ok) return set_error(ctx, HJ_ERR_INVALID, "%s: a previous coordinate or radius is not finite", kFn);
  }
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  hj_context::Motion& q = ctx->motion;
  const size_t image_bytes = (size_t)width * height * HJ_MOTION_WORDS * sizeof(float);
  // every allocation before anything is enqueued
  struct Kind { const void* user; size_t bytes; DevBuf* stage; const void* uploaded; };
  const Kind kinds[3] = {{prev->spheres, ns * sizeof(hj_sphere), &q.spheres, sc.spheres},
                         {prev->quads, nq * sizeof(hj_quad), &q.quads, sc.quads},
                         {prev->vertices, nv * sizeof(hj_vertex), &q.vertices, sc.vertices}};
  const void* d_kind[3];
  for (int k = 0; k < 3; k++) {
    d_kind[k] = kinds[k].user && kinds[k].bytes ? kinds[k].user : kinds[k].uploaded;   // (NULL: the kind did not move)
    if (dev_shapes || !kinds[k].user || !kinds[k].bytes) continue;
    HJ_TRY(dev_alloc(ctx, *kinds[k].stage, kinds[k].bytes));
    d_kind[k] = kinds[k].stage->p;
  }
  float4* d_motion = reinterpret_cast<float4*>(motion);
  if (!dev_out) {
    HJ_TRY(dev_alloc(ctx, q.image, image_bytes));
    d_motion = static_cast<float4*>(q.image.p);
  }
  if (max_follow != 0) HJ_TRY(motion_follow_reserve(ctx, (size_t)width * height));
  hipStream_t s = ctx->stream;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; k++)
    if (!dev_shapes && kinds[k].user && kinds[k].bytes) e = hipMemcpyAsync(kinds[k].stage->p, kinds[k].user, kinds[k].bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    const uint32_t n = hj::mv_entries(width, height, sc.group_tile);
    const uint32_t wg_rays = walk_wg_rays(ctx, n);                   // entries per workgroup: hj_trace_rays' rule
    const dim3 grid((n + wg_rays - 1u) / wg_rays), blk(hj::kBlockThreads);
    if (sc.has_pairs != 0) hipLaunchKernelGGL(hj::k_mv_walk<true>, grid, blk, 0, s, sc, width, height, n, wg_rays, d_motion);
    else hipLaunchKernelGGL(hj::k_mv_walk<false>, grid, blk, 0, s, sc, width, height, n, wg_rays, d_motion);
    e = hipGetLastError();
  }
  bool followed = false;
  if (e == hipSuccess && max_follow != 0) e = motion_follow_rounds(ctx, width, height, d_motion, max_follow, followed);
  if (e == hipSuccess) {
    const hj::MvPrev p{static_cast<const float4*>(d_kind[0]), static_cast<const float4*>(d_kind[1]), static_cast<const float4*>(d_kind[2]),
                       hj::dt_host_camera(prev->camera)};
    if (followed) motion_follow_resolve(ctx, p, width, height, d_motion);
    else hipLaunchKernelGGL(hj::k_mv_resolve, per_lane(width * height), dim3(hj::kBlockThreads), 0, s, sc, p, width, height, d_motion);
    e = hipGetLastError();
  }
  if (e == hipSuccess && !dev_out) e = hipMemcpyAsync(motion, d_motion, image_bytes, hipMemcpyDeviceToHost, s);
  return drain(ctx, kFn, e);
}

}  // namespace hjapi

extern "C" {

int hj_render_motion(hj_context* ctx, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t flags, float* motion) {
  return motion_render(ctx, "hj_render_motion", prev, width, height, 0, flags, motion);
}

}  // extern "C"
