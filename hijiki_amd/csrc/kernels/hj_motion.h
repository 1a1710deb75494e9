// Per-pixel motion for the temporal denoiser ("Motion for the temporal denoiser"; include/hijiki_hip.h: hj_render_motion):
// for every pixel where the surface point its centre ray sees was in the previous frame, as a position in the previous image and a
// distance from the previous camera.  The walk is the path kernel's behind walk_segment (hj_walk_segment.h), the centre ray's direction is the
// temporal stage's (dt_camera_dir, hj_denoise_temporal.h), the sphere normal is populate_sphere's divs (hj_shade.h) - included here
// and edited nowhere.  No global atomics, no inline assembly of its own; loads and stores are the compiler's.
//   k_mv_walk<PAIRS>   the persistent walk over the image's pixels, a wave's 64 rays together in the image; the raw hit
//                      (id bits, t, u, v) goes into the pixel's own record of `motion`: no ray array and no hit array exist
//   k_mv_resolve       one lane per pixel: the raw hit read back, the previous point from the previous shape arrays, its projection
//                      into the previous camera, the record overwritten in place
// The previous-point arithmetic stays out of the walk's finish: inside it it would take the walk's registers.
#pragma once
#include "hj_walk_segment.h"
#define HJ_DENOISE_TEMPORAL_NO_KERNELS   // dt_camera_dir, dt_rotate, dn_sq and the accumulate template; the temporal unit's kernels stay its own
#include "hj_denoise_temporal.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kMvNone = 0xFFFFFFFFu;   // HJ_MOTION_NONE: word 3 of a record without a previous position
constexpr uint32_t kMvPad = 0xFFFFFFFFu;    // the slot of a walk entry beyond the image (no pixel has this index: at most 2^28)

// The previous frame as k_mv_resolve reads it: shape arrays with the uploaded scene's counts, and the camera
struct MvPrev {
  const float4* spheres;        // hj_sphere
  const float4* quads;          // hj_quad as 3 x float4
  const float4* vertices;       // hj_vertex as 2 x float4 (pos.xyz, u | normal.xyz, v)
  DtCamera cam;
};

// the uploaded scene's camera as dt_camera_dir takes it
HJ_DEV DtCamera mv_camera(const DeviceScene& sc) {
  return DtCamera{V(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]),
                  V(sc.camera.rotation[0], sc.camera.rotation[1], sc.camera.rotation[2]), sc.camera.rotation[3], sc.tan_half_fov};
}

// Walk entries of a W x H image: 64-entry groups, a group either an 8 x 8 pixel tile (tile != 0: DeviceScene::group_tile, as the
// camera packets over a large tree) or a run of 64 pixels of a row; groups in raster order of tiles / runs.  The image is padded to
// whole groups, so every pixel is exactly one entry: a bijection between the pixels and the entries that are no padding.
__host__ __device__ inline uint32_t mv_entries(uint32_t W, uint32_t H, uint32_t tile) {
  return tile != 0u ? ((W + 7u) >> 3) * ((H + 7u) >> 3) * 64u : ((W + 63u) >> 6) * H * 64u;
}
// ... entry q's pixel; false: padding
HJ_DEV bool mv_pixel(uint32_t q, uint32_t W, uint32_t H, uint32_t tile, uint32_t& x, uint32_t& y) {
  const uint32_t grp = q >> 6, lane = q & 63u;
  if (tile != 0u) {
    const uint32_t across = (W + 7u) >> 3;
    x = ((grp % across) << 3) | (lane & 7u);
    y = ((grp / across) << 3) | (lane >> 3);
  } else {
    const uint32_t across = (W + 63u) >> 6;
    x = ((grp % across) << 6) | lane;
    y = grp / across;
  }
  return x < W && y < H;
}

// The contract's arithmetic (include/hijiki_hip.h, hj_render_motion), operation for operation - one rounding each, uncontracted, except
// dt_camera_dir, dt_rotate and divs, which are the numeric contract's, and the hit point's fmaf - as ONE text for k_mv_resolve and for
// the followed resolve (kernels/hj_motion_follow.h), whose pixels without a continuation take mv_record as it stands.
// ... the sphere normal at the hit point P of sphere id of the uploaded scene: populate_sphere's
HJ_DEV v3 mv_sphere_normal(const DeviceScene& sc, uint32_t id, v3 P) {
  const float4 sp = sc.spheres[id];
  return divs(P - xyz(sp), sp.w);
}
// ... the point of shape id (< shapes) on the shape arrays given: a sphere's at the normal n, a quad's and a triangle's at (u, v); the
// index triple is the uploaded one
HJ_DEV v3 mv_shape_point(const DeviceScene& sc, const float4* __restrict__ spheres, const float4* __restrict__ quads, const float4* __restrict__ vertices,
                         uint32_t id, v3 n, float u, float v) {
  if (id < sc.ns) {
    const float4 pp = spheres[id];
    return V(pp.x + n.x * pp.w, pp.y + n.y * pp.w, pp.z + n.z * pp.w);
  }
  if (id < sc.ns + sc.nq) {
    const float4* __restrict__ q = quads + 3 * (size_t)(id - sc.ns);
    const float4 o = q[0], e1 = q[1], e2 = q[2];
    return V((o.x + e1.x * u) + e2.x * v, (o.y + e1.y * u) + e2.y * v, (o.z + e1.z * u) + e2.z * v);
  }
  const hj_triangle tri = sc.triangles[id - sc.ns - sc.nq];
  const float4 a = vertices[2 * (size_t)tri.v[0]], b = vertices[2 * (size_t)tri.v[1]], c = vertices[2 * (size_t)tri.v[2]];
  const float l0 = (1.0f - u) - v;
  return V((a.x * l0 + b.x * u) + c.x * v, (a.y * l0 + b.y * u) + c.y * v, (a.z * l0 + b.z * u) + c.z * v);
}
// ... PROJECTION of the point Pp into the previous camera -> the record, its word 3 `word`; (0, 0, 0, HJ_MOTION_NONE) behind the camera
HJ_DEV float4 mv_project(const DtCamera& pc, v3 Pp, uint32_t W, uint32_t H, uint32_t word) {
  const v3 vv = Pp - pc.pos;
  const v3 c = dt_rotate(vv, -pc.qv, pc.qw);
  if (!(c.z < 0.0f)) return make_float4(0.f, 0.f, 0.f, __uint_as_float(kMvNone));
  const float Wf = (float)W, Hf = (float)H;
  const float k = (0.5f * Wf) / pc.tan_half;
  const float sx = (c.x / -c.z) * k + 0.5f * Wf, sy = (-c.y / -c.z) * k + 0.5f * Hf;
  return make_float4(sx, sy, __builtin_sqrtf(dn_sq(vv)), __uint_as_float(word));
}
// ... hj_render_motion's record of pixel t = y * W + x whose centre ray's raw hit is hr
HJ_DEV float4 mv_record(const DeviceScene& sc, const MvPrev& prev, uint32_t t, uint32_t W, uint32_t H, float4 hr) {
  const uint32_t id = __float_as_uint(hr.x);
  if (id >= sc.ns + sc.nq + sc.nt) return make_float4(0.f, 0.f, 0.f, __uint_as_float(kMvNone));   // (a miss is 0xFFFFFFFF; any other id outside the scene is one too)
  v3 n = V(0.f, 0.f, 0.f);
  if (id < sc.ns) {
    const uint32_t x = t % W, y = t / W;
    const DtCamera cam = mv_camera(sc);
    const v3 d = dt_camera_dir(cam, (float)x + 0.5f, (float)y + 0.5f, (float)W, (float)H);
    n = mv_sphere_normal(sc, id, V(fmaf(hr.y, d.x, cam.pos.x), fmaf(hr.y, d.y, cam.pos.y), fmaf(hr.y, d.z, cam.pos.z)));   // scene.glsl:164
  }
  return mv_project(prev.cam, mv_shape_point(sc, prev.spheres, prev.quads, prev.vertices, id, n, hr.z, hr.w), W, H, id);
}

#ifndef HJ_MOTION_NO_KERNELS   // (kernels/hj_motion_follow.h takes the functions above alone: api/motion.hip holds these kernels)

// Entries [0, n = mv_entries) of the image.  Workgroup g walks entries [g * wg_rays, ...) (walk_segment).  An entry's ray is
// built from its pixel - origin = the uploaded camera's position, d = dt_camera_dir through (x + 0.5, y + 0.5), tMin = eps, tMax =
// +inf - and its raw hit (objectID bits, t, u, v; a miss: (-1, 0, 0, 0)) goes to motion[y * W + x]: which lane or workgroup
// carried a pixel, and which grouping, shows in no record.  A padding entry is fetched as a ray with the empty range [+inf, -inf]:
// it fails every box and shape test, leaves the tree at the first node and writes nothing.
template <bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_mv_walk(DeviceScene sc, uint32_t W, uint32_t H, uint32_t n, uint32_t wg_rays,
                                                           float4* __restrict__ motion) {
  const DtCamera cam = mv_camera(sc);
  const float Wf = (float)W, Hf = (float)H;
  auto fetch = [&](uint32_t q, uint32_t& slot, Ray& r, bool& any, RawHit& h) {
    uint32_t x, y;
    const bool valid = mv_pixel(q, W, H, sc.group_tile, x, y);
    slot = valid ? y * W + x : kMvPad;
    any = false;
    r.o = cam.pos;
    r.d = valid ? dt_camera_dir(cam, (float)x + 0.5f, (float)y + 0.5f, Wf, Hf) : V(0.f, 0.f, 0.f);
    walk_empty_range(r, valid);
    walk_reset(h);
  };
  auto finish = [&](bool done, uint32_t slot, const RawHit& h, bool) {
    if (done && slot != kMvPad) motion[slot] = walk_hit_record(h);
  };
  walk_segment<0, PAIRS>(sc, n, wg_rays, fetch, finish);
}

// One lane per pixel t = y * W + x, in place: motion[t] holds the walk's raw hit on entry and the pixel's record on return, so a
// lane touches its own record alone.  The record: mv_record above.
__global__ __launch_bounds__(kBlockThreads) void k_mv_resolve(DeviceScene sc, MvPrev prev, uint32_t W, uint32_t H, float4* __restrict__ motion) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * H) return;
  motion[t] = mv_record(sc, prev, t, W, H, motion[t]);
}

#endif  // HJ_MOTION_NO_KERNELS

}  // namespace hj
