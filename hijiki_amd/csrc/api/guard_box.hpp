// The leaf guards' boxes on the device: ONE text for the upload's re-layout on the device (scene_relayout.hip, k_rl_guard_build) and
// for hj_scene_update_shapes (scene_update.hip, k_su_scatter) - api/scene_upload.hip's host formula, operation for operation.
#pragma once
#include "hj_internal.h"
#include "refit_pass.hpp"

namespace hjapi {

__device__ inline bool su_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// std::nextafter towards -inf / +inf as a step on the bit pattern (x is not NaN)
__device__ inline float su_next_down(float x) {
  const uint32_t u = __float_as_uint(x);
  if (u == 0xFF800000u) return x;                              // -inf stays
  if ((u << 1) == 0u) return __uint_as_float(0x80000001u);     // +-0 -> the smallest negative number
  return __uint_as_float((u >> 31) ? u + 1u : u - 1u);
}
__device__ inline float su_next_up(float x) {
  const uint32_t u = __float_as_uint(x);
  if (u == 0x7F800000u) return x;
  if ((u << 1) == 0u) return __uint_as_float(0x00000001u);
  return __uint_as_float((u >> 31) ? u - 1u : u + 1u);
}
__device__ inline float su_min(float a, float b) { return b < a ? b : a; }    // std::min / std::max as the host evaluates them
__device__ inline float su_max(float a, float b) { return a < b ? b : a; }

// The guard box of leaf shape `sh` (api/scene_upload.hip "Guard nodes for single leaves": the shape's own bounds, padded by a thousandth
// of its size plus pad_abs, one step outward) - the same float operations in the same order.
__device__ inline void su_guard_box(const RefitShapes& s, uint32_t sh, float pad_abs, float gmin[3], float gmax[3]) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, size = 0.f;
  auto grow = [&](float x, float y, float z) {
    const float p[3] = {x, y, z};
    for (int k = 0; k < 3; k++) { lo[k] = su_min(lo[k], p[k]); hi[k] = su_max(hi[k], p[k]); }
  };
  if (sh < s.ns) {
    const float4 sp = s.spheres[sh];
    const float r = fabsf(sp.w);
    grow(sp.x - r, sp.y - r, sp.z - r); grow(sp.x + r, sp.y + r, sp.z + r);
    size = r;
  } else if (sh < s.ns + s.nq) {
    const uint32_t q = sh - s.ns;
    const float4 o = s.quads[3 * q], e1 = s.quads[3 * q + 1], e2 = s.quads[3 * q + 2];
    for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) {
      const float fa = (float)a, fb = (float)b;
      grow(o.x + fa * e1.x + fb * e2.x, o.y + fa * e1.y + fb * e2.y, o.z + fa * e1.z + fb * e2.z);
    }
  } else {
    const hj_triangle t = s.triangles[sh - s.ns - s.nq];
    for (int c = 0; c < 3; c++) { const hj_vertex v = s.vertices[t.v[c]]; grow(v.pos[0], v.pos[1], v.pos[2]); }
  }
  for (int k = 0; k < 3; k++) size = su_max(size, hi[k] - lo[k]);
  const float pad = size * 1e-3f + pad_abs;
  bool ok = su_finite(pad);
  for (int k = 0; k < 3; k++) {
    gmin[k] = su_next_down(lo[k] - pad);
    gmax[k] = su_next_up(hi[k] + pad);
    ok = ok && gmin[k] <= gmax[k];
  }
  if (!ok) for (int k = 0; k < 3; k++) { gmin[k] = -INFINITY; gmax[k] = INFINITY; }
}

// The absolute part of the padding (api/scene_upload.hip): 2e-4, or 4e-6 of the extent of the root box joined with the camera
__host__ __device__ inline float guard_pad_abs(const float rlo[3], const float rhi[3], const float cam[3]) {
  float pad_abs = 2e-4f, ext = 0.f;
  for (int k = 0; k < 3; k++) {
    const float a = cam[k] < rlo[k] ? cam[k] : rlo[k], b = rhi[k] < cam[k] ? cam[k] : rhi[k];     // std::min / std::max as the host evaluates them
    if (b - a == b - a) ext = ext < b - a ? b - a : ext;
  }
  if ((__builtin_bit_cast(uint32_t, ext) & 0x7F800000u) != 0x7F800000u) pad_abs = pad_abs < 4e-6f * ext ? 4e-6f * ext : pad_abs;
  return pad_abs;
}

}  // namespace hjapi
