// Image textures (no counterpart upstream; include/hijiki_hip.h hj_texture): the colour of a HJ_MAT_DIFFUSE_TEXTURED hit.  One text for
// the shade stage (hj_stages.h) and the probe hj_debug_texture_lookup (api/texture.hip); DESIGN.md "Image textures" defines it.
#pragma once
#include "../../../include/hijiki_hip.h"
#include "hj_num.h"

#pragma clang fp contract(off)

namespace hj {

// DeviceScene::textures: one 16-byte record per texture, then the texels (float4 each).  Record t = (width, height, filter, index
// of its first texel counted in float4 from the START of the buffer) as uint32 bits - so one pointer serves both.
HJ_DEV float4 texel(const float4* __restrict__ tex, uint32_t first, uint32_t W, uint32_t x, uint32_t y) {
  return tex[(size_t)first + (size_t)y * W + x];
}
HJ_DEV int32_t wrap_index(int32_t i, int32_t n) { return i < 0 ? i + n : (i >= n ? i - n : i); }   // i in [-n, 2n)

HJ_DEV v3 texture_rgb(const float4* __restrict__ tex, uint32_t t, float u, float v) {
  const float4 r = tex[t];
  const uint32_t W = __float_as_uint(r.x), H = __float_as_uint(r.y), filter = __float_as_uint(r.z), first = __float_as_uint(r.w);
  float s = u - __builtin_floorf(u), q = v - __builtin_floorf(v);        // repeat; s or q may round to 1.0
  if (!__builtin_isfinite(s)) s = 0.0f;
  if (!__builtin_isfinite(q)) q = 0.0f;
  const float fW = (float)W, fH = (float)H;
  if (filter == HJ_TEX_NEAREST) {
    const uint32_t x = (uint32_t)(int32_t)(s * fW), y = (uint32_t)(int32_t)((1.0f - q) * fH);   // (W, H <= 2^24: hj_scene_upload_textured)
    return xyz(texel(tex, first, W, x < W - 1u ? x : W - 1u, y < H - 1u ? y : H - 1u));
  }
  const float fx = s * fW - 0.5f, fy = (1.0f - q) * fH - 0.5f;
  const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
  const float ax = fx - x0f, ay = fy - y0f;
  const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
  const uint32_t xa = (uint32_t)wrap_index(x0, (int32_t)W), xb = (uint32_t)wrap_index(x0 + 1, (int32_t)W);
  const uint32_t ya = (uint32_t)wrap_index(y0, (int32_t)H), yb = (uint32_t)wrap_index(y0 + 1, (int32_t)H);
  const v3 c00 = xyz(texel(tex, first, W, xa, ya)), c10 = xyz(texel(tex, first, W, xb, ya));
  const v3 c01 = xyz(texel(tex, first, W, xa, yb)), c11 = xyz(texel(tex, first, W, xb, yb));
  const float bx = 1.0f - ax, by = 1.0f - ay;
  return (c00 * bx + c10 * ax) * by + (c01 * bx + c11 * ax) * ay;
}

}  // namespace hj
