// Environment lighting (no counterpart upstream; include/hijiki_hip.h hj_environment): the radiance a ray that leaves the scene brings
// back, and the next-event sample of the environment.  One text for the shade stage (hj_stages.h) and the probes hj_debug_env_lookup /
// hj_debug_env_sample (api/environment.hip); DESIGN.md "Environment lighting" defines both.
#pragma once
#include "hj_device.h"
#include "hj_texture.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kEnvEmitter = 8u;   // the environment's emitter index: >= 8, so shadow_ray_proven_free never answers for it

// Le(d) = scale * texture_rgb(env, u, v): the sphere's lat-long convention (populate_sphere) with +y up; d need not be normalised.
HJ_DEV v3 env_radiance(const DeviceScene& sc, v3 d) {
  float u = 0.5f + hj_atan2(d.z, d.x) * (1.0f / kTwoPi);
  const float v = 0.5f + hj_atan2(d.y, __builtin_sqrtf(d.x * d.x + d.z * d.z)) * kInvPi;
  if (u != u) u = 0.0f;
  const v3 c = texture_rgb(sc.textures, sc.env_tex, u, v);
  return V(sc.env_scale[0] * c.x, sc.env_scale[1] * c.y, sc.env_scale[2] * c.z);
}

// A direction from the environment's distribution (api/environment.hip builds the alias table): draw `a` picks a column of the table,
// `coin` in [0, 1) keeps it or takes its alias (one gather), draw `b` places the direction uniformly in the cell's phi and sin(latitude)
// (16 bits each), so pdf = P(cell) / solid angle(cell) is constant in the cell.  Returns the unit direction; pdf excludes env_p.
HJ_DEV v3 env_sample(const DeviceScene& sc, float coin, uint32_t a, uint32_t b, float& pdf, uint32_t& cell) {
  const uint32_t W = sc.env_w, H = sc.env_h;
  const uint32_t i = (uint32_t)(((uint64_t)a * (uint64_t)(W * H)) >> 32);
  const float4 r = sc.env_alias[i];
  const bool take_alias = coin >= r.x;
  cell = take_alias ? __float_as_uint(r.y) : i;
  pdf = take_alias ? r.w : r.z;
  const uint32_t x = cell % W, y = cell / W;
  const float fu = ((float)(b >> 16) + 0.5f) * (1.0f / 65536.0f), fv = ((float)(b & 0xFFFFu) + 0.5f) * (1.0f / 65536.0f);
  float sp, cp, s0, c0, s1, c1;
  hj_sincos2pi(((float)x + fu) / (float)W - 0.5f, sp, cp);           // phi = 2 pi (u - 1/2)
  hj_sincos2pi((float)y / (float)(2u * H), s0, c0);                  // sin of the row's upper latitude: cos(pi y / H)
  hj_sincos2pi((float)(y + 1u) / (float)(2u * H), s1, c1);           // ... of its lower one
  const float ys = c1 + fv * (c0 - c1);
  const float rr = __builtin_sqrtf(f_max(0.0f, 1.0f - ys * ys));
  return V(rr * cp, ys, rr * sp);
}

}  // namespace hj
