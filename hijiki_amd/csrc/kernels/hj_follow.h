// Followed AOVs and the specular continuation ("Followed AOVs"; include/hijiki_hip.h hj_follow_specular,
// hj_render_aovs_followed): what a mirror or glass SHOWS - the chain through specular surfaces that the path kernel takes, as a
// deterministic query.  The functions a hit needs are the shade stage's - populate_*, reflect3 - and kernels/hj_aov.h's (aov_record,
// eval_material behind it), included here and edited nowhere: this header adds the continuation (follow_continue, ONE text for the
// per-record query and the frame kernel) and the kernels around it.  No global atomics, no inline assembly of its own.
//   k_follow                 one lane per (ray, hit) record pair of hj_trace_rays: the continued ray, or the empty ray
//   k_af_scatter<FIRST>      the live chains of a walk launch's sample slots, in slot order, as a list; the first round's also sets
//                            every sample's chain state from its camera ray (kernels/hj_chain.h's chain_scatter, behind its count and scan)
//   k_aov_follow<PAIRS>      one round: the persistent walk over the list (hj_chain.h's chain_round), which leaves (kFollowLeft, n)
//                            in the record of a chain it continues
//   k_aov_resolve_followed   k_aov_resolve with the chain's last segment in place of the camera ray (aov_record: one text of the record)
// The chain state of a sample slot: hj_chain.h's.
#pragma once
#define HJ_AOV_NO_KERNELS   // the functions of hj_aov.h, no kernel of its: api/aov.hip holds those
#include "hj_aov.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kFollowLeft = 0xFFFFFFFEu;       // word 0 of a hit record whose chain left a specular surface and hit nothing:
                                                    // words 1..3 hold that surface's normal (no shape id: a miss to everything else)

// The ray (o, d) hit the scene at hr (objectID bits, t, u, v).  Does its chain go on, and with which ray?  Hit point and populate
// as stage_shade has them (hj_stages.h:506-510); the material word from the scene by id.  A mirror reflects about the stored normal;
// a dielectric takes the expressions of hj_stages.h:560-583 word for word, and in place of the random draw the branch the path kernel
// takes more often than not: reflect when k <= 0 or fr >= 0.5f, else refract (direction not normalised, as the reference leaves
// it).  Every other tag, a miss, an id outside the scene: false, nothing written.  -> p: the hit point, the next origin; wo: the next
// direction; n: the surface's shading normal; reflected: the continuation is a reflection (a mirror, a dielectric's reflect branch) and
// not a refraction - what the followed motion image (kernels/hj_motion_follow.h) multiplies its Householder matrices by
HJ_DEV bool follow_continue_branch(const DeviceScene& sc, v3 o, v3 d, float4 hr, v3& p, v3& wo, v3& n, bool& reflected) {
  const uint32_t id = __float_as_uint(hr.x);
  if (id >= sc.ns + sc.nq + sc.nt) return false;
  const uint32_t mat = sc.materials[id];
  const uint32_t tag = mat >> HJ_MATERIAL_TAG_SHIFT, midx = mat & HJ_MATERIAL_INDEX_MASK;
  if (tag != HJ_MAT_MIRROR && tag != HJ_MAT_DIELECTRIC) return false;
  Its its;
  its.p = V(fmaf(hr.y, d.x, o.x), fmaf(hr.y, d.y, o.y), fmaf(hr.y, d.z, o.z));   // scene.glsl:164
  if (id < sc.ns) populate_sphere(sc.spheres[id], its);
  else if (id < sc.ns + sc.nq) populate_quad(sc, id - sc.ns, hr.z, hr.w, its);
  else populate_triangle(sc, id - sc.ns - sc.nq, hr.z, hr.w, its);
  p = its.p;
  n = its.n;
  reflected = true;
  if (tag == HJ_MAT_MIRROR) {
    wo = reflect3(d, its.n);
    return true;
  }
  const float4 m = sc.dielectric[midx];                                            // material.glsl:50-87
  float eta = m.w;
  float etaInv = 1.0f / eta;
  float cosI = -dot3(its.n, d);
  v3 normal = its.n;
  if (cosI < 0.0f) { eta = etaInv; etaInv = 1.0f / eta; normal = -normal; cosI = -cosI; }
  const float k = 1.0f - (etaInv * etaInv) * (1.0f - cosI * cosI);
  bool reflect = k <= 0.0f;
  float cosO = 0.0f;
  if (!reflect) {
    cosO = __builtin_sqrtf(k);
    const float rpar = (eta * cosI - cosO) / (eta * cosI + cosO);
    const float rorth = (cosI - eta * cosO) / (cosI + eta * cosO);
    const float fr = 0.5f * (rpar * rpar + rorth * rorth);
    reflect = fr >= 0.5f;
  }
  if (reflect) {
    wo = reflect3(d, normal);
  } else {
    const v3 par = d - normal * dot3(d, normal);
    wo = par * etaInv - normal * cosO;
    reflected = false;
  }
  return true;
}
// ... for the callers that do not ask which branch
HJ_DEV bool follow_continue(const DeviceScene& sc, v3 o, v3 d, float4 hr, v3& p, v3& wo, v3& n) {
  bool reflected_unused = false;
  return follow_continue_branch(sc, o, d, hr, p, wo, n, reflected_unused);
}

// Is the chain of sample slot `slot` (< n) live: its last hit on a mirror or a dielectric, fewer than max_follow continuations taken?
// FIRST: behind the camera walk no state exists yet and no continuation has been taken.
template <bool FIRST>
HJ_DEV bool follow_live(const DeviceScene& sc, const float4* __restrict__ hits, const float4* __restrict__ state, uint32_t slot, uint32_t n,
                        uint32_t max_follow) {
  if (slot >= n) return false;
  const uint32_t id = __float_as_uint(hits[slot].x);
  if (id >= sc.ns + sc.nq + sc.nt) return false;                  // (a miss, kFollowLeft)
  const uint32_t tag = sc.materials[id] >> HJ_MATERIAL_TAG_SHIFT;
  if (tag != HJ_MAT_MIRROR && tag != HJ_MAT_DIELECTRIC) return false;
  return FIRST || __float_as_uint(state[2 * (size_t)slot + 1].w) < max_follow;
}

}  // namespace hj

#ifndef HJ_FOLLOW_NO_KERNELS   // (hj_chain.h, hj_motion_follow.h and hj_probe_lit.h take the functions above alone: api/follow.hip holds these kernels)
#include "hj_chain.h"

namespace hj {

static_assert(kSlotsPerBlock % kChainThreads == 0, "a launch's sample slots are whole tiles");

// rays: two float4 per record (origin.xyz, direction.x | direction.yz, tMin, tMax), hits: (objectID bits, t, u, v) - hj_trace_rays'
// arrays.  out: the continued ray (p, wo, tMin = eps, tMax = +inf: the next segment of a path), or where the chain ends the empty ray
// (zeros, tMin = +inf, tMax = -inf).
__global__ __launch_bounds__(kBlockThreads) void k_follow(DeviceScene sc, const float4* __restrict__ rays, const float4* __restrict__ hits, uint32_t n,
                                                          float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
  float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = make_float4(0.f, 0.f, kInf, -kInf);
  v3 p, wo, nrm;
  if (follow_continue(sc, V(a.x, a.y, a.z), V(a.w, b.x, b.y), hits[i], p, wo, nrm)) {
    o0 = make_float4(p.x, p.y, p.z, wo.x);
    o1 = make_float4(wo.y, wo.z, kEps, kInf);
  }
  out[2 * (size_t)i] = o0;
  out[2 * (size_t)i + 1] = o1;
}

// chain_scatter over a launch's n sample slots.  A slot's first ray is its camera ray (camera_ray says whether it has a sample).
template <bool FIRST>
__global__ __launch_bounds__(kChainThreads) void k_af_scatter(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                              const float4* __restrict__ hits, float4* __restrict__ state, uint32_t n, uint32_t max_follow,
                                                              const uint32_t* __restrict__ offsets, uint32_t* __restrict__ list) {
  chain_scatter<FIRST>(
      sc, hits, state, n, max_follow, offsets, list,
      [&](uint32_t slot, v3& o, v3& d) {
        const BatchState st = aov_batch(blocks, num_blocks);
        uint32_t rng_unused = 0;
        o = V(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
        return camera_ray(st, sc, slot, rng_unused, d);
      },
      [](uint32_t) {});
}

// chain_round over the live slots.  What a continuation leaves in the hit record: (kFollowLeft, n), the normal of the surface that
// was left, which k_aov_resolve_followed records should the new segment hit nothing.
template <bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_aov_follow(DeviceScene sc, const uint32_t* __restrict__ list, uint32_t count, uint32_t wg_rays,
                                                              float4* __restrict__ hits, float4* __restrict__ state) {
  chain_round<PAIRS>(sc, list, count, wg_rays, hits, state,
                     [](uint32_t, v3 nrm, bool) { return make_float4(__uint_as_float(kFollowLeft), nrm.x, nrm.y, nrm.z); });
}

// k_aov_resolve over a run whose launch was followed: the sample's record is the record of its chain's last hit - aov_record over
// the chain's last segment, the depth word the float32 sum of the chain's t values in chain order -, and for a chain that left a
// specular surface and hit nothing the record of that surface: albedo 1, its normal, the sum so far, hit 1.
__global__ __launch_bounds__(kBlockThreads) void k_aov_resolve_followed(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                                        uint32_t b0, uint32_t nb, const float4* __restrict__ hits,
                                                                        const float4* __restrict__ state, uint32_t width, uint32_t height,
                                                                        float4* __restrict__ aov) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb * kSlotsPerBlock) return;
  const uint32_t smp = b0 * kSlotsPerBlock + j;
  const BatchState st = aov_batch(blocks, num_blocks);
  uint32_t rng_unused = 0;
  v3 d = V(0.f, 0.f, 0.f);
  if (!camera_ray(st, sc, smp, rng_unused, d)) return;
  uint32_t px, py;
  if (!aov_pixel(blocks, smp, width, height, px, py)) return;
  const float4 hr = hits[smp], s0 = state[2 * (size_t)smp], s1 = state[2 * (size_t)smp + 1];
  float4 r0, r1, r2;
  if (__float_as_uint(hr.x) == kFollowLeft) {
    r0 = make_float4(1.f, 1.f, 1.f, 1.f);
    r1 = make_float4(hr.y, hr.z, hr.w, s0.w);
    r2 = make_float4(0.f, 0.f, 0.f, 1.f);
  } else if (aov_record(sc, xyz(s0), xyz(s1), hr, r0, r1, r2)) {
    r1.w = s0.w + hr.y;
  }
  aov_add(aov + 3 * ((size_t)py * width + px), r0, r1, r2);
}

}  // namespace hj

#endif  // HJ_FOLLOW_NO_KERNELS
