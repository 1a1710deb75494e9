// Probe-lit frames ("Probe-lit frames"; include/hijiki_hip.h hj_render_probe_lit): the frame a probe volume is for - every
// sample of hj_render_aovs_followed's chains lit at its last diffuse hit by the volume's look-up.  The functions a hit needs are the
// shade stage's - populate_*, camera_ray, env_radiance - and kernels/hj_aov.h's (aov_record, aov_pixel, aov_batch), included here and
// edited nowhere; the chain state is kernels/hj_follow.h's (kFollowLeft, two float4 a slot).  The look-up between the two kernels below
// is the volume's own kernel - k_pv_sample, k_pvv_sample or k_pp_sample -, launched by the unit that holds it: none of its text is
// here.  No global atomics, no inline assembly.
//   k_pl_points    one lane per sample slot of a walk launch: the slot's look-up point (p, n, 0, 0) and its side record (Le, kind)
//   k_pl_resolve   one lane per sample slot of a run of blocks: L = Le + (albedo * E) * (1 / pi) added to its pixel, the count beside it
// HJ_PROBE_LIT_NO_KERNELS (kernels/hj_direct_lit.h): the functions alone - pl_segment, pl_compose -; api/probe_lit.hip holds the kernels.
#pragma once
#define HJ_FOLLOW_NO_KERNELS   // the functions of hj_follow.h (and through it of hj_aov.h), no kernel of theirs
#include "hj_follow.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kPlDiffuse = 0u;    // side record word 3: the sample has a diffuse term, its point is the chain's last hit
constexpr uint32_t kPlNone = 1u;       // ... it has none: L is the side record's (Le) alone and its point the dummy below
constexpr uint32_t kPlNoSample = 2u;   // ... the slot holds no sample (outside its block or the image): the resolve never reads it
static_assert(kInvPi == 0.318309886f, "the compose multiplies by the shade stage's own 1 / pi, which has the contract's bits");

// The last segment (o, d) of slot smp's chain and its hit record -> false: the slot holds no sample.  state == nullptr: the launch took
// no follow round, so the segment is the camera ray itself (k_aov_resolve); else the chain state (k_aov_resolve_followed).
HJ_DEV bool pl_segment(const DeviceScene& sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks, const float4* __restrict__ state,
                       uint32_t smp, v3& o, v3& d) {
  const BatchState st = aov_batch(blocks, num_blocks);
  uint32_t rng_unused = 0;
  d = V(0.f, 0.f, 0.f);
  if (!camera_ray(st, sc, smp, rng_unused, d)) return false;
  o = V(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
  if (state) {
    o = xyz(state[2 * (size_t)smp]);
    d = xyz(state[2 * (size_t)smp + 1]);
  }
  return true;
}

// The radiance of a sample with a diffuse term (side record kPlDiffuse) whose chain's last segment (o, d) ended in hit record hr: the
// albedo is aov_record's at that hit, recomputed here; e: the look-up's record of the slot's point, E in words 0..2.
// L[c] = Le[c] + (albedo[c] * E[c]) * kInvPi, uncontracted, in that order.  ONE text for k_pl_resolve and kernels/hj_direct_lit.h's resolve.
HJ_DEV v3 pl_compose(const DeviceScene& sc, v3 o, v3 d, float4 hr, float4 sd, float4 e) {
  float4 r0, r1, r2;
  (void)aov_record(sc, o, d, hr, r0, r1, r2);
  return V(sd.x + (r0.x * e.x) * kInvPi, sd.y + (r0.y * e.y) * kInvPi, sd.z + (r0.z * e.z) * kInvPi);
}

#ifndef HJ_PROBE_LIT_NO_KERNELS

// points: two float4 per slot, the look-ups' own layout (position.xyz, normal.x | normal.yz, 0, 0); side: (Le.rgb, kind bits).
//   a hit on anything but a mirror or a dielectric: the populated hit point and shading normal aov_record builds its record from,
//     Le = the material's emission, kPlDiffuse
//   a mirror or a dielectric (the cap cut the chain there): Le = its emission, which eval_material has as 0; kPlNone
//   no hit - a camera miss, or kFollowLeft: the chain left a specular surface -: Le = the environment along d when one is uploaded,
//     else 0; kPlNone
// Every slot without a diffuse term gets the point (0, 0, 0 | 0, 0, 1): finite, with a normal the look-up can normalise.
__global__ __launch_bounds__(kBlockThreads) void k_pl_points(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                             const float4* __restrict__ hits, const float4* __restrict__ state,
                                                             float4* __restrict__ points, float4* __restrict__ side) {
  const uint32_t smp = blockIdx.x * blockDim.x + threadIdx.x;
  if (smp >= num_blocks * kSlotsPerBlock) return;
  float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = make_float4(0.f, 1.f, 0.f, 0.f);
  float4 sd = make_float4(0.f, 0.f, 0.f, __uint_as_float(kPlNoSample));
  v3 o, d;
  if (pl_segment(sc, blocks, num_blocks, state, smp, o, d)) {
    const float4 hr = hits[smp];
    const uint32_t id = __float_as_uint(hr.x);
    if (id >= sc.ns + sc.nq + sc.nt) {                              // (a miss, kFollowLeft, any other id outside the scene)
      const v3 le = sc.env_alias ? env_radiance(sc, d) : V(0.f, 0.f, 0.f);
      sd = make_float4(le.x, le.y, le.z, __uint_as_float(kPlNone));
    } else {
      const uint32_t tag = sc.materials[id] >> HJ_MATERIAL_TAG_SHIFT;
      const bool specular = tag == HJ_MAT_MIRROR || tag == HJ_MAT_DIELECTRIC;
      Its its;
      its.p = V(fmaf(hr.y, d.x, o.x), fmaf(hr.y, d.y, o.y), fmaf(hr.y, d.z, o.z));   // (aov_record's hit point, populated as it populates it)
      if (id < sc.ns) populate_sphere(sc.spheres[id], its);
      else if (id < sc.ns + sc.nq) populate_quad(sc, id - sc.ns, hr.z, hr.w, its);
      else populate_triangle(sc, id - sc.ns - sc.nq, hr.z, hr.w, its);
      v3 albedo, emission;
      uint32_t word;
      eval_material(sc, id, its.u, its.v, albedo, emission, word);
      sd = make_float4(emission.x, emission.y, emission.z, __uint_as_float(specular ? kPlNone : kPlDiffuse));
      if (!specular) {
        p0 = make_float4(its.p.x, its.p.y, its.p.z, its.n.x);
        p1 = make_float4(its.n.y, its.n.z, 0.f, 0.f);
      }
    }
  }
  points[2 * (size_t)smp] = p0;
  points[2 * (size_t)smp + 1] = p1;
  side[smp] = sd;
}

// A RUN, as k_aov_resolve has it: blocks [b0, b0 + nb) of the launch's list have pairwise disjoint pixels, so the read-add-write below
// races with nothing.  One lane per sample slot.  lookup: the look-up's record of the slot's point, E in words 0..2; L: pl_compose's.
// image: four floats a pixel, (sum of L.rgb, the count of samples); a pixel outside width x height is not written.
__global__ __launch_bounds__(kBlockThreads) void k_pl_resolve(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                              uint32_t b0, uint32_t nb, const float4* __restrict__ hits,
                                                              const float4* __restrict__ state, const float4* __restrict__ lookup,
                                                              const float4* __restrict__ side, uint32_t width, uint32_t height,
                                                              float4* __restrict__ image) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb * kSlotsPerBlock) return;
  const uint32_t smp = b0 * kSlotsPerBlock + j;
  v3 o, d;
  if (!pl_segment(sc, blocks, num_blocks, state, smp, o, d)) return;
  uint32_t px, py;
  if (!aov_pixel(blocks, smp, width, height, px, py)) return;
  const float4 sd = side[smp];
  v3 L = xyz(sd);
  if (__float_as_uint(sd.w) == kPlDiffuse) L = pl_compose(sc, o, d, hits[smp], sd, lookup[smp]);
  float4* p = image + ((size_t)py * width + px);
  float4 a = *p;
  a.x += L.x; a.y += L.y; a.z += L.z; a.w += 1.0f;
  *p = a;
}

#endif  // HJ_PROBE_LIT_NO_KERNELS

}  // namespace hj
