// The followed motion image ("Followed motion"; include/hijiki_hip.h: hj_render_motion_followed): hj_render_motion's
// record for what a mirror or glass SHOWS - the chain the followed AOVs follow, for the pixel's centre ray, and at its end the
// displacement of the surface it reaches carried back through the chain's reflections onto the virtual point the temporal stage
// reprojects.  The rounds are kernels/hj_chain.h's (the continuation of kernels/hj_follow.h behind them), the first-hit record and the
// point on a shape are kernels/hj_motion.h's (mv_record, mv_shape_point, mv_project) - included here and edited nowhere; round 0 is
// api/motion.hip's k_mv_walk.  No global atomics, no inline assembly; loads and stores are the compiler's.
//   k_mf_scatter<FIRST>  the live pixels of the image in pixel order as a list; the first round's also sets every pixel's chain state
//                        from its centre ray (hj_chain.h's chain_scatter, behind its count and scan, which api/follow.hip holds)
//   k_mf_follow<PAIRS>   one round: the persistent walk over the list (hj_chain.h's chain_round), which multiplies M by a reflection's
//                        Householder matrix
//   k_mf_resolve         one lane per pixel, in place: mv_record for a pixel that took no continuation, the followed record otherwise
// The chain state of a pixel: hj_chain.h's two float4 in `state`, as the followed AOVs keep it, and three float4 in `mat`, the columns
// of M (word 3 unused).  mat is written when a pixel takes its first continuation and read for no other pixel.
#pragma once
#define HJ_MOTION_NO_KERNELS   // the functions of hj_motion.h, no kernel of its: api/motion.hip holds those
#include "hj_motion.h"
#define HJ_CHAIN_NO_KERNELS    // chain_scatter and chain_round, not the count and scan kernels: api/follow.hip holds those
#include "hj_chain.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kMvLeft = kFollowLeft;        // HJ_MOTION_LEFT: word 3 of a record whose chain left a specular surface and hit nothing;
                                                 // between the rounds word 0 of such a pixel's hit record (a miss to follow_live)

// M -> M - 2 (M n) n^T, columns m0, m1, m2: w = M n per row as (m0 * n.x + m1 * n.y) + m2 * n.z, w2 = 2 * w, column j less w2 * n.j
HJ_DEV void mf_householder(v3& m0, v3& m1, v3& m2, v3 n) {
  const v3 w = V((m0.x * n.x + m1.x * n.y) + m2.x * n.z, (m0.y * n.x + m1.y * n.y) + m2.y * n.z, (m0.z * n.x + m1.z * n.y) + m2.z * n.z);
  const v3 w2 = V(2.0f * w.x, 2.0f * w.y, 2.0f * w.z);
  m0 = V(m0.x - w2.x * n.x, m0.y - w2.y * n.x, m0.z - w2.z * n.x);
  m1 = V(m1.x - w2.x * n.y, m1.y - w2.y * n.y, m1.z - w2.z * n.y);
  m2 = V(m2.x - w2.x * n.z, m2.y - w2.y * n.z, m2.z - w2.z * n.z);
}

// chain_scatter over the image's n = W * H pixels.  A pixel's first ray is its centre ray; a listed pixel also gets M = the identity.
template <bool FIRST>
__global__ __launch_bounds__(kChainThreads) void k_mf_scatter(DeviceScene sc, uint32_t W, uint32_t H, const float4* __restrict__ hits, float4* __restrict__ state,
                                                              float4* __restrict__ mat, uint32_t n, uint32_t max_follow, const uint32_t* __restrict__ offsets,
                                                              uint32_t* __restrict__ list) {
  chain_scatter<FIRST>(
      sc, hits, state, n, max_follow, offsets, list,
      [&](uint32_t t, v3& o, v3& d) {
        const DtCamera cam = mv_camera(sc);
        d = dt_camera_dir(cam, (float)(t % W) + 0.5f, (float)(t / W) + 0.5f, (float)W, (float)H);
        o = cam.pos;
        return true;
      },
      [&](uint32_t t) {
        mat[3 * (size_t)t] = make_float4(1.f, 0.f, 0.f, 0.f);
        mat[3 * (size_t)t + 1] = make_float4(0.f, 1.f, 0.f, 0.f);
        mat[3 * (size_t)t + 2] = make_float4(0.f, 0.f, 1.f, 0.f);
      });
}

// chain_round over the live pixels.  A reflection multiplies M by its Householder matrix - M is read and written inside the reflect
// branch alone and is dead before the ray enters the walk -, and what a continuation leaves in the hit record is (kMvLeft, 0, 0, 0):
// what the resolve reads should the new segment hit nothing.
template <bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_mf_follow(DeviceScene sc, const uint32_t* __restrict__ list, uint32_t count, uint32_t wg_rays,
                                                             float4* __restrict__ hits, float4* __restrict__ state, float4* __restrict__ mat) {
  chain_round<PAIRS>(sc, list, count, wg_rays, hits, state, [&](uint32_t slot, v3 nrm, bool reflected) {
    if (reflected) {
      float4* __restrict__ m = mat + 3 * (size_t)slot;
      v3 m0 = xyz(m[0]), m1 = xyz(m[1]), m2 = xyz(m[2]);
      mf_householder(m0, m1, m2, nrm);
      m[0] = make_float4(m0.x, m0.y, m0.z, 0.f);
      m[1] = make_float4(m1.x, m1.y, m1.z, 0.f);
      m[2] = make_float4(m2.x, m2.y, m2.z, 0.f);
    }
    return make_float4(__uint_as_float(kMvLeft), 0.f, 0.f, 0.f);
  });
}

// One lane per pixel t = y * W + x, in place: motion[t] holds the chain's last raw hit - or kMvLeft - on entry and the pixel's record
// on return.  A pixel that took no continuation: mv_record, hj_render_motion's own text.  Otherwise the contract's arithmetic
// (include/hijiki_hip.h, hj_render_motion_followed), operation for operation, one rounding each, uncontracted, except what mv_record
// excepts.  now: the uploaded shape arrays in MvPrev's form (its camera is not read).
__global__ __launch_bounds__(kBlockThreads) void k_mf_resolve(DeviceScene sc, MvPrev now, MvPrev prev, uint32_t W, uint32_t H, const float4* __restrict__ state,
                                                              const float4* __restrict__ mat, float4* __restrict__ motion) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * H) return;
  const float4 hr = motion[t];
  const float4 s0 = state[2 * (size_t)t], s1 = state[2 * (size_t)t + 1];
  if (__float_as_uint(s1.w) == 0u) {
    motion[t] = mv_record(sc, prev, t, W, H, hr);
    return;
  }
  const uint32_t id = __float_as_uint(hr.x);
  const bool left = id >= sc.ns + sc.nq + sc.nt;                  // (kMvLeft: a continued pixel's record is a hit or that)
  const DtCamera cam = mv_camera(sc);
  const v3 d0 = dt_camera_dir(cam, (float)(t % W) + 0.5f, (float)(t / W) + 0.5f, (float)W, (float)H);
  const float D = left ? s0.w : s0.w + hr.y;
  v3 Pv = V(cam.pos.x + D * d0.x, cam.pos.y + D * d0.y, cam.pos.z + D * d0.z);
  if (!left) {
    v3 n = V(0.f, 0.f, 0.f);
    if (id < sc.ns) n = mv_sphere_normal(sc, id, V(fmaf(hr.y, s1.x, s0.x), fmaf(hr.y, s1.y, s0.y), fmaf(hr.y, s1.z, s0.z)));
    const v3 Xn = mv_shape_point(sc, now.spheres, now.quads, now.vertices, id, n, hr.z, hr.w);
    const v3 Xp = mv_shape_point(sc, prev.spheres, prev.quads, prev.vertices, id, n, hr.z, hr.w);
    const v3 dl = V(Xp.x - Xn.x, Xp.y - Xn.y, Xp.z - Xn.z);
    const float4 m0 = mat[3 * (size_t)t], m1 = mat[3 * (size_t)t + 1], m2 = mat[3 * (size_t)t + 2];
    Pv = V(Pv.x + ((m0.x * dl.x + m1.x * dl.y) + m2.x * dl.z), Pv.y + ((m0.y * dl.x + m1.y * dl.y) + m2.y * dl.z),
           Pv.z + ((m0.z * dl.x + m1.z * dl.y) + m2.z * dl.z));
  }
  motion[t] = mv_project(prev.cam, Pv, W, H, left ? kMvLeft : id);
}

}  // namespace hj
