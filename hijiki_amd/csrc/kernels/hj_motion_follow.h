// The followed motion image ("Followed motion"; include/hijiki_hip.h: hj_render_motion_followed): hj_render_motion's
// record for what a mirror or glass SHOWS - the chain the followed AOVs follow, for the pixel's centre ray, and at its end the
// displacement of the surface it reaches carried back through the chain's reflections onto the virtual point the temporal stage
// reprojects.  The continuation is kernels/hj_follow.h's (follow_continue_branch, follow_live), the first-hit record and the point on
// a shape are kernels/hj_motion.h's (mv_record, mv_shape_point, mv_project), the compaction is kernels/hj_compact.h's - included here
// and edited nowhere; round 0 is api/motion.hip's k_mv_walk.  No global atomics, no inline assembly; loads and stores are the compiler's.
//   k_mf_count / _scan / _scatter   the live pixels of the image in pixel order as a list; the first round's scatter also sets every
//                        pixel's chain state from its centre ray
//   k_mf_follow<PAIRS>   one round: the persistent walk over the list with a fetch that continues a chain from its state and last hit,
//                        stores the new segment and multiplies M by the reflection's Householder matrix; a finish that stores the hit
//   k_mf_resolve         one lane per pixel, in place: mv_record for a pixel that took no continuation, the followed record otherwise
// The chain state of a pixel: two float4 in `state` - (segment origin.xyz, depth so far) (segment direction.xyz, continuations taken
// as bits), as the followed AOVs keep it - and three float4 in `mat`, the columns of M (word 3 unused).  mat is written when a pixel
// takes its first continuation and read for no other pixel.
#pragma once
#define HJ_MOTION_NO_KERNELS   // the functions of hj_motion.h, no kernel of its: api/motion.hip holds those
#include "hj_motion.h"
#define HJ_FOLLOW_NO_KERNELS   // follow_continue_branch and follow_live, no kernel of hj_follow.h's: api/follow.hip holds those
#include "hj_follow.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kMfThreads = 256u;            // threads of a k_mf_count / _scan / _scatter workgroup: a compaction tile
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

// The live pixels of the image's n = W * H in ascending order -> list.  Tiles of kMfThreads pixels; counts: a word per tile and the
// total behind them (the host reads it: it sizes the round's grid).  FIRST: behind k_mv_walk no state exists yet.
template <bool FIRST>
__global__ __launch_bounds__(kMfThreads) void k_mf_count(DeviceScene sc, const float4* __restrict__ hits, const float4* __restrict__ state, uint32_t n,
                                                         uint32_t max_follow, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kMfThreads / 64u];
  (void)compact_wave_counts(follow_live<FIRST>(sc, hits, state, blockIdx.x * kMfThreads + threadIdx.x, n, max_follow), wave_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = compact_tile_count<kMfThreads>(wave_cnt);
}

__global__ __launch_bounds__(kMfThreads) void k_mf_scan(uint32_t* __restrict__ counts, uint32_t nb) { compact_scan_tiles<kMfThreads>(counts, nb); }

// FIRST: every pixel also gets its chain state - the centre ray, depth 0, no continuation -, so the resolve reads one kind of record
// for every pixel; a listed pixel also gets M = the identity.
template <bool FIRST>
__global__ __launch_bounds__(kMfThreads) void k_mf_scatter(DeviceScene sc, uint32_t W, uint32_t H, const float4* __restrict__ hits, float4* __restrict__ state,
                                                           float4* __restrict__ mat, uint32_t n, uint32_t max_follow, const uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ list) {
  __shared__ uint32_t wave_cnt[kMfThreads / 64u];
  const uint32_t t = blockIdx.x * kMfThreads + threadIdx.x;
  if (FIRST && t < n) {
    const DtCamera cam = mv_camera(sc);
    const v3 d = dt_camera_dir(cam, (float)(t % W) + 0.5f, (float)(t / W) + 0.5f, (float)W, (float)H);
    state[2 * (size_t)t] = make_float4(cam.pos.x, cam.pos.y, cam.pos.z, 0.f);
    state[2 * (size_t)t + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(0u));
  }
  const bool keep = follow_live<FIRST>(sc, hits, state, t, n, max_follow);
  const unsigned long long mask = compact_wave_counts(keep, wave_cnt);
  if (!keep) return;
  if (FIRST) {
    mat[3 * (size_t)t] = make_float4(1.f, 0.f, 0.f, 0.f);
    mat[3 * (size_t)t + 1] = make_float4(0.f, 1.f, 0.f, 0.f);
    mat[3 * (size_t)t + 2] = make_float4(0.f, 0.f, 1.f, 0.f);
  }
  HJ_COMPACT_RANK(pos, offsets[blockIdx.x], wave_cnt, mask);
  list[pos] = t;
}

// One round over the `count` live pixels of list.  Workgroup g walks list entries [g * wg_rays, ...) as k_mv_walk walks its entries.
// fetch: the chain's state and last hit -> follow_continue_branch -> the walk's ray (p, wo, eps, +inf); the state becomes the new
// segment's (p, depth + t | wo, continuations + 1), a reflection multiplies M by its Householder matrix, and the hit record becomes
// (kMvLeft, 0, 0, 0) - what the resolve reads should the new segment hit nothing.  The walk's finish hook sees the hit and not the
// ray, so the segment is stored here, in the service phase, where the walk issues its stores anyway; M is read and written inside the
// reflect branch alone and is dead before the ray enters the walk.  finish: a hit replaces the record; a miss leaves it.  A pixel is
// in the list once, so one lane reads and writes its records; which lane or workgroup carried a chain shows in no result.
template <bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_mf_follow(DeviceScene sc, const uint32_t* __restrict__ list, uint32_t count, uint32_t wg_rays,
                                                             float4* __restrict__ hits, float4* __restrict__ state, float4* __restrict__ mat) {
  __shared__ WgShared sh;
  const uint32_t first = blockIdx.x * wg_rays;                    // (the grid is ceil(count / wg_rays): first < count)
  const uint32_t cnt = count - first < wg_rays ? count - first : wg_rays;
  if (threadIdx.x == 0) sh.head = 0;
  load_hot_nodes(sc, sh);
  __syncthreads();
  auto fetch = [&](uint32_t i, uint32_t& slot, Ray& r, bool& any, RawHit& h) {
    slot = list[first + i];
    any = false;
    const float4 s0 = state[2 * (size_t)slot], s1 = state[2 * (size_t)slot + 1];
    const float4 hr = hits[slot];
    v3 p = V(0.f, 0.f, 0.f), wo = p, nrm = p;
    bool reflected = false;
    const bool go = follow_continue_branch(sc, xyz(s0), xyz(s1), hr, p, wo, nrm, reflected);   // (true for every entry the scatter listed)
    r.o = p;
    r.d = wo;
    r.tmin = go ? kEps : kInf;                                     // render.glsl:33
    r.tmax = go ? kInf : -kInf;
    if (go) {
      state[2 * (size_t)slot] = make_float4(p.x, p.y, p.z, s0.w + hr.y);
      state[2 * (size_t)slot + 1] = make_float4(wo.x, wo.y, wo.z, __uint_as_float(__float_as_uint(s1.w) + 1u));
      hits[slot] = make_float4(__uint_as_float(kMvLeft), 0.f, 0.f, 0.f);
      if (reflected) {
        float4* __restrict__ m = mat + 3 * (size_t)slot;
        v3 m0 = xyz(m[0]), m1 = xyz(m[1]), m2 = xyz(m[2]);
        mf_householder(m0, m1, m2, nrm);
        m[0] = make_float4(m0.x, m0.y, m0.z, 0.f);
        m[1] = make_float4(m1.x, m1.y, m1.z, 0.f);
        m[2] = make_float4(m2.x, m2.y, m2.z, 0.f);
      }
    }
    h.t = 0.f; h.u = 0.f; h.v = 0.f; h.id = -1;
  };
  auto finish = [&](bool done, uint32_t slot, const RawHit& h, bool) {
    if (done && h.id >= 0) hits[slot] = make_float4(__int_as_float(h.id), h.t, h.u, h.v);
  };
  trace_persistent<0, PAIRS>(sc, cnt, &sh.head, sh.nodes, fetch, finish);
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
