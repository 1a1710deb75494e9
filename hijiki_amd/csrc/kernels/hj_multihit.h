// All-hit queries ("All-hit queries"): every hit along a caller-given ray - the K nearest in order, how many there
// are, and the signed sum of their crossings - and from that sum whether a point lies inside closed geometry.  ONE specification
// with two texts: this header and tests/allhits_ref.py.  HJ-NUM-1: binary32, one rounding per operation, no contraction except
// dot3 / cross3 of hj_num.h, correctly rounded `/` and sqrt.  The multi-hit formulation is Gribble et al. 2014.
//
// The contract is a function of the ray (o, d, tMin, tMax) and the uploaded tree alone.
//   Candidates.  The pre-order skip-link walk of the verbatim second copy of the uploaded tree (DeviceScene::root2: record i at
//     root2 + i, its left child record i + 1, its exit the second word's), with the caller's [tMin, tMax] NEVER shrunk.  An inner node
//     is entered iff its box passes mh_box_enter below; a leaf's box is not tested; every shape whose leaf is reached is tested with
//     the caller's range.  A quad or a triangle gives one candidate (t, u, v) when quad_test / triangle_test of hj_intersect.h
//     accept it.  A sphere gives up to two: intersect_sphere's arithmetic up to t0, t1 (nothing when its discriminant is < 0), and
//     each root with tMin <= t <= tMax is a candidate with u = 0 for t0, 1 for t1, and v = 0.
//   Box test (mh_box_enter), without fused multiply-add, so that numpy float32 restates it operation for operation:
//     inv = 1 / d per axis;  t1 = (lo - o) * inv, t2 = (hi - o) * inv;  tn = t1 < t2 ? t1 : t2, tp = t1 < t2 ? t2 : t1;
//     T0 = the three tn folded x, y, z by a < b ? b : a;  T1 = the three tp folded by a < b ? a : b;
//     enter iff !(T0 > T1) && !(T0 > tMax) && !(T1 < tMin).
//     Negated comparisons and selects: a NaN T0, T1, tMin or tMax never culls, and zero components, infinities and NaNs of d come out the same in numpy's
//     np.where and ~(a > b).  The closest-hit walk's test (node_step: fused, with an epsilon, against a shrinking tMax) is another one;
//     the candidates here are this test's.
//   Key.  (t as a float, shape index, root), compared in that order: equal t goes to the lower shape index, a sphere's t0 before its t1.
//   Crossing.  +1 for a candidate that leaves through its surface (dot3(d, n_g) > 0), -1 for one that enters (< 0), 0 for == 0 or NaN;
//     n_g = cross3(e1, e2) of a quad's record, cross3(b - a, c - a) of a triangle's; a sphere's t0 enters (-1), its t1 leaves (+1).
//     A point inside a closed surface whose n_g point outward gets +1 along any direction.
//   Records.  counts[i] = (number of candidates as uint32, crossing sum as int32).  hits[i][j], j < K: the min(count, K) candidates
//     with the smallest keys in ascending key order as (shape index bits, t, u, v) - hj_trace_rays' record -, the rest (-1, 0, 0, 0).
//   Record i depends on ray i and the scene alone: not on the lane, the workgroup or the chunk.
//
// k_mh_walk<LIST>     one lane per ray, the stackless while-while walk (exits relative to root2, kEndOfWalk).  LIST: the K best are
//                     kept per lane in LDS as list[j][lane] - 16 bytes a slot, consecutive lanes 16 bytes apart, so a wave's b128
//                     access is conflict-free -, kMhMaxHits x 256 x 16 B = 32 KB a workgroup, inserted by key from the tail.  No register
//                     array is indexed by a variable.  !LIST (K = 0, counting): no list, no LDS.  Counts stay in registers.
// k_mh_inside<PARITY> one lane per point: three K = 0 walks from p along kMhDir[0..2] (HJ_INSIDE_DIR0 .. 2 of the public header) with
//                     tMin = 0, tMax = +inf, one after the other in the lane, and the vote: a ray votes inside when its crossing sum
//                     is > 0 (PARITY: when its number of candidates is odd), the point is inside with two votes or more.
// Ordinary loads and stores, no global atomics, no inline assembly.
#pragma once
#include "hj_intersect.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kMhMaxHits = 8;     // HJ_ALLHITS_MAX_HITS

// the three directions of hj_points_inside, from the public header: pairwise non-parallel, no zero component, no two components of one direction equal in
// magnitude (axis-aligned scenes are in general position), of length 1 to float32's rounding (the sphere's roots assume it)
constexpr float kMhDir[3][3] = {{HJ_INSIDE_DIR0_X, HJ_INSIDE_DIR0_Y, HJ_INSIDE_DIR0_Z},
                                 {HJ_INSIDE_DIR1_X, HJ_INSIDE_DIR1_Y, HJ_INSIDE_DIR1_Z},
                                 {HJ_INSIDE_DIR2_X, HJ_INSIDE_DIR2_Y, HJ_INSIDE_DIR2_Z}};

struct MhCount { uint32_t n; int32_t cross; };

HJ_DEV bool mh_box_enter(v3 o, v3 inv, float tmin, float tmax, float4 lo, float4 hi) {
  const float x1 = (lo.x - o.x) * inv.x, x2 = (hi.x - o.x) * inv.x;
  const float y1 = (lo.y - o.y) * inv.y, y2 = (hi.y - o.y) * inv.y;
  const float z1 = (lo.z - o.z) * inv.z, z2 = (hi.z - o.z) * inv.z;
  const float tnx = x1 < x2 ? x1 : x2, tpx = x1 < x2 ? x2 : x1;
  const float tny = y1 < y2 ? y1 : y2, tpy = y1 < y2 ? y2 : y1;
  const float tnz = z1 < z2 ? z1 : z2, tpz = z1 < z2 ? z2 : z1;
  float T0 = tnx < tny ? tny : tnx;
  T0 = T0 < tnz ? tnz : T0;
  float T1 = tpx < tpy ? tpx : tpy;
  T1 = T1 < tpz ? T1 : tpz;
  return !(T0 > T1) && !(T0 > tmax) && !(T1 < tmin);
}

HJ_DEV int32_t mh_facing(float dn) { return dn > 0.0f ? 1 : (dn < 0.0f ? -1 : 0); }

// key order of two records (shape index bits, t, u, v): (t, shape index, root); the root of a sphere's candidate is its u
HJ_DEV bool mh_before(float4 a, float4 b) {
  const uint32_t ia = __float_as_uint(a.x), ib = __float_as_uint(b.x);
  return a.y < b.y || (a.y == b.y && (ia < ib || (ia == ib && a.z < b.z)));
}

// One candidate: counted, and with LIST inserted by key into the lane's list of at most K (held: how many it holds).
template <bool LIST>
HJ_DEV void mh_candidate(float4 (*list)[kBlockThreads], uint32_t K, uint32_t& held, MhCount& c, float4 rec, int32_t facing) {
  c.n++;
  c.cross += facing;
  if (!LIST) return;
  const uint32_t t = threadIdx.x;
  uint32_t pos;
  if (held == K) {
    if (!mh_before(rec, list[K - 1u][t])) return;
    pos = K - 1u;
  } else {
    pos = held++;
  }
  while (pos > 0u) {
    const float4 prev = list[pos - 1u][t];
    if (!mh_before(rec, prev)) break;
    list[pos][t] = prev;
    pos--;
  }
  list[pos][t] = rec;
}

// A leaf: the shape's candidates under the caller's range
template <bool LIST>
HJ_DEV void mh_shape(const DeviceScene& sc, const Ray& r, uint32_t shape, float4 (*list)[kBlockThreads], uint32_t K, uint32_t& held, MhCount& c) {
  const float id = __uint_as_float(shape);
  if (shape < sc.ns) {
    const float4 sp = sc.spheres[shape];
    const v3 l = r.o - xyz(sp);                                          // intersect_sphere's arithmetic up to t0, t1
    const float b = 2.0f * dot3(r.d, l);
    const float cc = dot3(l, l) - sp.w * sp.w;
    float d = b * b - 4.0f * cc;
    if (d < 0.0f) return;
    d = __builtin_sqrtf(d);
    const float t0 = -0.5f * (b + d), t1 = -0.5f * (b - d);
    if (r.tmin <= t0 && t0 <= r.tmax) mh_candidate<LIST>(list, K, held, c, make_float4(id, t0, 0.0f, 0.0f), -1);
    if (r.tmin <= t1 && t1 <= r.tmax) mh_candidate<LIST>(list, K, held, c, make_float4(id, t1, 1.0f, 0.0f), 1);
    return;
  }
  RawHit h;
  h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.id = -1;
  if (shape < sc.ns + sc.nq) {
    const float4* __restrict__ rec = sc.quads + 3 * (size_t)(shape - sc.ns);
    const float4 O = rec[0], E1 = rec[1], E2 = rec[2];
    if (quad_test(r, O, E1, E2, h)) mh_candidate<LIST>(list, K, held, c, make_float4(id, h.t, h.u, h.v), mh_facing(dot3(r.d, cross3(xyz(E1), xyz(E2)))));
    return;
  }
  const float4* __restrict__ rec = sc.tri_isect + 3 * (size_t)(shape - sc.ns - sc.nq);
  const float4 A = rec[0], B = rec[1], C = rec[2];
  if (triangle_test(r, A, B, C, h)) mh_candidate<LIST>(list, K, held, c, make_float4(id, h.t, h.u, h.v), mh_facing(dot3(r.d, cross3(xyz(B), xyz(C)))));
}

// The walk of one ray: every candidate counted, the K best listed
template <bool LIST>
HJ_DEV MhCount mh_walk(const DeviceScene& sc, const Ray& r, float4 (*list)[kBlockThreads], uint32_t K, uint32_t& held) {
  MhCount c;
  c.n = 0u; c.cross = 0;
  const uint32_t nn = sc.num_nodes - sc.root2;
  const float4* __restrict__ nodes = sc.nodes + 2 * (size_t)sc.root2;
  const v3 inv = V(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
  uint32_t cur = 0;
  for (;;) {
    // while-while: box steps until the lane stands on a leaf, then the shape's candidates
    uint32_t shape = 0, ex = 0;
    bool at_leaf = false;
    while (cur < nn && !at_leaf) {
      const float4 n0 = nodes[2 * (size_t)cur], n1 = nodes[2 * (size_t)cur + 1];
      const uint32_t a = __float_as_uint(n0.w), e = __float_as_uint(n1.w);
      ex = e == kEndOfWalk ? nn : e - sc.root2;
      const bool enter = mh_box_enter(r.o, inv, r.tmin, r.tmax, n0, n1);
      at_leaf = (a & kInnerFlag) == 0u;                                 // (a leaf's box is not tested)
      shape = a;
      cur = at_leaf ? cur : (enter ? cur + 1u : ex);
    }
    if (!at_leaf) break;
    mh_shape<LIST>(sc, r, shape, list, K, held, c);
    cur = ex;
  }
  return c;
}

// rays: two float4 per ray (origin.xyz, direction.x | direction.yz, tMin, tMax), hj_trace_rays' layout
HJ_DEV Ray mh_ray(float4 a, float4 b) {
  Ray r; r.o = V(a.x, a.y, a.z); r.d = V(a.w, b.x, b.y); r.tmin = b.z; r.tmax = b.w;
  return r;
}

// counts: (candidates, crossing sum) per ray; hits: K float4 per ray (LIST alone; 1 <= K <= kMhMaxHits)
template <bool LIST>
__global__ __launch_bounds__(kBlockThreads) void k_mh_walk(DeviceScene sc, const float4* __restrict__ rays, uint32_t n, uint32_t K,
                                                           uint2* __restrict__ counts, float4* __restrict__ hits) {
  __shared__ float4 list[LIST ? kMhMaxHits : 1u][kBlockThreads];
  const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= n) return;
  uint32_t held = 0;
  const MhCount c = mh_walk<LIST>(sc, mh_ray(rays[2 * (size_t)i], rays[2 * (size_t)i + 1]), list, K, held);
  counts[i] = make_uint2(c.n, (uint32_t)c.cross);
  if (LIST) {
    float4* __restrict__ out = hits + (size_t)K * i;
    for (uint32_t j = 0; j < K; j++) out[j] = j < held ? list[j][threadIdx.x] : make_float4(__int_as_float(-1), 0.0f, 0.0f, 0.0f);
  }
}

// points: float4 (p.xyz, reserved) per point; out: (inside, votes) per point.  A ray votes inside when its crossing sum is > 0,
// PARITY: when its number of candidates is odd; the point is inside with two votes or more.
template <bool PARITY>
__global__ __launch_bounds__(kBlockThreads) void k_mh_inside(DeviceScene sc, const float4* __restrict__ points, uint32_t n, uint2* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= n) return;
  const float4 p = points[i];
  Ray r;
  r.o = V(p.x, p.y, p.z); r.tmin = 0.0f; r.tmax = kInf;
  uint32_t votes = 0, held = 0;
#pragma nounroll
  for (uint32_t k = 0; k < 3u; k++) {
    r.d = k == 0u ? V(kMhDir[0][0], kMhDir[0][1], kMhDir[0][2])
                  : (k == 1u ? V(kMhDir[1][0], kMhDir[1][1], kMhDir[1][2]) : V(kMhDir[2][0], kMhDir[2][1], kMhDir[2][2]));
    const MhCount c = mh_walk<false>(sc, r, nullptr, 0u, held);
    votes += (PARITY ? (c.n & 1u) != 0u : c.cross > 0) ? 1u : 0u;
  }
  out[i] = make_uint2(votes >= 2u ? 1u : 0u, votes);
}

}  // namespace hj
