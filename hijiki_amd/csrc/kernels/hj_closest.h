// Distance queries ("Distance queries"): the nearest surface point of the uploaded scene to a caller-given point.
// ONE specification with two texts: this header and tests/closest_ref.py.  HJ-NUM-1: binary32, one rounding per operation, no
// contraction except dot3 / cross3 of hj_num.h, correctly rounded `/` and sqrt.
//
// Per-shape functions: pure functions of the point p and the shape's uploaded record -> (q, d2, u, v, side).
//   closest_sphere    record (c, r):  w = p - c, l = len3(w);  q = c + w * (r / l), and c + (r, 0, 0) when l == 0;
//                     d2 = (l - r) * (l - r);  u = v = 0;  side = +1 when l >= r, else -1.
//   closest_triangle  record (a, ab, ac) - the pre-gathered one of the ray walk, ab = b - a and ac = c - a each ONE subtraction.
//                     The region walk of Ericson, Real-Time Collision Detection 5.1.5, on ap = p - a, bp = ap - ab, cp = ap - ac:
//                       d1 = dot3(ab, ap)  d2 = dot3(ac, ap)  d3 = dot3(ab, bp)  d4 = dot3(ac, bp)  d5 = dot3(ab, cp)  d6 = dot3(ac, cp)
//                       vc = d1 * d4 - d3 * d2    vb = d5 * d2 - d1 * d6    va = d3 * d6 - d5 * d4     (two products, one difference)
//                     tested in THIS order, the first that holds decides (u, v), the coefficients of ab and ac - the barycentric
//                     pair of hj_trace_rays' raw hit:
//                       1. vertex a   d1 <= 0 and d2 <= 0                            (0, 0)
//                       2. vertex b   d3 >= 0 and d4 <= d3                           (1, 0)
//                       3. vertex c   d6 >= 0 and d5 <= d6                           (0, 1)
//                       4. edge ab    vc <= 0 and d1 >= 0 and d3 <= 0                (d1 / (d1 - d3), 0)
//                       5. edge ac    vb <= 0 and d2 >= 0 and d6 <= 0                (0, d2 / (d2 - d6))
//                       6. edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0      w = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (1 - w, w)
//                       7. face       x' = (x < 0) ? 0 : x for x = va, vb, vc (a NaN stays);  k = 1 / ((va' + vb') + vc'):  (vb' * k, vc' * k)
//                     The floor in 7 is not Ericson's: in real numbers it changes nothing (the face is reached with all three
//                     positive), in binary32 it keeps the computed pair inside the triangle for a sliver whose areas cancel - the
//                     property the tree's skipping rests on (below).  q = (a + ab * u) + ac * v;  d2 = dot3(p - q, p - q);
//                     side = +1 when dot3(p - q, cross3(ab, ac)) >= 0, else -1.  A degenerate triangle is not special-cased: it
//                     comes out as this text computes it, NaN included (0 / 0 on a zero edge, 0 * inf on a zero face).
//   closest_quad      record (o, e1, e2), a parallelogram:  w = p - o;  s = dot3(w, e1) / dot3(e1, e1), t = dot3(w, e2) / dot3(e2, e2),
//                     each clamped as x = (x < 0) ? 0 : ((x > 1) ? 1 : x) (a NaN stays);  (u, v) = (s, t);  q = (o + e1 * s) + e2 * t;
//                     d2 and side as for the triangle with cross3(e1, e2).  Projecting on the two edges separately is the nearest
//                     point for RECTANGLES only (e1 . e2 == 0); for a sheared quad it is a point of the quad, not the nearest.
//
// The answer for a point (p, r), r2 = r * r: a shape is a candidate when its d2 is not NaN and d2 <= r2; the answer is the candidate
// with the smallest key (d2 as uint32 bits, global shape index).  A NaN or negative r, a non-finite coordinate of p, or no candidate:
// a miss.  The answer depends on the point and the shapes alone - not on the tree, the visiting order or the lane.
//
// The tree decides only what is skipped (cq_box_d2, cq_skip_above; the derivation is in DESIGN.md).  With M the largest magnitude of
// the root box's coordinates, every computed d2 of a shape under a node with box B satisfies
//     sqrt(d2) >= (1 - 6 * 2^-24) * max(0, D - 45 * 2^-24 * M),      D = the real distance from p to B,
// so a node is skipped when its computed box distance cq_box_d2 is above ((sqrt(limit) + 2^-18 * M) * (1 + 2^-19))^2, limit = the
// smaller of r2 and the best d2 so far.  That holds for trees whose boxes bound their subtrees (a leaf's box its shape, the root's box
// everything): every tree the host compiler, hj_build_bvh_device, the refit and the reinsertion produce.  For caller-supplied boxes
// that do not bound their subtrees the answer is whatever the skipping gives: some candidate or a miss, never a fault.
//
// The walk reads the SECOND copy of the uploaded tree (DeviceScene::root2): the uploaded array verbatim in pre-order - every node,
// every leaf with a box of its own, nothing collapsed, no guard records (a guard's padded box is a ray argument) -, kept current by
// hj_scene_update_shapes.  Record i sits at root2 + i; its left child is record i + 1 whatever the first word's link says (a pair
// mark included), its exit is the second word's.  Stackless: a node whose bound exceeds the limit goes to its exit, an inner node to
// i + 1, a leaf runs the shape function and goes to its exit; exits grow, so the walk ends at any depth.  Ordered: nearer child first
// with a bounded stack in LDS, and the stackless walk for a point whose stack would overflow (cq_walk_ordered below).
//   k_cq_walk<STATS, ORDERED>   one lane per point; STATS: nodes visited and shapes tested, summed per workgroup into `partial` (two
//                      uint64 per workgroup, reduced in the wave and through LDS: no global atomics)
//   k_cq_pack          gather points (8 words: hj_probe_points' layout) -> query points (p.xyz, radius)
//   k_cq_resolve       query records -> one float per point: side * distance or distance, max_distance for a miss
// Ordinary loads and stores, no inline assembly.
#pragma once
#include "hj_intersect.h"

#pragma clang fp contract(off)

namespace hj {

constexpr float kCqSlack = 3.814697265625e-06f;      // 2^-18: the absolute slack of the bound, times M
constexpr float kCqGrow = 1.0000019073486328125f;    // 1 + 2^-19: its relative part
constexpr uint32_t kCqNone = 0xFFFFFFFFu;

struct Closest { v3 q; float d2, u, v, side; };

HJ_DEV float cq_side(v3 pq, v3 n) { return dot3(pq, n) >= 0.0f ? 1.0f : -1.0f; }

HJ_DEV Closest closest_sphere(v3 p, float4 sp) {
  const v3 c = xyz(sp);
  const float r = sp.w;
  const v3 w = p - c;
  const float l = len3(w);
  Closest o;
  o.q = (l == 0.0f) ? c + V(r, 0.0f, 0.0f) : c + w * (r / l);
  const float t = l - r;
  o.d2 = t * t;
  o.u = 0.0f; o.v = 0.0f;
  o.side = l >= r ? 1.0f : -1.0f;
  return o;
}

HJ_DEV float cq_floor0(float x) { return x < 0.0f ? 0.0f : x; }
HJ_DEV float cq_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

HJ_DEV Closest closest_triangle(v3 p, v3 a, v3 ab, v3 ac) {
  const v3 ap = p - a, bp = ap - ab, cp = ap - ac;
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  float u, v;
  if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; }
  else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; }
  else if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; }
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; }
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); }
  else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) { const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); u = 1.0f - w; v = w; }
  else {
    const float fa = cq_floor0(va), fb = cq_floor0(vb), fc = cq_floor0(vc);
    const float k = 1.0f / ((fa + fb) + fc);
    u = fb * k; v = fc * k;
  }
  Closest o;
  o.q = (a + ab * u) + ac * v;
  const v3 pq = p - o.q;
  o.d2 = dot3(pq, pq);
  o.u = u; o.v = v;
  o.side = cq_side(pq, cross3(ab, ac));
  return o;
}

HJ_DEV Closest closest_quad(v3 p, v3 o, v3 e1, v3 e2) {
  const v3 w = p - o;
  const float s = cq_clamp01(dot3(w, e1) / dot3(e1, e1)), t = cq_clamp01(dot3(w, e2) / dot3(e2, e2));
  Closest c;
  c.q = (o + e1 * s) + e2 * t;
  const v3 pq = p - c.q;
  c.d2 = dot3(pq, pq);
  c.u = s; c.v = t;
  c.side = cq_side(pq, cross3(e1, e2));
  return c;
}

HJ_DEV Closest closest_shape(const DeviceScene& sc, v3 p, uint32_t shape) {
  if (shape < sc.ns) return closest_sphere(p, sc.spheres[shape]);
  if (shape < sc.ns + sc.nq) {
    const float4* __restrict__ rec = sc.quads + 3 * (size_t)(shape - sc.ns);
    return closest_quad(p, xyz(rec[0]), xyz(rec[1]), xyz(rec[2]));
  }
  const float4* __restrict__ rec = sc.tri_isect + 3 * (size_t)(shape - sc.ns - sc.nq);
  return closest_triangle(p, xyz(rec[0]), xyz(rec[1]), xyz(rec[2]));
}

// The squared distance from p to the box [lo, hi], computed: per axis max(lo - p, p - hi, 0), then dot3.
HJ_DEV float cq_box_d2(v3 p, float4 lo, float4 hi) {
  const v3 d = V(f_max(f_max(lo.x - p.x, p.x - hi.x), 0.0f), f_max(f_max(lo.y - p.y, p.y - hi.y), 0.0f), f_max(f_max(lo.z - p.z, p.z - hi.z), 0.0f));
  return dot3(d, d);
}
// A node whose cq_box_d2 is above this holds no shape whose computed d2 is <= limit.  (limit +inf: +inf, nothing is skipped; a NaN
// slack - a root box that is not finite - compares false: nothing is skipped.)
HJ_DEV float cq_skip_above(float limit, float slack) {
  const float t = (__builtin_sqrtf(limit) + slack) * kCqGrow;
  return t * t;
}
// M of the root record: the largest magnitude of its six coordinates
HJ_DEV float cq_magnitude(float4 lo, float4 hi) {
  return f_max(f_max(f_max(__builtin_fabsf(lo.x), __builtin_fabsf(hi.x)), f_max(__builtin_fabsf(lo.y), __builtin_fabsf(hi.y))),
               f_max(__builtin_fabsf(lo.z), __builtin_fabsf(hi.z)));
}

// The best candidate so far and the threshold it (or the radius) sets
struct CqBest { uint32_t id, key; Closest c; float skip; };

// A leaf: the shape function, the candidate rule, the key rule
HJ_DEV void cq_consider(const DeviceScene& sc, v3 p, float r2, float slack, uint32_t shape, CqBest& b) {
  const Closest c = closest_shape(sc, p, shape);
  const uint32_t key = __float_as_uint(c.d2);
  if (c.d2 <= r2 && (key < b.key || (key == b.key && shape < b.id))) {
    b.id = shape; b.key = key; b.c = c;
    b.skip = cq_skip_above(c.d2, slack);
  }
}

// The stackless walk in array order from record 0, continuing whatever best `b` holds (the answer does not depend on the order, and a
// shape met twice changes nothing: its key is not below itself).
template <bool STATS>
HJ_DEV void cq_walk_stackless(const DeviceScene& sc, const float4* __restrict__ nodes, uint32_t nn, v3 p, float r2, float slack, CqBest& b,
                              uint32_t& visited, uint32_t& tested) {
  uint32_t cur = 0;
  for (;;) {
    // while-while: box steps until the lane stands on a leaf it has to test, then the shape function
    uint32_t shape = 0, ex = 0;
    bool at_leaf = false;
    while (cur < nn && !at_leaf) {
      const float4 n0 = nodes[2 * (size_t)cur], n1 = nodes[2 * (size_t)cur + 1];
      const uint32_t a = __float_as_uint(n0.w), e = __float_as_uint(n1.w);
      ex = e == kEndOfWalk ? nn : e - sc.root2;
      if (STATS) visited++;
      const bool inside = !(cq_box_d2(p, n0, n1) > b.skip);
      const bool inner = (a & kInnerFlag) != 0u;
      at_leaf = inside && !inner;
      shape = a;
      cur = at_leaf ? cur : (inside ? cur + 1u : ex);
    }
    if (!at_leaf) break;
    cq_consider(sc, p, r2, slack, shape, b);
    if (STATS) tested++;
    cur = ex;
  }
}

// The ordered walk: at an inner node both children's records are read - the left child is record i + 1, the right child the left
// child's exit -, the nearer one (by cq_box_d2; a tie: the left) is entered and the farther one pushed, unless its bound already
// exceeds the threshold.  A popped record is tested again: the threshold has shrunk since.  The stack is kCqStack indices per lane
// in LDS, stack[level][lane] (conflict-free).  A push that finds it full gives up: returns false, and the caller runs the stackless
// walk with the best found so far - uploaded trees can be arbitrarily deep.
constexpr uint32_t kCqStack = 32;
template <bool STATS>
HJ_DEV bool cq_walk_ordered(const DeviceScene& sc, const float4* __restrict__ nodes, uint32_t nn, v3 p, float r2, float slack, CqBest& b,
                            uint32_t (*stack)[kBlockThreads], uint32_t& visited, uint32_t& tested) {
  const uint32_t t = threadIdx.x;
  uint32_t sp = 0, cur = 0;
  float4 n0 = nodes[0], n1 = nodes[1];
  if (STATS) visited++;
  bool have = !(cq_box_d2(p, n0, n1) > b.skip);
  for (;;) {
    if (!have) {                                                       // pop until a record passes the threshold as it is now
      while (sp > 0u && !have) {
        cur = stack[--sp][t];
        n0 = nodes[2 * (size_t)cur]; n1 = nodes[2 * (size_t)cur + 1];
        if (STATS) visited++;
        have = !(cq_box_d2(p, n0, n1) > b.skip);
      }
      if (!have) return true;
    }
    const uint32_t a = __float_as_uint(n0.w);
    if ((a & kInnerFlag) == 0u) {
      cq_consider(sc, p, r2, slack, a, b);
      if (STATS) tested++;
      have = false;
      continue;
    }
    const uint32_t l = cur + 1u;
    if (l >= nn) { have = false; continue; }                           // (no pre-order tree: an inner node without children)
    const float4 l0 = nodes[2 * (size_t)l], l1 = nodes[2 * (size_t)l + 1];
    const uint32_t le = __float_as_uint(l1.w);
    const uint32_t r = le == kEndOfWalk ? nn : le - sc.root2;
    if (r >= nn) {                                                     // (no pre-order tree: an inner node has two children; the one there is)
      cur = l; n0 = l0; n1 = l1;
      if (STATS) visited++;
      have = !(cq_box_d2(p, n0, n1) > b.skip);
      continue;
    }
    const float4 r0 = nodes[2 * (size_t)r], r1 = nodes[2 * (size_t)r + 1];
    if (STATS) visited += 2u;
    const float dl = cq_box_d2(p, l0, l1), dr = cq_box_d2(p, r0, r1);
    const bool left_first = !(dr < dl);
    const float d_far = left_first ? dr : dl;
    if (!(d_far > b.skip)) {
      if (sp == kCqStack) return false;
      stack[sp++][t] = left_first ? r : l;
    }
    cur = left_first ? l : r;
    n0 = left_first ? l0 : r0; n1 = left_first ? l1 : r1;
    have = !((left_first ? dl : dr) > b.skip);
  }
}

// points: float4 (p.xyz, r) per point; out: two float4 per point - (shape index as int32 bits or -1, sqrt(d2), q.x, q.y),
// (q.z, u, v, side); a miss: -1 and seven zeros.  ORDERED: cq_walk_ordered with the stackless walk as its fall-back, else the
// stackless walk alone; the records are the same bits either way.
template <bool STATS, bool ORDERED>
__global__ __launch_bounds__(kBlockThreads) void k_cq_walk(DeviceScene sc, const float4* __restrict__ points, uint32_t n, float4* __restrict__ out,
                                                           unsigned long long* __restrict__ partial) {
  __shared__ uint32_t stack[ORDERED ? kCqStack : 1u][kBlockThreads];
  const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
  uint32_t visited = 0, tested = 0;
  if (i < n) {
    const float4 pr = points[i];
    const v3 p = xyz(pr);
    const float r = pr.w, r2 = r * r;
    const float fin = (p.x - p.x) + (p.y - p.y) + (p.z - p.z);         // 0 for finite coordinates, else NaN
    const uint32_t nn = sc.num_nodes - sc.root2;
    const float4* __restrict__ nodes = sc.nodes + 2 * (size_t)sc.root2;
    CqBest b;
    b.id = kCqNone; b.key = kCqNone; b.skip = 0.0f;
    b.c.q = V(0.0f, 0.0f, 0.0f); b.c.d2 = 0.0f; b.c.u = 0.0f; b.c.v = 0.0f; b.c.side = 0.0f;
    if (r >= 0.0f && fin == 0.0f && nn != 0u) {
      const float slack = kCqSlack * cq_magnitude(nodes[0], nodes[1]);
      b.skip = cq_skip_above(r2, slack);
      bool done = false;
      if (ORDERED) done = cq_walk_ordered<STATS>(sc, nodes, nn, p, r2, slack, b, stack, visited, tested);
      if (!done) cq_walk_stackless<STATS>(sc, nodes, nn, p, r2, slack, b, visited, tested);
    }
    const bool hit = b.id != kCqNone;
    out[2 * (size_t)i] = make_float4(__uint_as_float(b.id), hit ? __builtin_sqrtf(b.c.d2) : 0.0f, b.c.q.x, b.c.q.y);
    out[2 * (size_t)i + 1] = make_float4(b.c.q.z, b.c.u, b.c.v, b.c.side);
  }
  if (STATS) {
    __shared__ unsigned long long sums[2][kBlockThreads / 64];
    unsigned long long a = visited, c = tested;
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); c += __shfl_down(c, off); }
    if ((threadIdx.x & 63u) == 0u) { sums[0][threadIdx.x >> 6] = a; sums[1][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long ta = 0, tb = 0;
      for (uint32_t w = 0; w < kBlockThreads / 64; w++) { ta += sums[0][w]; tb += sums[1][w]; }
      partial[2 * (size_t)blockIdx.x] = ta;
      partial[2 * (size_t)blockIdx.x + 1] = tb;
    }
  }
}

// gather points (two float4: position.xyz, ... as hj_probe_points emits them) -> query points (position.xyz, radius)
__global__ __launch_bounds__(kBlockThreads) void k_cq_pack(const float4* __restrict__ gather, uint32_t n, float radius, float4* __restrict__ points) {
  const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= n) return;
  const float4 g = gather[2 * (size_t)i];
  points[i] = make_float4(g.x, g.y, g.z, radius);
}

// query records -> field[i] = side * distance (is_signed) or distance; a miss: max_distance
__global__ __launch_bounds__(kBlockThreads) void k_cq_resolve(const float4* __restrict__ records, uint32_t n, float max_distance, uint32_t is_signed,
                                                              float* __restrict__ field) {
  const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= n) return;
  const float4 r0 = records[2 * (size_t)i];
  const float side = records[2 * (size_t)i + 1].w;
  const bool hit = __float_as_uint(r0.x) != kCqNone;
  field[i] = !hit ? max_distance : (is_signed ? side * r0.y : r0.y);
}

}  // namespace hj
