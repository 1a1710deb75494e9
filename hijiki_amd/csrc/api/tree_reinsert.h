// Parallel reinsertion on the device (hj_optimize_bvh_device, api/tree_reinsert.hip; Meister & Bittner 2018, "Parallel reinsertion for
// bounding volume hierarchy optimization"; objective and bound: host/tree_opt.cpp optimize_by_reinsertion_batched): the per-node steps
// of one pass on the POINTER form of the tree - parent, two children and box per node, node ids = the positions of the input records,
// node 0 the root.  Plain functions of the arrays: the kernels of api/tree_reinsert.hip call them on the device, tests/reinsert_restatement.hip
// on the host (the CPU reference of tests/test_reinsert_host.py and tests/test_reinsert_gpu.py).
//
//   ri_search    the node X whose sibling N should become, and the decrease in surface-area cost
//                    gain(X) = area(P) + sum over the ancestors A of P that shrink (area(A) - area(A')) - area(X' u N) - growth of X's ancestors
//                (P: N's parent, which moves with it; ': the box once N is gone).  From P towards the root; at every ancestor the OTHER
//                child's subtree is walked through the parent links: no stack, no heap, no depth limit.  A branch is dead when what its
//                nodes inherit plus area(N) cannot beat the best found.  Areas and sums in double (a float box's area is exact to 2^-53):
//                a gain that is reported is a decrease of the cost k_rf_cost measures.
//   ri_walk_path the nodes a move N -> X must hold, by one of two conflict rules: the four nodes whose links it rewrites (with
//                ri_target_stays: the links remain a tree's, the gains may interact), or every node whose links or box it changes - N, its
//                parent, sibling and grandparent, X and its parent, and the path from N up to the common ancestor (`pivot`, which the
//                search reports) and down to X - (the gains are independent: the cost cannot rise)
//   ri_apply     the link changes of a move (host/tree_opt.cpp, phase 2): the sibling takes the parent's place, the parent goes between
//                X and X's parent with the children (X, N)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hj {
namespace reinsert {

#define HJ_RI_FN __host__ __device__ inline

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxPasses = 64;
enum : uint32_t { kInfoMoves = 0, kInfoError = 1, kInfoHolders = 2, kInfoWords = 4 };

struct Tree {
  uint32_t N;                   // nodes = records
  uint32_t* parent;             // [N] kNone: the root
  uint32_t* c0;                 // [N] kNone: a leaf
  uint32_t* c1;
  float4* lo;                   // [N] box; lo.w = the record's shape word
  float4* hi;
  uint32_t* target;             // [N] per pass: the X of node N's move, kNone: none
  uint32_t* moving;             // [N] ... the move holds the nodes its conflict rule covers
  uint32_t* win;                // [N] ... and is applied
  uint32_t* pivot;              // [N] ... the common ancestor of N and X
  float* gain;                  // [N]
  unsigned long long* lock;     // [N] zero between passes
  uint32_t* arrived;            // [N] zero between passes
  uint32_t* size;               // [N] records of the subtree
  uint32_t* info;               // [kInfoWords]
};

struct Box { float lo[3], hi[3]; };

HJ_RI_FN Box ri_box(const Tree& t, uint32_t i) {
  const float4 a = t.lo[i], b = t.hi[i];
  return Box{{a.x, a.y, a.z}, {b.x, b.y, b.z}};
}
HJ_RI_FN Box ri_join(const Box& a, const Box& b) {
  Box r;
  for (int k = 0; k < 3; k++) { r.lo[k] = __builtin_fminf(a.lo[k], b.lo[k]); r.hi[k] = __builtin_fmaxf(a.hi[k], b.hi[k]); }
  return r;
}
HJ_RI_FN double ri_area(const Box& b) {                     // (kernels/hj_lbvh.h rf_area)
  const double dx = (double)b.hi[0] - (double)b.lo[0], dy = (double)b.hi[1] - (double)b.lo[1], dz = (double)b.hi[2] - (double)b.lo[2];
  return (dx >= 0 && dy >= 0 && dz >= 0) ? dx * dy + dy * dz + dz * dx : 0.0;
}
HJ_RI_FN uint32_t ri_sibling(const Tree& t, uint32_t p, uint32_t child) { return t.c0[p] == child ? t.c1[p] : t.c0[p]; }

struct Found {
  uint32_t x = kNone, pivot = kNone;
  double gain = 0.0;
  uint32_t steps = 0;           // nodes looked at; a tree of N nodes needs fewer than 4 N + 16 (more: the links are no tree's)
};

// The subtree of R, whose nodes all gain `base` before their own terms; `pivot`: what a find reports as the common ancestor.
// root_counts: R itself is a place (not so N's own sibling, where N already is).
HJ_RI_FN bool ri_scan(const Tree& t, uint32_t R, uint32_t pivot, double base, const Box& nb, double an, bool root_counts, Found& f) {
  const uint32_t budget = 4u * t.N + 16u;
  uint32_t cur = R;
  double ind = 0.0;                                         // growth of the nodes between R and cur (both inclusive of R, exclusive of cur)
  for (;;) {
    if (cur >= t.N || ++f.steps > budget) return false;
    const Box xb = ri_box(t, cur);
    const double m = ri_area(ri_join(xb, nb));
    const double g = base - ind - m;
    if (g > f.gain && (cur != R || root_counts)) { f.gain = g; f.x = cur; f.pivot = pivot; }
    const double down = ind + (m - ri_area(xb));            // what cur's children inherit
    const uint32_t l = t.c0[cur];
    if (l != kNone && base - down - an > f.gain) { ind = down; cur = l; continue; }
    for (;;) {                                              // the next node in pre-order that is not below cur
      if (cur == R) return true;
      const uint32_t par = t.parent[cur];
      if (par >= t.N || ++f.steps > budget) return false;
      if (t.c0[par] == cur) { cur = t.c1[par]; break; }
      cur = par;
      const Box pb = ri_box(t, cur);
      ind -= ri_area(ri_join(pb, nb)) - ri_area(pb);
    }
  }
}

// false: the links are no tree's (f is void)
HJ_RI_FN bool ri_search(const Tree& t, uint32_t n, Found& f) {
  f = Found{};
  if (n == 0 || n >= t.N) return true;
  const uint32_t P = t.parent[n];
  if (P == 0) return true;                                  // the root's children stay (record 0 stays the root)
  if (P >= t.N) return false;
  const uint32_t S = ri_sibling(t, P, n);
  if (S >= t.N) return false;
  const Box nb = ri_box(t, n);
  const double an = ri_area(nb);
  double base = ri_area(ri_box(t, P));
  if (!ri_scan(t, S, P, base, nb, an, false, f)) return false;
  uint32_t below = P;
  Box bb = ri_box(t, S);                                    // the box of `below` once N is gone
  for (uint32_t A = t.parent[P]; A != kNone; A = t.parent[A]) {
    if (A >= t.N || ++f.steps > 4u * t.N + 16u) return false;
    const uint32_t other = ri_sibling(t, A, below);
    if (other >= t.N) return false;
    if (!ri_scan(t, other, A, base, nb, an, true, f)) return false;
    bb = ri_join(bb, ri_box(t, other));                     // A without N
    const double shrunk = ri_area(bb);
    if (A != 0 && base - shrunk > f.gain) { f.gain = base - shrunk; f.x = A; f.pivot = A; }   // beside the ancestor itself
    base += ri_area(ri_box(t, A)) - shrunk;
    below = A;
  }
  if (!((float)f.gain > 0.f)) { f.x = kNone; f.pivot = kNone; f.gain = 0.0; }   // only a float gain > 0 counts
  return true;
}

// f(node) for every node of the move n -> x that the conflict rule covers; ends with false as soon as f does (or where the links
// are no tree's).  WHOLE_PATH: N, its parent, sibling and grandparent, X and its parent, and every node from N up to `pivot` and down
// to X - the moves that survive touch disjoint paths, so their gains are independent.  Otherwise the four nodes whose PARENT word (and,
// for the moved parent, child words) a move rewrites: N, its parent and sibling, and X; the grandparent and X's parent only have
// the child word rewritten that holds one of those four, so two moves never write one word (ri_apply).
template <bool WHOLE_PATH, class F>
HJ_RI_FN bool ri_walk_path(const Tree& t, uint32_t n, uint32_t x, uint32_t pivot, F&& f) {
  const uint32_t P = t.parent[n];
  if (P >= t.N || x >= t.N || pivot >= t.N) return false;
  const uint32_t S = ri_sibling(t, P, n), G = t.parent[P], XP = t.parent[x];
  if (S >= t.N || G >= t.N || XP >= t.N) return false;
  if (!WHOLE_PATH) return f(n) && f(P) && f(S) && f(x);
  if (!f(S) || !f(G) || !f(XP)) return false;
  uint32_t steps = 0;
  for (uint32_t a = n;; a = t.parent[a]) {
    if (a >= t.N || ++steps > t.N) return false;
    if (!f(a)) return false;
    if (a == pivot) break;
  }
  for (uint32_t a = x; a != pivot; a = t.parent[a]) {
    if (a >= t.N || ++steps > t.N) return false;
    if (!f(a)) return false;
  }
  return true;
}

// The four-node rule's second condition: X lies in no subtree that another surviving move takes away (moving[a] != 0: a is the N of
// a move that holds its four nodes) - every subtree that moves is hung onto an edge that stays, so the links remain a tree's.
HJ_RI_FN bool ri_target_stays(const Tree& t, const uint32_t* moving, uint32_t n, uint32_t x) {
  uint32_t steps = 0;
  for (uint32_t a = x; a != kNone; a = t.parent[a]) {
    if (a >= t.N || ++steps > t.N) return false;
    if (a != n && moving[a]) return false;
  }
  return true;
}

HJ_RI_FN unsigned long long ri_key(float gain, uint32_t n) { return ((unsigned long long)__builtin_bit_cast(uint32_t, gain) << 32) | n; }

HJ_RI_FN void ri_apply(const Tree& t, uint32_t n, uint32_t X) {
  const uint32_t P = t.parent[n], G = t.parent[P], S = ri_sibling(t, P, n), XP = t.parent[X];
  (t.c0[G] == P ? t.c0[G] : t.c1[G]) = S;
  t.parent[S] = G;
  (t.c0[XP] == X ? t.c0[XP] : t.c1[XP]) = P;
  t.parent[P] = XP;
  t.c0[P] = X; t.c1[P] = n;
  t.parent[X] = P; t.parent[n] = P;
}

}  // namespace reinsert
}  // namespace hj
