// The re-layout of hj_scene_upload ON THE DEVICE (large trees): from the reference's skip-link array and triangle / vertex
// arrays, uploaded as they are, to what the kernels read (kernels/hj_device.h) - pre-gathered triangle records, collapsed
// tree, pair nodes, hot-first node order, sibling groups, explicit links.  Same derivation as the host code in
// scene_upload.hip (which stays for small trees, where it takes a millisecond, and for arrays that are not trees), step by step:
//
//   k_rl_triangles                 tri_isect / tri_shade, one thread per triangle
//   k_rl_guard_want, _unpair, scan, k_rl_guard_build    leaf guards (HJ_LEAF_GUARDS): the uploaded array with a one-child inner node in
//                                  front of every guarded leaf - what the steps below work on, as the host's do
//   k_rl_init, k_rl_links          area, parent and parent count of every node: the device path wants a TREE (every node but
//                                  the root has exactly one parent, children lie behind their parent); anything else -> host path
//   k_rl_collapse_level  x depth   the collapse (an inner node over two inner nodes dropped when its area is > thr x its nearest
//                                  kept ancestor's): the ancestor's area comes down level by level, one launch per level
//   k_rl_pair_flags, scan, k_rl_pair_records    pair nodes numbered in array order, their 96-byte records
//   k_rl_kept + scan, radix sort   the kept nodes in array order; stable sort by area, descending: the first 512 are the hot ones
//   k_rl_preorder_flags + scan     small-tree order of the cold nodes: pre-order    (or)
//   k_rl_group_sizes x depth (bottom-up), k_rl_group_offsets x depth (top-down)    sibling groups: the cold children of a node
//                                  side by side, every group on an even index, the group of the larger child following directly
//                                  (the host's depth-first numbering, with every group padded to an even size so that a
//                                  subtree's size does not depend on where it starts)
//   k_rl_records                   the 32-byte device records with explicit links
//
// The image does not depend on the layout; tests render every scene kind through both paths (HJ_UPLOAD_DEVICE = 0 / 1).
#include "hj_internal.h"
#include "guard_box.hpp"
#include "scene_relayout.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kMaxKids = 64;            // children of a kept node after the collapse (a collapsed binary tree: 2^levels); more -> host path

struct RL {
  const hj_bvh_node* bvh;              // the array the steps work on: the uploaded one, or the guarded one
  uint32_t N, first_tri, nshapes;
  uint32_t guarded;                     // bvh holds guard nodes: inner nodes over one leaf, which share their exit
  float thr;                            // collapse threshold
  float* sa;
  float* anc;
  uint32_t* parent;
  uint32_t* nparents;
  uint32_t* depth;
  uint8_t* del;                         // 1: no record (collapsed inner node, or a leaf folded into a pair)
  uint8_t* is_hot;
  uint32_t* pair_flag;                  // then (after the scan) the pair index of a pair node
  uint32_t* pair_idx;
  uint32_t* map;                        // device index of a kept node
  uint32_t* tsub;                       // slots of the sibling groups below a node
  uint32_t* goff;                       // where a node's group of children starts
  uint32_t* err;                        // [0] not a tree  [1] too many children  [2] levels that did something (collapse pass)
};

__device__ inline bool rl_inner(const RL& r, uint32_t i) { return r.bvh[i].shape_index == HJ_BVH_INNER; }
__device__ inline uint32_t rl_resolve(const RL& r, uint32_t i) { while (i < r.N && r.del[i]) i++; return i; }   // first kept node of a subtree

__global__ void k_rl_triangles(const hj_triangle* __restrict__ tris, const hj_vertex* __restrict__ verts, uint32_t nt,
                               float4* __restrict__ isect, float4* __restrict__ shade) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  tri_records(tris, verts, i, isect, shade);
}

// Leaf guards (scene_upload.hip "Guard nodes for single leaves"): which leaves of the uploaded array get one ...
__global__ void k_rl_guard_want(const hj_bvh_node* __restrict__ bvh, uint32_t n0, uint32_t ns, uint32_t guard_spheres, uint32_t guard_flat,
                                uint32_t* __restrict__ want) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  const uint32_t sh = bvh[i].shape_index;
  want[i] = sh == HJ_BVH_INNER ? 0u : (sh < ns ? guard_spheres : guard_flat);
}
// ... but the two triangle leaves of a future pair node, which keep their parent's box as their guard (a launch of its own: it
// clears what k_rl_guard_want set)
__global__ void k_rl_guard_unpair(const hj_bvh_node* __restrict__ bvh, uint32_t n0, uint32_t first_tri, uint32_t* __restrict__ want) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0 || i + 2 >= n0 || bvh[i].shape_index != HJ_BVH_INNER) return;
  const uint32_t l = i + 1, rr = bvh[l].exit_index;
  if (rr != l + 1) return;                                    // (rr = i + 2 < n0 from here on)
  const uint32_t sl = bvh[l].shape_index, sr = bvh[rr].shape_index;
  if (sl == HJ_BVH_INNER || sr == HJ_BVH_INNER) return;
  if (sl >= first_tri && sr >= first_tri) { want[l] = 0; want[rr] = 0; }
}
// The guarded array: node i at gidx[i] = i + before[i] + want[i], its guard - the shape's own padded bounds, the leaf's exit - in
// front of it; exits move with the nodes they name (an exit beyond the array stays beyond it).  before = exclusive scan of want.
__global__ void k_rl_guard_build(const hj_bvh_node* __restrict__ bvh, uint32_t n0, RefitShapes shapes, float pad_abs,
                                 const uint32_t* __restrict__ want, const uint32_t* __restrict__ before, uint32_t guards,
                                 hj_bvh_node* __restrict__ out, uint32_t* __restrict__ gidx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  hj_bvh_node nd = bvh[i];
  const uint32_t e = nd.exit_index;
  nd.exit_index = e < n0 ? e + before[e] : e + guards;
  uint32_t at = i + before[i];
  if (want[i]) {
    hj_bvh_node g = nd;
    g.shape_index = HJ_BVH_INNER;
    su_guard_box(shapes, nd.shape_index, pad_abs, g.aabb_min, g.aabb_max);
    out[at++] = g;
  }
  out[at] = nd;
  gidx[i] = at;
}

__global__ void k_rl_init(RL r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N) return;
  const hj_bvh_node nd = r.bvh[i];
  const float dx = nd.aabb_max[0] - nd.aabb_min[0], dy = nd.aabb_max[1] - nd.aabb_min[1], dz = nd.aabb_max[2] - nd.aabb_min[2];
  float a = (dx >= 0 && dy >= 0 && dz >= 0) ? dx * dy + dy * dz + dz * dx : 0.f;
  if (!(a == a)) a = 0.f;
  r.sa[i] = a;
  r.anc[i] = 0.f;
  r.parent[i] = kNone; r.nparents[i] = 0; r.depth[i] = i == 0 ? 0u : kNone;
  r.del[i] = 0; r.is_hot[i] = 0; r.pair_flag[i] = 0; r.map[i] = 0; r.tsub[i] = 0; r.goff[i] = 0;
}

__global__ void k_rl_links(RL r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N) return;
  if (r.bvh[i].exit_index <= i) { atomicOr(&r.err[0], 1u); return; }
  if (!rl_inner(r, i)) return;
  const uint32_t l = i + 1;
  if (l >= r.N) { atomicOr(&r.err[0], 1u); return; }
  const uint32_t rr = r.bvh[l].exit_index;
  if (r.guarded && !rl_inner(r, l) && rr == r.bvh[i].exit_index) {   // a guard: its only child is its leaf
    r.parent[l] = i;
    atomicAdd(&r.nparents[l], 1u);
    return;
  }
  if (rr >= r.N || rr <= l || r.bvh[rr].exit_index != r.bvh[i].exit_index) { atomicOr(&r.err[0], 1u); return; }   // (the right child's exit is its parent's)
  r.parent[l] = i; r.parent[rr] = i;
  atomicAdd(&r.nparents[l], 1u); atomicAdd(&r.nparents[rr], 1u);
}
__global__ void k_rl_check_tree(RL r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N) return;
  if (r.nparents[i] != (i == 0 ? 0u : 1u)) atomicOr(&r.err[0], 1u);
}

// One level of the collapse (scene_upload.hip: "Collapse"): nodes of depth L decide, and hand their children the area of their
// nearest kept ancestor and depth L + 1.
__global__ void k_rl_collapse_level(RL r, uint32_t L) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N || r.depth[i] != L || !rl_inner(r, i)) return;
  // (branch-free on purpose: with the short-circuit form of this condition AMD clang 22 kept the zero high half of a 64-bit index
  // in a register it re-used for a load inside a narrower exec mask - lanes whose left child is a leaf then formed a wild address)
  const size_t l = (size_t)i + 1;
  const hj_bvh_node ni = r.bvh[i], nl = r.bvh[l];
  // (a guard's only child is its leaf, and their common exit may lie beyond the array: the leaf stands in for the sibling, which
  // keeps the guard - a leaf child - and hands the leaf the guard's area and depth L + 1, as the host does)
  const bool single = (r.guarded != 0) & (nl.shape_index != HJ_BVH_INNER) & (nl.exit_index == ni.exit_index);
  const size_t rr = single ? l : (size_t)nl.exit_index;
  const hj_bvh_node nr = r.bvh[rr];
  bool in = true;
  for (int k = 0; k < 3; k++)
    in = in & (nl.aabb_min[k] >= ni.aabb_min[k]) & (nl.aabb_max[k] <= ni.aabb_max[k]) & (nr.aabb_min[k] >= ni.aabb_min[k]) & (nr.aabb_max[k] <= ni.aabb_max[k]);
  const float a = r.anc[i], si = r.sa[i];
  const bool d = (i != 0) & (nl.shape_index == HJ_BVH_INNER) & (nr.shape_index == HJ_BVH_INNER) & (a > 0.f) & (si > r.thr * a) & in;
  r.del[i] = d ? 1 : 0;
  const float down = d ? a : si;
  r.anc[l] = down; r.anc[rr] = down;
  r.depth[l] = L + 1; r.depth[rr] = L + 1;
  r.err[2] = L + 1;                                 // (any writer: a level that had an inner node)
}

__global__ void k_rl_pair_flags(RL r) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N) return;
  uint32_t f = 0;
  if (i + 2 < r.N && rl_inner(r, i)) {
    const uint32_t l = i + 1, rr = r.bvh[l].exit_index;
    if (rr == l + 1) {
      const uint32_t sl = r.bvh[l].shape_index, sr = r.bvh[rr].shape_index;
      if (sl != HJ_BVH_INNER && sr != HJ_BVH_INNER && sl >= r.first_tri && sr >= r.first_tri && r.bvh[rr].exit_index == r.bvh[i].exit_index) f = 1;
    }
  }
  r.pair_flag[i] = f;
}
__global__ void k_rl_pair_records(RL r, const float4* __restrict__ isect, float4* __restrict__ pairs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N || !r.pair_flag[i]) return;
  const uint32_t l = i + 1, rr = l + 1;
  const uint32_t sh[2] = {r.bvh[l].shape_index, r.bvh[rr].shape_index};
  float4* out = pairs + 6 * (size_t)r.pair_idx[i];
  for (int k = 0; k < 2; k++) {
    const size_t t = sh[k] - r.first_tri;
    float4 a = isect[3 * t];
    a.w = __uint_as_float(sh[k]);
    out[3 * k] = a; out[3 * k + 1] = isect[3 * t + 1]; out[3 * k + 2] = isect[3 * t + 2];
  }
  r.del[l] = 1; r.del[rr] = 1;                       // no records for the two leaves
}

// kept nodes, in array order: flags for the scan, then keys (area bits; areas are >= 0, so the bits order like the floats) and
// values (node index) for the stable descending sort
__global__ void k_rl_kept_flags(RL r, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < r.N) flag[i] = r.del[i] ? 0u : 1u;
}
__global__ void k_rl_kept_list(RL r, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, uint32_t* __restrict__ keys,
                               uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N || !flag[i]) return;
  keys[rank[i]] = __float_as_uint(r.sa[i]);
  vals[rank[i]] = i;
}
__global__ void k_rl_mark_hot(RL r, const uint32_t* __restrict__ sorted, uint32_t hot) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= hot) return;
  r.is_hot[sorted[k]] = 1;
  r.map[sorted[k]] = k;
}

// small trees: the cold kept nodes keep pre-order behind the hot ones
__global__ void k_rl_cold_flags(RL r, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < r.N) flag[i] = (!r.del[i] && !r.is_hot[i]) ? 1u : 0u;
}
__global__ void k_rl_preorder_map(RL r, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, uint32_t hot) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < r.N && flag[i]) r.map[i] = hot + rank[i];
}

// The kept children of kept node i, in the walk's order (scene_upload.hip "node order").  Returns their number, or -1.
__device__ inline int rl_kids(const RL& r, uint32_t i, uint32_t* kids) {
  const uint32_t e0 = r.bvh[i].exit_index;
  const uint32_t end = e0 < r.N ? rl_resolve(r, e0) : r.N;
  int n = 0;
  for (uint32_t c = rl_resolve(r, i + 1); c < r.N && c != end;) {
    if (n == kMaxKids) return -1;
    kids[n++] = c;
    const uint32_t e = r.bvh[c].exit_index;
    c = e < r.N ? rl_resolve(r, e) : r.N;
  }
  return n;
}
__device__ inline bool rl_has_group(const RL& r, uint32_t i) { return rl_inner(r, i) && !r.pair_flag[i]; }   // a kept node whose children have records

// bottom-up: slots of a node's own group (its cold children, padded to an even number) + of the groups below its children
__global__ void k_rl_group_sizes(RL r, uint32_t L) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N || r.depth[i] != L || r.del[i] || !rl_has_group(r, i)) return;
  uint32_t kids[kMaxKids];
  const int n = rl_kids(r, i, kids);
  if (n < 0) { atomicOr(&r.err[1], 1u); return; }
  uint32_t cold = 0, below = 0;
  for (int k = 0; k < n; k++) {
    cold += r.is_hot[kids[k]] ? 0u : 1u;
    if (rl_has_group(r, kids[k])) below += r.tsub[kids[k]];
  }
  r.tsub[i] = ((cold + 1u) & ~1u) + below;
}
// top-down: a node's cold children take the slots of its group in the walk's order; the groups of its children follow, the
// largest child's first
__global__ void k_rl_group_offsets(RL r, uint32_t L) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N || r.depth[i] != L || r.del[i] || !rl_has_group(r, i)) return;
  uint32_t kids[kMaxKids];
  const int n = rl_kids(r, i, kids);
  if (n < 0) return;
  uint32_t next = r.goff[i], cold = 0;
  for (int k = 0; k < n; k++) if (!r.is_hot[kids[k]]) { r.map[kids[k]] = next + cold; cold++; }
  next += (cold + 1u) & ~1u;
  // stable insertion sort by area, descending
  for (int a = 1; a < n; a++) {
    const uint32_t x = kids[a];
    const float sx = r.sa[x];
    int b = a - 1;
    while (b >= 0 && r.sa[kids[b]] < sx) { kids[b + 1] = kids[b]; b--; }
    kids[b + 1] = x;
  }
  for (int k = 0; k < n; k++) if (rl_has_group(r, kids[k])) { r.goff[kids[k]] = next; next += r.tsub[kids[k]]; }
}

// the second copy of the tree (api/scene_upload.hip, kernels/hj_intersect.h general_position): the reference's own array, record i
// at base + i - nothing collapsed; pair nodes keep their mark, their two leaves' records are never reached
// (bvh0, n0: the uploaded array; gidx: where its nodes are in r.bvh, NULL without guards)
__global__ void k_rl_records2(RL r, const hj_bvh_node* __restrict__ bvh0, uint32_t n0, const uint32_t* __restrict__ gidx,
                              float4* __restrict__ dev, uint32_t base) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  const hj_bvh_node nd = bvh0[i];
  const uint32_t g = gidx ? gidx[i] : i;
  uint32_t a;
  if (nd.shape_index != HJ_BVH_INNER) a = nd.shape_index;
  else if (r.pair_flag[g]) a = hj::kInnerFlag | hj::kPairFlag | r.pair_idx[g];
  else a = hj::kInnerFlag | (i + 1 < n0 ? base + i + 1 : hj::kEndOfWalk);
  const uint32_t b = nd.exit_index < n0 ? base + nd.exit_index : hj::kEndOfWalk;
  float4* rec = dev + 2 * ((size_t)base + i);
  rec[0] = make_float4(nd.aabb_min[0], nd.aabb_min[1], nd.aabb_min[2], __uint_as_float(a));
  rec[1] = make_float4(nd.aabb_max[0], nd.aabb_max[1], nd.aabb_max[2], __uint_as_float(b));
}

__global__ void k_rl_records(RL r, float4* __restrict__ dev) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.N || r.del[i]) return;
  const hj_bvh_node nd = r.bvh[i];
  uint32_t a;
  if (nd.shape_index != HJ_BVH_INNER) a = nd.shape_index;
  else if (r.pair_flag[i]) a = hj::kInnerFlag | hj::kPairFlag | r.pair_idx[i];
  else {
    const uint32_t l = rl_resolve(r, i + 1);
    a = hj::kInnerFlag | (l < r.N ? r.map[l] : hj::kEndOfWalk);
  }
  const uint32_t e = nd.exit_index < r.N ? rl_resolve(r, nd.exit_index) : r.N;
  const uint32_t b = e < r.N ? r.map[e] : hj::kEndOfWalk;
  float4* rec = dev + 2 * (size_t)r.map[i];
  rec[0] = make_float4(nd.aabb_min[0], nd.aabb_min[1], nd.aabb_min[2], __uint_as_float(a));
  rec[1] = make_float4(nd.aabb_max[0], nd.aabb_max[1], nd.aabb_max[2], __uint_as_float(b));
}

// where every node of the uploaded array went (hj_scene_update_shapes): its record, its guard's record (a guard is the record in
// front of its leaf in the guarded array: an inner node over one child, which the collapse never drops)
__global__ void k_rl_node_map(RL r, uint32_t n0, const uint32_t* __restrict__ gidx, uint2* __restrict__ where) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  const uint32_t g = gidx ? gidx[i] : i;
  const bool has_guard = gidx && g != (i ? gidx[i - 1] + 1u : 0u);
  where[i] = make_uint2(r.del[g] ? kNone : r.map[g], has_guard && !r.del[g - 1] ? r.map[g - 1] : kNone);
}

}  // namespace

namespace hjapi {

int place_node_array(DevBufs& bufs, size_t rec_bytes, size_t kept, float4** out) {
  // The walk adds 32 * index to the low word of the array's address without a carry (kernels/hj_walk.h): the array must not
  // cross a 4 GiB boundary.  Allocate twice the size and start at the boundary if it would.
  const size_t bytes = std::max<size_t>(rec_bytes, 16) + 128;   // (slack: a whole 128-byte line may be read around the last record)
  if (bytes >= (1ull << 32)) return set_error(bufs.ctx, HJ_ERR_UNSUPPORTED, "BVH of %zu records: the device node array is limited to 4 GiB", kept);
  uint8_t* p = nullptr;
  HJ_TRY(bufs.alloc(p, bytes));
  uintptr_t start = reinterpret_cast<uintptr_t>(p);
  if ((start >> 32) != ((start + bytes - 1) >> 32)) {
    bufs.take(p).release();
    HJ_TRY(bufs.alloc(p, 2 * bytes));
    start = reinterpret_cast<uintptr_t>(p);
    if ((start >> 32) != ((start + bytes - 1) >> 32)) start = ((start >> 32) + 1) << 32;
  }
  *out = reinterpret_cast<float4*>(start);
  return HJ_OK;
}

int relayout_on_device(hj_context* ctx, const hj_scene_desc* s, const hj_triangle* d_tris, const hj_vertex* d_verts, bool pairs_on,
                       int node_order, float collapse_thr, bool timing, DevBufs& keep, RelayoutOut& out, const hj_bvh_node* d_tree) {
  // d_tree: the skip-link array is on the device already (hj_build_bvh_device's tree: hj_context::resident); s->bvh is not read then
  out = RelayoutOut{};
  const size_t N0 = s->num_bvh_nodes;                       // the uploaded array; N: the array the steps work on (with the guards)
  if (N0 < 3 || N0 >= 0x3FFFFFFFu) return HJ_ERR_UNSUPPORTED;
  size_t N = N0;
  hipStream_t st = ctx->stream;
  StageClock clock{timing, "hj_scene_upload (device): %-24s %8.2f ms\n", st};
  DevBufs tmp(ctx);                                         // scratch: released on return
  int rc = HJ_OK;
  const uint32_t n0 = (uint32_t)N0, nt = (uint32_t)s->num_triangles;
  const dim3 blk(256), grid0((n0 + 255) / 256);

  // triangle records
  float4 *isect = nullptr, *shade = nullptr;
  HJ_TRY(keep.alloc(isect, 3 * (size_t)nt, 64));
  HJ_TRY(keep.alloc(shade, 4 * (size_t)nt, 64));
  if (nt) hipLaunchKernelGGL(k_rl_triangles, dim3((nt + 255) / 256), blk, 0, st, d_tris, d_verts, nt, isect, shade);
  clock.mark("triangle records");

  // the skip-link array as it is
  hj_bvh_node* d_bvh = const_cast<hj_bvh_node*>(d_tree);      // (the kernels only read it)
  if (!d_bvh) {
    HJ_TRY(tmp.alloc(d_bvh, N0));
    HJ_HIP(ctx, hipMemcpyAsync(d_bvh, s->bvh, sizeof(hj_bvh_node) * N0, hipMemcpyHostToDevice, st));
  }
  const hj_bvh_node* d_bvh0 = d_bvh;

  // leaf guards (HJ_LEAF_GUARDS, scene_upload.hip): 2 (default) every triangle or quad leaf that does not become half of a pair
  // node; 1 sphere leaves only, 3 all leaves (not exact).  The steps below then work on the guarded array.
  uint32_t* gidx = nullptr;
  {
    const int mode = ctx->tuning.leaf_guards;
    const bool guard_spheres = mode == 1 || mode == 3, guard_flat = mode >= 2;
    if ((guard_spheres && s->num_spheres != 0) || (guard_flat && s->num_quads + s->num_triangles != 0)) {
      uint32_t *want = nullptr, *before = nullptr;
      HJ_TRY(tmp.alloc(want, N0)); HJ_TRY(tmp.alloc(before, N0 + 1));
      hipLaunchKernelGGL(k_rl_guard_want, grid0, blk, 0, st, d_bvh0, n0, (uint32_t)s->num_spheres, guard_spheres ? 1u : 0u, guard_flat ? 1u : 0u, want);
      if (guard_flat) hipLaunchKernelGGL(k_rl_guard_unpair, grid0, blk, 0, st, d_bvh0, n0, (uint32_t)(s->num_spheres + s->num_quads), want);
      size_t bytes = 0;
      HJ_HIP(ctx, rocprim::exclusive_scan(nullptr, bytes, want, before, 0u, N0, rocprim::plus<uint32_t>(), st));
      uint8_t* scan_tmp = nullptr;
      HJ_TRY(tmp.alloc(scan_tmp, std::max<size_t>(bytes, 16)));
      HJ_HIP(ctx, rocprim::exclusive_scan(scan_tmp, bytes, want, before, 0u, N0, rocprim::plus<uint32_t>(), st));
      uint32_t last[2] = {0, 0};
      hj_bvh_node root{};
      HJ_HIP(ctx, hipMemcpyAsync(&last[0], before + (N0 - 1), 4, hipMemcpyDeviceToHost, st));
      HJ_HIP(ctx, hipMemcpyAsync(&last[1], want + (N0 - 1), 4, hipMemcpyDeviceToHost, st));
      HJ_HIP(ctx, hipMemcpyAsync(&root, d_bvh0, sizeof root, hipMemcpyDeviceToHost, st));
      HJ_HIP(ctx, hipStreamSynchronize(st));
      const uint32_t guards = last[0] + last[1];
      if (guards != 0 && N0 + guards < 0x3FFFFFFFu) {
        RefitShapes shapes{};
        shapes.ns = (uint32_t)s->num_spheres; shapes.nq = (uint32_t)s->num_quads; shapes.nt = nt;
        shapes.triangles = d_tris; shapes.vertices = d_verts;
        float4 *d_spheres = nullptr, *d_quads = nullptr;
        HJ_TRY(tmp.alloc(d_spheres, std::max<size_t>(s->num_spheres, 1))); HJ_TRY(tmp.alloc(d_quads, std::max<size_t>(3 * s->num_quads, 1)));
        if (s->num_spheres) HJ_HIP(ctx, hipMemcpyAsync(d_spheres, s->spheres, sizeof(float4) * s->num_spheres, hipMemcpyHostToDevice, st));
        if (s->num_quads) HJ_HIP(ctx, hipMemcpyAsync(d_quads, s->quads, sizeof(float4) * 3 * s->num_quads, hipMemcpyHostToDevice, st));
        shapes.spheres = d_spheres; shapes.quads = d_quads;
        hj_bvh_node* guarded = nullptr;
        N = N0 + guards;
        HJ_TRY(tmp.alloc(guarded, N)); HJ_TRY(tmp.alloc(gidx, N0));
        hipLaunchKernelGGL(k_rl_guard_build, grid0, blk, 0, st, d_bvh0, n0, shapes, guard_pad_abs(root.aabb_min, root.aabb_max, s->camera.position),
                           want, before, guards, guarded, gidx);
        d_bvh = guarded;
      }
    }
  }
  clock.mark("leaf guards");
  const uint32_t n32 = (uint32_t)N;
  const dim3 grid((n32 + 255) / 256);
  RL r{};
  r.bvh = d_bvh; r.N = n32; r.guarded = gidx ? 1u : 0u; r.first_tri = (uint32_t)(s->num_spheres + s->num_quads);
  r.nshapes = (uint32_t)(s->num_spheres + s->num_quads + s->num_triangles);
  r.thr = collapse_thr;
  HJ_TRY(tmp.alloc(r.sa, N)); HJ_TRY(tmp.alloc(r.anc, N)); HJ_TRY(tmp.alloc(r.parent, N)); HJ_TRY(tmp.alloc(r.nparents, N));
  HJ_TRY(tmp.alloc(r.depth, N)); HJ_TRY(tmp.alloc(r.del, N)); HJ_TRY(tmp.alloc(r.is_hot, N)); HJ_TRY(tmp.alloc(r.pair_flag, N));
  HJ_TRY(tmp.alloc(r.pair_idx, N + 1)); HJ_TRY(tmp.alloc(r.map, N)); HJ_TRY(tmp.alloc(r.tsub, N)); HJ_TRY(tmp.alloc(r.goff, N));
  HJ_TRY(tmp.alloc(r.err, 4));
  uint32_t *flag = nullptr, *rank = nullptr, *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr;
  HJ_TRY(tmp.alloc(flag, N)); HJ_TRY(tmp.alloc(rank, N + 1)); HJ_TRY(tmp.alloc(keys, N)); HJ_TRY(tmp.alloc(vals, N));
  HJ_TRY(tmp.alloc(keys2, N)); HJ_TRY(tmp.alloc(vals2, N));
  HJ_HIP(ctx, hipMemsetAsync(r.err, 0, sizeof(uint32_t) * 4, st));
  size_t scan_bytes = 0, sort_bytes = 0;
  HJ_HIP(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, flag, rank, 0u, N, rocprim::plus<uint32_t>(), st));
  HJ_HIP(ctx, rocprim::radix_sort_pairs_desc(nullptr, sort_bytes, keys, keys2, vals, vals2, N, 0, 32, st));
  uint8_t* prim_tmp = nullptr;
  HJ_TRY(tmp.alloc(prim_tmp, std::max(scan_bytes, sort_bytes)));
  size_t prim_bytes = std::max(scan_bytes, sort_bytes);
  uint32_t h_err[4] = {0, 0, 0, 0};
  auto read_err = [&]() -> int {
    HJ_HIP(ctx, hipMemcpyAsync(h_err, r.err, sizeof h_err, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipStreamSynchronize(st));
    return HJ_OK;
  };
  auto last_of_scan = [&](const uint32_t* fl, const uint32_t* rk, uint32_t& total) -> int {    // exclusive scan: total = rank[N-1] + flag[N-1]
    uint32_t a = 0, b = 0;
    HJ_HIP(ctx, hipMemcpyAsync(&a, rk + (N - 1), 4, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipMemcpyAsync(&b, fl + (N - 1), 4, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipStreamSynchronize(st));
    total = a + b;
    return HJ_OK;
  };

  const bool dbg = ctx->tuning.relayout_debug;
  auto check = [&](const char* what) {
    if (!dbg) return;
    const hipError_t e1 = hipStreamSynchronize(st), e2 = hipGetLastError();
    std::fprintf(stderr, "rl debug: %-20s sync %s, last %s\n", what, hipGetErrorString(e1), hipGetErrorString(e2));
  };
  if (dbg) std::fprintf(stderr, "rl debug: N %u bvh %p sa %p anc %p parent %p nparents %p depth %p del %p hot %p pf %p pi %p map %p tsub %p goff %p err %p\n", r.N,
                        (const void*)r.bvh, (void*)r.sa, (void*)r.anc, (void*)r.parent, (void*)r.nparents, (void*)r.depth, (void*)r.del, (void*)r.is_hot,
                        (void*)r.pair_flag, (void*)r.pair_idx, (void*)r.map, (void*)r.tsub, (void*)r.goff, (void*)r.err);
  check("uploads");
  hipLaunchKernelGGL(k_rl_init, grid, blk, 0, st, r);
  check("init");
  hipLaunchKernelGGL(k_rl_links, grid, blk, 0, st, r);
  check("links");
  hipLaunchKernelGGL(k_rl_check_tree, grid, blk, 0, st, r);
  check("check_tree");
  rc = read_err();
  if (rc != HJ_OK) return rc;
  if (h_err[0]) return HJ_ERR_UNSUPPORTED;                   // not a tree: the host path reasons about arbitrary arrays
  clock.mark("node upload + tree check");

  // collapse, level by level (the levels end when one has no inner node)
  uint32_t levels = 0;
  for (uint32_t L = 0; L < 4096; L += 16) {
    for (uint32_t k = 0; k < 16; k++) { hipLaunchKernelGGL(k_rl_collapse_level, grid, blk, 0, st, r, L + k); if (dbg && L + k < 3) check("collapse level"); }
    rc = read_err();
    if (rc != HJ_OK) return rc;
    levels = h_err[2];                                       // deepest level + 1 that held an inner node
    if (levels < L + 16) break;
  }
  clock.mark("collapse");

  // pair nodes
  uint32_t num_pairs = 0;
  float4* pairs = nullptr;
  if (pairs_on) {
    hipLaunchKernelGGL(k_rl_pair_flags, grid, blk, 0, st, r);
    HJ_HIP(ctx, rocprim::exclusive_scan(prim_tmp, prim_bytes, r.pair_flag, r.pair_idx, 0u, N, rocprim::plus<uint32_t>(), st));
    rc = last_of_scan(r.pair_flag, r.pair_idx, num_pairs);
    if (rc != HJ_OK) return rc;
  }
  HJ_TRY(keep.alloc(pairs, 6 * (size_t)num_pairs, 64));
  if (num_pairs) hipLaunchKernelGGL(k_rl_pair_records, grid, blk, 0, st, r, isect, pairs);
  clock.mark("pair nodes");

  // kept nodes, hot-first
  uint32_t M = 0;
  hipLaunchKernelGGL(k_rl_kept_flags, grid, blk, 0, st, r, flag);
  HJ_HIP(ctx, rocprim::exclusive_scan(prim_tmp, prim_bytes, flag, rank, 0u, N, rocprim::plus<uint32_t>(), st));
  rc = last_of_scan(flag, rank, M);
  if (rc != HJ_OK) return rc;
  hipLaunchKernelGGL(k_rl_kept_list, grid, blk, 0, st, r, flag, rank, keys, vals);
  HJ_HIP(ctx, rocprim::radix_sort_pairs_desc(prim_tmp, prim_bytes, keys, keys2, vals, vals2, M, 0, 32, st));   // stable: equal areas keep array order
  const uint32_t hot = std::min<uint32_t>(hj::kHotNodes, M);
  hipLaunchKernelGGL(k_rl_mark_hot, dim3((hot + 255) / 256), blk, 0, st, r, vals2, hot);
  clock.mark("hot-first sort");

  // order of the cold nodes
  uint32_t m_all = 0;
  if (node_order == 0 || (node_order < 0 && num_pairs == 0)) {    // small trees (cache-resident): pre-order; large ones: sibling groups
    uint32_t cold = 0;
    hipLaunchKernelGGL(k_rl_cold_flags, grid, blk, 0, st, r, flag);
    HJ_HIP(ctx, rocprim::exclusive_scan(prim_tmp, prim_bytes, flag, rank, 0u, N, rocprim::plus<uint32_t>(), st));
    rc = last_of_scan(flag, rank, cold);
    if (rc != HJ_OK) return rc;
    hipLaunchKernelGGL(k_rl_preorder_map, grid, blk, 0, st, r, flag, rank, hot);
    m_all = hot + cold;
  } else {
    for (uint32_t L = levels + 1; L-- > 0;) hipLaunchKernelGGL(k_rl_group_sizes, grid, blk, 0, st, r, L);
    // the root: a record of its own behind the hot ones when it is not one of them, then its group on the next even index
    uint8_t root_hot = 0;
    uint32_t t_root = 0;
    HJ_HIP(ctx, hipMemcpyAsync(&root_hot, r.is_hot, 1, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipMemcpyAsync(&t_root, r.tsub, 4, hipMemcpyDeviceToHost, st));
    rc = read_err();
    if (rc != HJ_OK) return rc;
    if (h_err[1]) return HJ_ERR_UNSUPPORTED;                 // a node with more than kMaxKids kept children
    uint32_t base = (hot + 1u) & ~1u;
    if (!root_hot) { const uint32_t m0 = base; HJ_HIP(ctx, hipMemcpyAsync(r.map, &m0, 4, hipMemcpyHostToDevice, st)); base += 2; }
    HJ_HIP(ctx, hipMemcpyAsync(r.goff, &base, 4, hipMemcpyHostToDevice, st));
    HJ_HIP(ctx, hipStreamSynchronize(st));                   // (the two words above live on this stack frame)
    for (uint32_t L = 0; L <= levels; L++) hipLaunchKernelGGL(k_rl_group_offsets, grid, blk, 0, st, r, L);
    m_all = base + t_root;
  }
  clock.mark("node order");

  // device records (zero-filled padding), placed so that the array does not cross a 4 GiB boundary (kernels/hj_walk.h)
  if ((size_t)m_all + N0 >= hj::kEndOfWalk) return set_error(ctx, HJ_ERR_UNSUPPORTED, "BVH of %zu records: too large", (size_t)m_all + N0);
  const size_t rec_bytes = sizeof(float4) * 2 * ((size_t)m_all + N0);     // the two copies of the tree
  float4* dev = nullptr;
  HJ_TRY(place_node_array(keep, rec_bytes, M, &dev));
  HJ_HIP(ctx, hipMemsetAsync(dev, 0, rec_bytes, st));
  hipLaunchKernelGGL(k_rl_records, grid, blk, 0, st, r, dev);
  hipLaunchKernelGGL(k_rl_records2, grid0, blk, 0, st, r, d_bvh0, n0, gidx, dev, m_all);
  out.nodes = dev;
  uint2* where = nullptr;
  HJ_TRY(keep.alloc(where, N0));
  hipLaunchKernelGGL(k_rl_node_map, grid0, blk, 0, st, r, n0, gidx, where);
  out.node_map = where;
  uint32_t root = 0;
  HJ_HIP(ctx, hipMemcpyAsync(&root, r.map, 4, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));
  HJ_HIP(ctx, hipGetLastError());
  clock.mark("device records");
  out.tri_isect = isect; out.tri_shade = shade; out.tri_pair = pairs;
  out.num_nodes = m_all + n0; out.root = root; out.root2 = m_all; out.num_hot = hot; out.num_pairs = num_pairs; out.kept = M;
  return HJ_OK;
}

}  // namespace hjapi
