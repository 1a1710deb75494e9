// hj_optimize_bvh_device: the tree hj_build_bvh_device / hj_refit_bvh_device left on the device, optimised by parallel reinsertion
// (api/tree_reinsert.h: the per-node steps; DESIGN.md 4, "Reinsertion on the device").  A pass is launches on the context's stream -
// search, lock, check, win, apply, boxes, cost - and ONE synchronisation, for the counts and the cost (a second one where a pass
// is done again by the whole-path rule); the pointer form is derived once and flattened once.  Includes no kernel header but hj_num.h's: the cost's kernel and the vote are other units' (refit_pass.hpp,
// tree_vote.hpp).
#include "hj_internal.h"
#include "refit_pass.hpp"
#include "tree_vote.hpp"
#include "tree_reinsert.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {
namespace reinsert {

// A word another CU may have written in this launch: not through the vector L1 (kernels/hj_lbvh.h ld_agent)
HJ_DEV float4 ri_ld_agent(const float4* p) {
  const float* f = reinterpret_cast<const float*>(p);
  return make_float4(__hip_atomic_load(f + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                     __hip_atomic_load(f + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                     __hip_atomic_load(f + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0.f);
}

// records -> pointer form, one thread per record.  The records are a build's or a refit's (checked there); links that point outside
// the array all the same leave a leaf and a word in info[kInfoError], so that nothing below reads outside [0, N).
__global__ __launch_bounds__(256) void k_ri_init(const float4* __restrict__ rec, Tree t) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.N) return;
  const float4 lo = rec[2 * (size_t)i], hi = rec[2 * (size_t)i + 1];
  t.lo[i] = lo; t.hi[i] = hi;
  t.lock[i] = 0ull; t.arrived[i] = 0u; t.target[i] = kNone;
  if (i == 0) t.parent[0] = kNone;
  uint32_t l = kNone, r = kNone;
  if (__float_as_uint(lo.w) == HJ_BVH_INNER) {
    l = i + 1;
    r = l < t.N ? __float_as_uint(rec[2 * (size_t)l + 1].w) : kNone;
    if (l >= t.N || r >= t.N || r <= l) { atomicOr(&t.info[kInfoError], 1u); l = r = kNone; }
    else { t.parent[l] = i; t.parent[r] = i; }
  }
  t.c0[i] = l; t.c1[i] = r;
}

// 1. search: one thread per node (64-thread workgroups: the walks' lengths differ widely)
__global__ __launch_bounds__(64) void k_ri_search(Tree t) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= t.N) return;
  Found f;
  if (!ri_search(t, n, f)) { atomicOr(&t.info[kInfoError], 2u); f.x = kNone; }
  t.target[n] = f.x; t.pivot[n] = f.pivot; t.gain[n] = (float)f.gain;
}

// 2. conflicts: the key (gain bits << 32) | N by atomicMax into the lock word of every node the rule covers (api/tree_reinsert.h
// ri_walk_path: WHOLE_PATH or the four nodes whose links the move rewrites)
template <bool WHOLE_PATH>
__global__ __launch_bounds__(64) void k_ri_lock(Tree t) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= t.N || t.target[n] == kNone) return;
  const unsigned long long key = ri_key(t.gain[n], n);
  if (!ri_walk_path<WHOLE_PATH>(t, n, t.target[n], t.pivot[n], [&](uint32_t a) { atomicMax(&t.lock[a], key); return true; }))
    atomicOr(&t.info[kInfoError], 4u);
}
// ... a move holds its nodes if it reads its own key back on all of them
template <bool WHOLE_PATH>
__global__ __launch_bounds__(64) void k_ri_check(Tree t) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= t.N) return;
  uint32_t holds = 0;
  if (t.target[n] != kNone) {
    const unsigned long long key = ri_key(t.gain[n], n);
    holds = ri_walk_path<WHOLE_PATH>(t, n, t.target[n], t.pivot[n], [&](uint32_t a) { return t.lock[a] == key; }) ? 1u : 0u;
    if (holds) atomicAdd(&t.info[kInfoHolders], 1u);
  }
  t.moving[n] = holds;
}
// ... and wins; under the four-node rule only if its X lies in no subtree that another holder takes away
template <bool WHOLE_PATH>
__global__ __launch_bounds__(64) void k_ri_win(Tree t) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= t.N) return;
  t.win[n] = (t.moving[n] && (WHOLE_PATH || ri_target_stays(t, t.moving, n, t.target[n]))) ? 1u : 0u;
}
// 3. apply: no two winners write one word; the lock words go back to zero (every thread its own node's)
__global__ __launch_bounds__(256) void k_ri_apply(Tree t) {
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= t.N) return;
  t.lock[n] = 0ull;
  if (!t.win[n]) return;
  ri_apply(t, n, t.target[n]);
  atomicAdd(&t.info[kInfoMoves], 1u);
}

// The cost of the pointer form, k_rf_cost's sums: partial[b] = sum over the inner nodes among workgroup b's 256 nodes of area(node),
// in double, in a fixed order
__global__ __launch_bounds__(256) void k_ri_cost(Tree t, double* __restrict__ partial) {
  __shared__ double s_sum[256];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  s_sum[threadIdx.x] = (i < t.N && t.c0[i] != kNone) ? ri_area(ri_box(t, i)) : 0.0;
  __syncthreads();
  for (uint32_t w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = s_sum[0];
}

// 4. boxes, k_rf_climb's form: one thread per node, a leaf's climbs with its box in registers; at every inner node the first thread
// to arrive leaves, the second one joins its box with the SIBLING's (agent scope) and writes the node's.  A leaf's box never changes.
// SIZES: the same climb for the subtree's record count instead (after the last pass).
template <bool SIZES>
__global__ __launch_bounds__(256) void k_ri_climb(Tree t) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.N || t.c0[i] != kNone) return;
  Box b = ri_box(t, i);
  uint32_t size = 1;
  if (SIZES) t.size[i] = 1;
  uint32_t child = i, node = t.parent[i], steps = 0;
  while (node < t.N && ++steps <= t.N) {
    __threadfence();                                         // my child's box is visible before I count myself in
    if (atomicAdd(&t.arrived[node], 1u) == 0u) return;
    t.arrived[node] = 0;                                     // (nobody else comes: the counters are zero again when the pass ends)
    __threadfence();
    const uint32_t sib = ri_sibling(t, node, child);
    if (sib >= t.N) return;
    if (SIZES) {
      size += 1u + __hip_atomic_load(&t.size[sib], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      t.size[node] = size;
    } else {
      const float4 slo = ri_ld_agent(&t.lo[sib]), shi = ri_ld_agent(&t.hi[sib]);
      b.lo[0] = f_min(b.lo[0], slo.x); b.lo[1] = f_min(b.lo[1], slo.y); b.lo[2] = f_min(b.lo[2], slo.z);
      b.hi[0] = f_max(b.hi[0], shi.x); b.hi[1] = f_max(b.hi[1], shi.y); b.hi[2] = f_max(b.hi[2], shi.z);
      t.lo[node] = make_float4(b.lo[0], b.lo[1], b.lo[2], __uint_as_float(HJ_BVH_INNER));
      t.hi[node] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.f);
    }
    child = node;
    node = t.parent[node];
  }
}

// Flatten, one thread per node: its pre-order position is what precedes it - one record per ancestor, and the left sibling's subtree
// wherever the path comes up from a right child -, its exit the end of its subtree (the right spine: root_exit), left child first.
__global__ __launch_bounds__(256) void k_ri_flatten(Tree t, uint32_t root_exit, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.N) return;
  uint32_t pos = 0, steps = 0;
  for (uint32_t a = i, p = t.parent[i]; p < t.N && ++steps <= t.N; a = p, p = t.parent[p]) pos += 1u + (t.c1[p] == a ? t.size[t.c0[p]] : 0u);
  const uint32_t end = pos + t.size[i];
  if (pos >= t.N) return;                                    // (links that are no tree's: nothing is written outside the array)
  const float4 lo = t.lo[i], hi = t.hi[i];
  out[2 * (size_t)pos] = lo;
  out[2 * (size_t)pos + 1] = make_float4(hi.x, hi.y, hi.z, __uint_as_float(end < t.N ? end : root_exit));
}

}  // namespace reinsert
}  // namespace hj

namespace {

namespace ri = hj::reinsert;

int read_cost(hj_context* ctx, const hj_bvh_node* d_nodes, const double* d_partial, size_t num_partial, double* out) {
  std::vector<double> partial(num_partial);
  hj_bvh_node root{};
  HJ_HIP(ctx, hipMemcpy(partial.data(), d_partial, sizeof(double) * num_partial, hipMemcpyDeviceToHost));
  HJ_HIP(ctx, hipMemcpy(&root, d_nodes, sizeof root, hipMemcpyDeviceToHost));
  *out = refit_cost(partial, root);
  return HJ_OK;
}

// Behind the refusals.  A failure in here releases the resident tree (the caller does).
int optimize_resident(hj_context* ctx, const hj_scene_desc* scene, uint32_t passes, hj_bvh_node* out_nodes, double* out_before,
                      double* out_after, uint32_t* out_moves) {
  hj_context::ResidentTree& rt = ctx->resident;
  const size_t total = rt.total;
  const uint32_t N = (uint32_t)total;
  const Tuning tn = ctx->tuning = Tuning::from_env();
  const bool timing = tn.lbvh_timing != 0;
  StageClock clock{timing, "hj_optimize_bvh_device: %-26s %7.2f ms\n", ctx->stream};
  hipStream_t st = ctx->stream;
  DevBufs bufs(ctx);
  hj_bvh_node* d_in = static_cast<hj_bvh_node*>(rt.nodes.p);
  const size_t num_partial = refit_cost_partials(N);
  double* d_partial = nullptr;
  HJ_TRY(bufs.alloc(d_partial, num_partial));
  refit_enqueue_cost(ctx, reinterpret_cast<const float4*>(d_in), N, d_partial);
  HJ_HIP(ctx, hipStreamSynchronize(st));
  HJ_HIP(ctx, hipGetLastError());
  double before = 0.0;
  HJ_TRY(read_cost(ctx, d_in, d_partial, num_partial, &before));
  if (out_before) *out_before = before;
  if (out_after) *out_after = before;
  if (out_moves) *out_moves = 0;
  clock.mark("cost of the input");
  uint32_t moves = 0;
  if (passes != 0 && total >= 7) {
    ri::Tree t{};
    t.N = N;
    HJ_TRY(bufs.alloc(t.parent, total)); HJ_TRY(bufs.alloc(t.c0, total)); HJ_TRY(bufs.alloc(t.c1, total));
    HJ_TRY(bufs.alloc(t.lo, total)); HJ_TRY(bufs.alloc(t.hi, total));
    HJ_TRY(bufs.alloc(t.target, total)); HJ_TRY(bufs.alloc(t.pivot, total)); HJ_TRY(bufs.alloc(t.gain, total));
    HJ_TRY(bufs.alloc(t.moving, total)); HJ_TRY(bufs.alloc(t.win, total));
    HJ_TRY(bufs.alloc(t.lock, total)); HJ_TRY(bufs.alloc(t.arrived, total)); HJ_TRY(bufs.alloc(t.size, total));
    HJ_TRY(bufs.alloc(t.info, ri::kInfoWords));
    const dim3 blk(256), grid((N + 255u) / 256u), blk_w(64), grid_w((N + 63u) / 64u);
    uint32_t info[ri::kInfoWords] = {0, 0, 0, 0};
    HJ_HIP(ctx, hipMemsetAsync(t.info, 0, sizeof info, st));
    double* d_sums = nullptr;
    HJ_TRY(bufs.alloc(d_sums, num_partial));
    std::vector<double> sums(num_partial);
    hipLaunchKernelGGL(ri::k_ri_init, grid, blk, 0, st, reinterpret_cast<const float4*>(d_in), t);
    hipLaunchKernelGGL(ri::k_ri_cost, grid, blk, 0, st, t, d_sums);          // (the area sum the first pass is measured against)
    HJ_HIP(ctx, hipMemcpyAsync(info, t.info, sizeof info, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * num_partial, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipStreamSynchronize(st));                    // (the verdict on the links, before any walk follows them)
    HJ_HIP(ctx, hipGetLastError());
    if (info[ri::kInfoError]) return set_error(ctx, HJ_ERR_DEVICE, "hj_optimize_bvh_device: the records on the device are no tree's (%u)", info[ri::kInfoError]);
    clock.mark("pointer form");
    // A pass resolves its conflicts by the four-node rule, which keeps the links a tree's and lets moves through the same upper nodes
    // share a pass, but whose gains may interact.  So the pass is MEASURED: the links are saved before it, the cost of the pointer form
    // (sum of the inner nodes' areas, in a fixed order) is taken after it, and a pass that did not lower it is taken back and done again
    // from the same search by the whole-path rule, whose gains are independent: the cost falls with every pass that moves anything.
    // The same second attempt where the four-node rule moved nothing although a move held its nodes (holders whose X lies in each
    // other's subtree refuse each other): under the whole-path rule the largest key always wins, so a call ends without a move only
    // when no node has a gain.
    uint32_t *save_parent = nullptr, *save_c0 = nullptr, *save_c1 = nullptr;
    HJ_TRY(bufs.alloc(save_parent, total)); HJ_TRY(bufs.alloc(save_c0, total)); HJ_TRY(bufs.alloc(save_c1, total));
    const size_t link_bytes = sizeof(uint32_t) * total;
    // enqueue: conflicts by `whole_path`, apply, boxes, cost; then the ONE synchronisation of the pass -> moves, area sum
    auto resolve = [&](bool whole_path, uint32_t pass, uint32_t& moved, uint32_t& holders, double& area_sum) -> int {
      if (whole_path) {
        hipLaunchKernelGGL(ri::k_ri_lock<true>, grid_w, blk_w, 0, st, t);
        hipLaunchKernelGGL(ri::k_ri_check<true>, grid_w, blk_w, 0, st, t);
        hipLaunchKernelGGL(ri::k_ri_win<true>, grid_w, blk_w, 0, st, t);
      } else {
        hipLaunchKernelGGL(ri::k_ri_lock<false>, grid_w, blk_w, 0, st, t);
        hipLaunchKernelGGL(ri::k_ri_check<false>, grid_w, blk_w, 0, st, t);
        hipLaunchKernelGGL(ri::k_ri_win<false>, grid_w, blk_w, 0, st, t);
      }
      clock.mark(whole_path ? "conflicts (whole path)" : "conflicts (four nodes)");
      hipLaunchKernelGGL(ri::k_ri_apply, grid, blk, 0, st, t);
      hipLaunchKernelGGL(ri::k_ri_climb<false>, grid, blk, 0, st, t);
      hipLaunchKernelGGL(ri::k_ri_cost, grid, blk, 0, st, t, d_sums);
      HJ_HIP(ctx, hipMemcpyAsync(info, t.info, sizeof info, hipMemcpyDeviceToHost, st));
      HJ_HIP(ctx, hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * num_partial, hipMemcpyDeviceToHost, st));
      HJ_HIP(ctx, hipMemsetAsync(t.info, 0, sizeof info, st));                // (the counts: the next attempt starts at zero)
      HJ_HIP(ctx, hipStreamSynchronize(st));
      HJ_HIP(ctx, hipGetLastError());
      if (info[ri::kInfoError]) return set_error(ctx, HJ_ERR_DEVICE, "hj_optimize_bvh_device: pass %u lost the tree (%u)", pass, info[ri::kInfoError]);
      moved = info[ri::kInfoMoves];
      holders = info[ri::kInfoHolders];
      clock.mark("apply, boxes, cost");
      area_sum = 0.0;
      for (double p : sums) area_sum += p;                    // index order: the same double for the same tree
      return HJ_OK;
    };
    double area_sum = 0.0;
    for (double p : sums) area_sum += p;                      // (of the input: read behind the synchronisation that followed k_ri_init)
    for (uint32_t pass = 0; pass < passes; pass++) {
      hipLaunchKernelGGL(ri::k_ri_search, grid_w, blk_w, 0, st, t);
      HJ_HIP(ctx, hipMemcpyAsync(save_parent, t.parent, link_bytes, hipMemcpyDeviceToDevice, st));
      HJ_HIP(ctx, hipMemcpyAsync(save_c0, t.c0, link_bytes, hipMemcpyDeviceToDevice, st));
      HJ_HIP(ctx, hipMemcpyAsync(save_c1, t.c1, link_bytes, hipMemcpyDeviceToDevice, st));
      clock.mark("search");
      uint32_t moved = 0, holders = 0;
      double now = 0.0;
      HJ_TRY(resolve(false, pass, moved, holders, now));
      const bool again = moved != 0 ? !(now < area_sum) : holders != 0;
      if (again) {                                            // taken back: the links (the boxes follow from them), then the strict rule
        HJ_HIP(ctx, hipMemcpyAsync(t.parent, save_parent, link_bytes, hipMemcpyDeviceToDevice, st));
        HJ_HIP(ctx, hipMemcpyAsync(t.c0, save_c0, link_bytes, hipMemcpyDeviceToDevice, st));
        HJ_HIP(ctx, hipMemcpyAsync(t.c1, save_c1, link_bytes, hipMemcpyDeviceToDevice, st));
        HJ_TRY(resolve(true, pass, moved, holders, now));
      }
      if (timing) std::fprintf(stderr, "hj_optimize_bvh_device: pass %u moved %u subtrees%s\n", pass, moved, again ? " (whole-path rule)" : "");
      moves += moved;
      if (moved == 0) break;
      area_sum = now;
    }
    if (moves != 0) {                                         // (no move: the resident records are the result, bit for bit)
      hj_bvh_node* d_flat = nullptr;
      HJ_TRY(bufs.alloc(d_flat, total));
      const uint32_t root_exit = total > HJ_BVH_ROOT_EXIT ? (uint32_t)total : HJ_BVH_ROOT_EXIT;
      hipLaunchKernelGGL(ri::k_ri_climb<true>, grid, blk, 0, st, t);
      hipLaunchKernelGGL(ri::k_ri_flatten, grid, blk, 0, st, t, root_exit, reinterpret_cast<float4*>(d_flat));
      HJ_HIP(ctx, hipGetLastError());
      clock.mark("flatten");
      hj_bvh_node* d_final = d_flat;
      const size_t vote_paths = scene ? (size_t)tn.lbvh_vote_paths : 0;
      if (vote_paths != 0) {                                  // (the moved parents hold (X, N): the voted order is gone there)
        hj_bvh_node* d_voted = nullptr;
        HJ_TRY(bufs.alloc(d_voted, total));
        const VoteShapes vsh{static_cast<const float4*>(rt.spheres.p), static_cast<const float4*>(rt.quads.p),
                             static_cast<const hj_triangle*>(rt.triangles.p), static_cast<const hj_vertex*>(rt.vertices.p)};
        const std::string error_before = get_error(ctx);
        const int rc = vote_on_device(ctx, scene, vsh, d_flat, total, vote_paths, d_voted, timing, nullptr);
        if (rc != HJ_OK && rc != HJ_ERR_UNSUPPORTED) return rc;
        if (rc == HJ_ERR_UNSUPPORTED) put_error(ctx, error_before);     // (a tree too deep for the exchange keeps the order it has)
        else d_final = d_voted;
        clock.mark("ray-voted child order");
      }
      refit_enqueue_cost(ctx, reinterpret_cast<const float4*>(d_final), N, d_partial);
      HJ_HIP(ctx, hipStreamSynchronize(st));
      HJ_HIP(ctx, hipGetLastError());
      double after = 0.0;
      HJ_TRY(read_cost(ctx, d_final, d_partial, num_partial, &after));
      if (out_after) *out_after = after;
      rt.nodes = bufs.take(d_final);                          // the optimised tree replaces the resident one; the shape arrays stay
      // the links a refit kept are no longer this tree's: a later refit with scene->bvh == NULL must not bring the old topology back
      hj_context::KeptLinks& kept = ctx->refit_links;
      kept.links.release(); kept.parent.release(); kept.arrived.release();
      kept.shapes = 0; kept.valid = false;
      clock.mark("cost of the result");
    }
  }
  if (out_nodes) HJ_HIP(ctx, hipMemcpy(out_nodes, rt.nodes.p, sizeof(hj_bvh_node) * total, hipMemcpyDeviceToHost));
  if (out_moves) *out_moves = moves;
  return HJ_OK;
}

}  // namespace

extern "C" {

// No counterpart upstream; host form: host/tree_opt.cpp optimize_by_reinsertion_batched (hjh_compiled_tune_bvh).
int hj_optimize_bvh_device(hj_context* ctx, const hj_scene_desc* scene, uint32_t passes, hj_bvh_node* out_nodes, size_t capacity,
                           size_t* out_num_nodes, double* out_cost_before, double* out_cost_after, uint32_t* out_moves) {
  if (passes > ri::kMaxPasses) return set_error(ctx, HJ_ERR_INVALID, "hj_optimize_bvh_device: %u passes, at most %u a call", passes, ri::kMaxPasses);
  if (!ctx) {
    if (hj_device_count() == 0) return set_error(nullptr, HJ_ERR_DEVICE, "hj_optimize_bvh_device: no HIP device available; this library has no CPU fallback");
    return set_error(nullptr, HJ_ERR_INVALID, "hj_optimize_bvh_device: null context");
  }
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  const hj_context::ResidentTree& rt = ctx->resident;
  if (!rt.valid) return set_error(ctx, HJ_ERR_STATE, "hj_optimize_bvh_device: no tree on the device (hj_build_bvh_device or hj_refit_bvh_device leaves one)");
  if (out_nodes && capacity < rt.total) return set_error(ctx, HJ_ERR_INVALID, "node buffer holds %zu records, the tree has %zu", capacity, rt.total);
  if (scene && (scene->num_spheres != rt.ns || scene->num_quads != rt.nq || scene->num_triangles != rt.nt))
    return set_error(ctx, HJ_ERR_INVALID, "hj_optimize_bvh_device: the scene has %zu spheres, %zu quads, %zu triangles, the tree on the device %zu, %zu, %zu",
                     scene->num_spheres, scene->num_quads, scene->num_triangles, rt.ns, rt.nq, rt.nt);
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const int rc = optimize_resident(ctx, scene, passes, out_nodes, out_cost_before, out_cost_after, out_moves);
  if (rc != HJ_OK) { ctx->resident.release(); return rc; }   // (as a failed refit: no tree is better than a doubtful one)
  if (out_num_nodes) *out_num_nodes = ctx->resident.total;
  return HJ_OK;
}

}  // extern "C"
