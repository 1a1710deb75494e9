// hj_tune_bvh_device and the host half of kernels/hj_vote.h: the child order of a flattened tree voted by sampled rays, on the device
// (host counterpart: host/tree_opt.cpp order_children_by_rays, hjh_compiled_tune_bvh).
#include "hj_internal.h"
#include "tree_vote.hpp"
#include "../kernels/hj_vote.h"

#pragma clang fp contract(off)

using namespace hjapi;

// hj_debug_vote_cast's kernel: one thread per caller-given ray; closest (or the caller's hit) and cast are the sampler's own
namespace hj {
namespace vote {

__global__ __launch_bounds__(64) void k_debug_cast(Scene s, const float4* __restrict__ rays, uint32_t n, const uint2* __restrict__ given, uint32_t any,
                                                   uint4* __restrict__ found) {
  const uint32_t index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= n) return;
  const float4 a = rays[2 * (size_t)index], b = rays[2 * (size_t)index + 1];
  Ray r;
  r.o = V(a.x, a.y, a.z); r.d = V(a.w, b.x, b.y); r.tmin = b.z; r.tmax = b.w;
  Hit h{-1, 0u, 0.f, 0.f, 0.f};
  if (given) {
    const uint2 g = given[index];                                          // (the host has refused positions that are no leaf)
    if (g.x < s.N) { h.pos = g.x; h.shape = (int)__float_as_uint(s.nodes[2 * (size_t)g.x].w); h.t = __uint_as_float(g.y); }
  } else {
    h = closest(s, r);
  }
  cast(s, r, h, any != 0u);
  found[index] = make_uint4(h.shape < 0 ? kNone : h.pos, (uint32_t)h.shape, __float_as_uint(h.t), 0u);
}

}  // namespace vote
}  // namespace hj

namespace hjapi {

namespace {

uint32_t vote_shadow_weight(const hj_context* ctx, size_t N) {
  return (uint32_t)Tuning::pick(ctx->tuning.bvh_vote_shadow, N >= (size_t)ctx->tuning.stream_min_nodes ? 4 : 1);
}

// What a vote's rays read, on the device: the caller's shape arrays and tree, the tags, emitters and dielectrics of `s` (uploaded here
// into `sc`), and two zeroed gain arrays of N words.
int vote_scene(hj_context* ctx, const hj_scene_desc* s, const VoteShapes& shapes, const hj_bvh_node* d_nodes, size_t N, uint32_t w_shadow, DevBufs& sc,
               hj::vote::Scene& vs) {
  hipStream_t st = ctx->stream;
  const size_t nshapes = s->num_spheres + s->num_quads + s->num_triangles;
  vs = hj::vote::Scene{};
  vs.spheres = shapes.spheres; vs.quads = shapes.quads; vs.triangles = shapes.triangles; vs.vertices = shapes.vertices;
  vs.ns = (uint32_t)s->num_spheres; vs.nq = (uint32_t)s->num_quads; vs.nt = (uint32_t)s->num_triangles;
  vs.cam = s->camera;
  vs.nodes = reinterpret_cast<const float4*>(d_nodes);
  vs.N = (uint32_t)N;
  vs.w_shadow = w_shadow;
  if (s->materials && s->num_materials == nshapes && nshapes) {
    uint32_t* m = nullptr;
    HJ_TRY(sc.alloc(m, nshapes));
    HJ_HIP(ctx, hipMemcpyAsync(m, s->materials, sizeof(uint32_t) * nshapes, hipMemcpyHostToDevice, st));
    vs.materials = m;
  }
  if (s->emitters && s->num_emitters) {
    hj_emitter* e = nullptr;
    HJ_TRY(sc.alloc(e, s->num_emitters));
    HJ_HIP(ctx, hipMemcpyAsync(e, s->emitters, sizeof(hj_emitter) * s->num_emitters, hipMemcpyHostToDevice, st));
    vs.emitters = e; vs.ne = (uint32_t)std::min<size_t>(s->num_emitters, 0x7FFFFFFFu);
  }
  if (s->dielectric && s->num_dielectric) {
    hj_dielectric* d = nullptr;
    HJ_TRY(sc.alloc(d, s->num_dielectric));
    HJ_HIP(ctx, hipMemcpyAsync(d, s->dielectric, sizeof(hj_dielectric) * s->num_dielectric, hipMemcpyHostToDevice, st));
    vs.dielectric = d; vs.ndielectric = (uint32_t)std::min<size_t>(s->num_dielectric, 0x7FFFFFFFu);
  }
  HJ_TRY(sc.alloc(vs.gain_l, N));
  HJ_TRY(sc.alloc(vs.gain_r, N));
  HJ_HIP(ctx, hipMemsetAsync(vs.gain_l, 0, sizeof(unsigned long long) * N, st));
  HJ_HIP(ctx, hipMemsetAsync(vs.gain_r, 0, sizeof(unsigned long long) * N, st));
  return HJ_OK;
}

// The shape arrays and the tree of a host-side scene description, copied into buffers of `sc`
int upload_vote_inputs(hj_context* ctx, const hj_scene_desc* s, DevBufs& sc, VoteShapes& shapes, hj_bvh_node*& d_nodes) {
  hipStream_t st = ctx->stream;
  const size_t N = s->num_bvh_nodes;
  float4 *sp = nullptr, *qd = nullptr;
  hj_triangle* tr = nullptr;
  hj_vertex* vx = nullptr;
  HJ_TRY(sc.alloc(sp, s->num_spheres));
  HJ_TRY(sc.alloc(qd, 3 * s->num_quads));
  HJ_TRY(sc.alloc(tr, s->num_triangles));
  HJ_TRY(sc.alloc(vx, s->num_vertices));
  HJ_TRY(sc.alloc(d_nodes, N));
  if (s->num_spheres) HJ_HIP(ctx, hipMemcpyAsync(sp, s->spheres, sizeof(float4) * s->num_spheres, hipMemcpyHostToDevice, st));
  if (s->num_quads) HJ_HIP(ctx, hipMemcpyAsync(qd, s->quads, sizeof(float4) * 3 * s->num_quads, hipMemcpyHostToDevice, st));
  if (s->num_triangles) HJ_HIP(ctx, hipMemcpyAsync(tr, s->triangles, sizeof(hj_triangle) * s->num_triangles, hipMemcpyHostToDevice, st));
  if (s->num_vertices) HJ_HIP(ctx, hipMemcpyAsync(vx, s->vertices, sizeof(hj_vertex) * s->num_vertices, hipMemcpyHostToDevice, st));
  HJ_HIP(ctx, hipMemcpyAsync(d_nodes, s->bvh, sizeof(hj_bvh_node) * N, hipMemcpyHostToDevice, st));
  shapes = VoteShapes{sp, qd, tr, vx};
  return HJ_OK;
}

}  // namespace

int vote_sample(hj_context* ctx, const hj_scene_desc* s, const VoteShapes& shapes, const hj_bvh_node* d_nodes, size_t N, size_t paths, DevBufs& sc,
                VoteGains& gains, StageClock* clock) {
  hj::vote::Scene vs;
  HJ_TRY(vote_scene(ctx, s, shapes, d_nodes, N, vote_shadow_weight(ctx, N), sc, vs));
  gains = VoteGains{vs.gain_l, vs.gain_r};
  if (clock) clock->mark("uploads");
  const uint32_t np = (uint32_t)std::min<size_t>(paths, (size_t)1 << 24);
  if (np) hipLaunchKernelGGL(hj::vote::k_vote_paths, dim3((np + 63u) / 64u), dim3(64), 0, ctx->stream, vs, np);
  if (clock) clock->mark("sampled paths");
  return HJ_OK;
}

int vote_exchange(hj_context* ctx, const hj_bvh_node* d_nodes, size_t N, const unsigned long long* gain_l, const unsigned long long* gain_r,
                  hj_bvh_node* d_out, uint32_t info[4]) {
  hipStream_t st = ctx->stream;
  info[0] = info[1] = info[2] = info[3] = 0;
  if (N < 3) {
    HJ_HIP(ctx, hipMemcpyAsync(d_out, d_nodes, sizeof(hj_bvh_node) * N, hipMemcpyDeviceToDevice, st));
    return HJ_OK;
  }
  DevBufs sc(ctx);
  hj::vote::Reorder r{};
  r.in = reinterpret_cast<const float4*>(d_nodes); r.out = reinterpret_cast<float4*>(d_out); r.N = (uint32_t)N; r.gain_l = gain_l; r.gain_r = gain_r;
  HJ_TRY(sc.alloc(r.depth, N));
  HJ_TRY(sc.alloc(r.npos, N));
  HJ_TRY(sc.alloc(r.nexit, N));
  HJ_TRY(sc.alloc(r.info, 4));
  HJ_HIP(ctx, hipMemsetAsync(r.info, 0, sizeof(uint32_t) * 4, st));
  const dim3 blk(256), grid((r.N + 255u) / 256u);
  hipLaunchKernelGGL(hj::vote::k_ro_init, grid, blk, 0, st, r);
  for (uint32_t L = 0; L < hj::vote::kMaxLevels; L += 16) {       // (the levels end when one has no inner node)
    for (uint32_t k = 0; k < 16; k++) hipLaunchKernelGGL(hj::vote::k_ro_level, grid, blk, 0, st, r, L + k);
    HJ_HIP(ctx, hipMemcpyAsync(info, r.info, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, st));
    HJ_HIP(ctx, hipStreamSynchronize(st));
    if (info[0] < L + 16) break;
  }
  hipLaunchKernelGGL(hj::vote::k_ro_scatter, grid, blk, 0, st, r);
  HJ_HIP(ctx, hipMemcpyAsync(info, r.info, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));
  HJ_HIP(ctx, hipGetLastError());
  if (info[2] & 1u) return set_error(ctx, HJ_ERR_INVALID, "ray-voted child order: the array is not a pre-order skip-link tree");
  if (info[2] & 2u) return set_error(ctx, HJ_ERR_UNSUPPORTED, "ray-voted child order: the tree is deeper than %u levels", hj::vote::kMaxLevels);
  return HJ_OK;
}

int vote_on_device(hj_context* ctx, const hj_scene_desc* s, const VoteShapes& shapes, const hj_bvh_node* d_nodes, size_t N, size_t paths,
                   hj_bvh_node* d_out, bool timing, VoteResult* result) {
  hipStream_t st = ctx->stream;
  if (result) *result = VoteResult{};
  if (N < 3 || paths == 0) {
    HJ_HIP(ctx, hipMemcpyAsync(d_out, d_nodes, sizeof(hj_bvh_node) * N, hipMemcpyDeviceToDevice, st));
    return HJ_OK;
  }
  if (N >= 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_UNSUPPORTED, "tree of %zu records: too large for the device vote", N);
  paths = std::min<size_t>(paths, (size_t)1 << 24);
  StageClock clock{timing, "ray-voted child order (device): %-20s %8.2f ms\n", st};
  DevBufs sc(ctx);
  VoteGains gains{};
  HJ_TRY(vote_sample(ctx, s, shapes, d_nodes, N, paths, sc, gains, &clock));
  uint32_t info[4];
  HJ_TRY(vote_exchange(ctx, d_nodes, N, gains.l, gains.r, d_out, info));
  clock.mark("exchange");
  if (result) { result->exchanged = info[1]; result->levels = info[0]; }
  if (timing) std::fprintf(stderr, "ray-voted child order (device): %zu paths, %u of %zu inner nodes exchanged, %u levels\n", paths, info[1], N / 2, info[0]);
  return HJ_OK;
}

int put_records(hj_context* ctx, const std::vector<std::pair<uint32_t, hj_bvh_node>>& records, hj_bvh_node* d_array) {
  if (records.empty()) return HJ_OK;
  hipStream_t st = ctx->stream;
  DevBufs sc(ctx);
  std::vector<uint32_t> pos(records.size());
  std::vector<hj_bvh_node> rec(records.size());
  for (size_t k = 0; k < records.size(); k++) { pos[k] = records[k].first; rec[k] = records[k].second; }
  uint32_t* d_pos = nullptr;
  hj_bvh_node* d_rec = nullptr;
  HJ_TRY(sc.alloc(d_pos, pos.size()));
  HJ_TRY(sc.alloc(d_rec, rec.size()));
  HJ_HIP(ctx, hipMemcpyAsync(d_pos, pos.data(), sizeof(uint32_t) * pos.size(), hipMemcpyHostToDevice, st));
  HJ_HIP(ctx, hipMemcpyAsync(d_rec, rec.data(), sizeof(hj_bvh_node) * rec.size(), hipMemcpyHostToDevice, st));
  const uint32_t n = (uint32_t)records.size();
  hipLaunchKernelGGL(hj::vote::k_put_records, dim3((n + 255u) / 256u), dim3(256), 0, st, d_pos, reinterpret_cast<const float4*>(d_rec), n,
                     reinterpret_cast<float4*>(d_array));
  HJ_HIP(ctx, hipStreamSynchronize(st));                         // (the staging vectors and buffers live on this frame)
  return HJ_OK;
}

}  // namespace hjapi

extern "C" {

// No counterpart upstream (the reference walks the tree the `bvh` crate hands it, src/main.rs:199-231); host form: hjh_compiled_tune_bvh.
int hj_tune_bvh_device(hj_context* ctx, const hj_scene_desc* s, hj_bvh_node* out_nodes, size_t capacity, size_t vote_paths) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!s || !out_nodes) return set_error(ctx, HJ_ERR_INVALID, "null argument");
  const size_t N = s->num_bvh_nodes;
  if (capacity < N) return set_error(ctx, HJ_ERR_INVALID, "node buffer holds %zu records, the tree has %zu", capacity, N);
  int rc = validate_scene(ctx, s, (size_t)HJ_MATERIAL_INDEX_MASK + 1);   // (the vote reads the tags of textured materials, not their textures)
  if (rc != HJ_OK) return rc;
  if (N == 0) return HJ_OK;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const Tuning tn = ctx->tuning = Tuning::from_env();
  const bool timing = tn.lbvh_timing != 0;
  hipStream_t st = ctx->stream;
  DevBufs sc(ctx);
  VoteShapes shapes{};
  hj_bvh_node *d_in = nullptr, *d_out = nullptr;
  HJ_TRY(upload_vote_inputs(ctx, s, sc, shapes, d_in));
  HJ_TRY(sc.alloc(d_out, N));
  rc = vote_on_device(ctx, s, shapes, d_in, N, vote_paths, d_out, timing, nullptr);
  if (rc != HJ_OK) return rc;
  HJ_HIP(ctx, hipMemcpyAsync(out_nodes, d_out, sizeof(hj_bvh_node) * N, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));
  return HJ_OK;
}

}  // extern "C"

// ---- the vote's probes: its two stages apart, on caller-given inputs (include/hijiki_hip.h)

namespace {

// what the three probes refuse of a scene and of the gain arrays that receive one word per record of its tree
int vote_probe_scene_check(hj_context* ctx, const char* fn, const hj_scene_desc* s, const void* gain_l, const void* gain_r, size_t capacity) {
  if (!s || !gain_l || !gain_r) return set_error(ctx, HJ_ERR_INVALID, "%s: null argument", fn);
  const size_t N = s->num_bvh_nodes;
  if (N == 0) return set_error(ctx, HJ_ERR_INVALID, "%s: the scene has no tree", fn);
  if (capacity < N) return set_error(ctx, HJ_ERR_INVALID, "%s: the gain arrays hold %zu words, the tree has %zu records", fn, capacity, N);
  return validate_scene(ctx, s, (size_t)HJ_MATERIAL_INDEX_MASK + 1);   // (as hj_tune_bvh_device)
}

int debug_vote_cast(hj_context* ctx, const hj_scene_desc* s, const float* rays, size_t n, bool any, uint32_t w_shadow, const uint32_t* given,
                    uint64_t* gain_l, uint64_t* gain_r, uint32_t* found) {
  hipStream_t st = ctx->stream;
  const size_t N = s->num_bvh_nodes;
  DevBufs sc(ctx);
  VoteShapes shapes{};
  hj_bvh_node* d_nodes = nullptr;
  HJ_TRY(upload_vote_inputs(ctx, s, sc, shapes, d_nodes));
  hj::vote::Scene vs;
  HJ_TRY(vote_scene(ctx, s, shapes, d_nodes, N, w_shadow, sc, vs));
  float4* d_rays = nullptr;
  uint2* d_given = nullptr;
  uint4* d_found = nullptr;
  HJ_TRY(sc.alloc(d_rays, 2 * n));
  HJ_TRY(sc.alloc(d_found, n));
  HJ_HIP(ctx, hipMemcpyAsync(d_rays, rays, sizeof(float4) * 2 * n, hipMemcpyHostToDevice, st));
  if (given) {
    HJ_TRY(sc.alloc(d_given, n));
    HJ_HIP(ctx, hipMemcpyAsync(d_given, given, sizeof(uint2) * n, hipMemcpyHostToDevice, st));
  }
  const uint32_t cnt = (uint32_t)n;
  hipLaunchKernelGGL(hj::vote::k_debug_cast, dim3((cnt + 63u) / 64u), dim3(64), 0, st, vs, d_rays, cnt, d_given, any ? 1u : 0u, d_found);
  HJ_HIP(ctx, hipGetLastError());
  HJ_HIP(ctx, hipMemcpyAsync(gain_l, vs.gain_l, sizeof(uint64_t) * N, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipMemcpyAsync(gain_r, vs.gain_r, sizeof(uint64_t) * N, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipMemcpyAsync(found, d_found, sizeof(uint4) * n, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));                          // (the buffers of `sc` live on this frame)
  return HJ_OK;
}

int debug_vote_exchange(hj_context* ctx, const hj_bvh_node* nodes, size_t N, const uint64_t* gain_l, const uint64_t* gain_r, hj_bvh_node* out_nodes,
                        uint32_t info[4]) {
  hipStream_t st = ctx->stream;
  DevBufs sc(ctx);
  hj_bvh_node *d_in = nullptr, *d_out = nullptr;
  unsigned long long *d_l = nullptr, *d_r = nullptr;
  HJ_TRY(sc.alloc(d_in, N));
  HJ_TRY(sc.alloc(d_out, N));
  HJ_TRY(sc.alloc(d_l, N));
  HJ_TRY(sc.alloc(d_r, N));
  HJ_HIP(ctx, hipMemcpyAsync(d_in, nodes, sizeof(hj_bvh_node) * N, hipMemcpyHostToDevice, st));
  HJ_HIP(ctx, hipMemcpyAsync(d_l, gain_l, sizeof(uint64_t) * N, hipMemcpyHostToDevice, st));
  HJ_HIP(ctx, hipMemcpyAsync(d_r, gain_r, sizeof(uint64_t) * N, hipMemcpyHostToDevice, st));
  HJ_TRY(vote_exchange(ctx, d_in, N, d_l, d_r, d_out, info));
  HJ_HIP(ctx, hipMemcpyAsync(out_nodes, d_out, sizeof(hj_bvh_node) * N, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));
  return HJ_OK;
}

int debug_vote_gains(hj_context* ctx, const hj_scene_desc* s, size_t paths, uint64_t* gain_l, uint64_t* gain_r) {
  hipStream_t st = ctx->stream;
  const size_t N = s->num_bvh_nodes;
  DevBufs sc(ctx);
  VoteShapes shapes{};
  hj_bvh_node* d_nodes = nullptr;
  HJ_TRY(upload_vote_inputs(ctx, s, sc, shapes, d_nodes));
  VoteGains gains{};
  HJ_TRY(vote_sample(ctx, s, shapes, d_nodes, N, N < 3 ? 0 : paths, sc, gains, nullptr));   // (vote_on_device samples no tree of fewer than 3 records)
  HJ_HIP(ctx, hipGetLastError());
  HJ_HIP(ctx, hipMemcpyAsync(gain_l, gains.l, sizeof(uint64_t) * N, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipMemcpyAsync(gain_r, gains.r, sizeof(uint64_t) * N, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));
  return HJ_OK;
}

}  // namespace

extern "C" {

int hj_debug_vote_cast(hj_context* ctx, const hj_scene_desc* s, const float* rays, size_t n, uint32_t any_hit, uint32_t w_shadow, const uint32_t* given_hits,
                       uint64_t* gain_l, uint64_t* gain_r, size_t capacity, uint32_t* found) {
  HJ_TRY(vote_probe_scene_check(ctx, __func__, s, gain_l, gain_r, capacity));
  if (!rays || !found) return set_error(ctx, HJ_ERR_INVALID, "%s: null argument", __func__);
  if (n == 0 || n > HJ_VOTE_MAX_RAYS) return set_error(ctx, HJ_ERR_INVALID, "%s: %zu rays, 1 ... %u a call", __func__, n, (unsigned)HJ_VOTE_MAX_RAYS);
  if (w_shadow > 16u) return set_error(ctx, HJ_ERR_INVALID, "%s: w_shadow %u, at most 16 (HJ_BVH_VOTE_SHADOW's range)", __func__, w_shadow);
  const size_t N = s->num_bvh_nodes;
  if (given_hits)
    for (size_t i = 0; i < n; i++) {
      const uint32_t pos = given_hits[2 * i];
      if (pos == 0xFFFFFFFFu) continue;                              // (a miss)
      if (pos >= N) return set_error(ctx, HJ_ERR_INVALID, "%s: ray %zu is given a hit in record %u of %zu", __func__, i, pos, N);
      if (s->bvh[pos].shape_index == HJ_BVH_INNER) return set_error(ctx, HJ_ERR_INVALID, "%s: ray %zu is given a hit in record %u, which is no leaf", __func__, i, pos);
    }
  HJ_TRY(context_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  return drain(ctx, __func__, debug_vote_cast(ctx, s, rays, n, any_hit != 0u, w_shadow, given_hits, gain_l, gain_r, found));
}

int hj_debug_vote_exchange(hj_context* ctx, const hj_bvh_node* nodes, size_t N, const uint64_t* gain_l, const uint64_t* gain_r, hj_bvh_node* out_nodes,
                           size_t capacity, uint32_t info[4]) {
  if (!nodes || !gain_l || !gain_r || !out_nodes || !info) return set_error(ctx, HJ_ERR_INVALID, "%s: null argument", __func__);
  if (N == 0 || N >= 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "%s: %zu records, 1 ... 2^31 - 2 a call", __func__, N);
  if (capacity < N) return set_error(ctx, HJ_ERR_INVALID, "%s: node buffer holds %zu records, the tree has %zu", __func__, capacity, N);
  HJ_TRY(validate_tree_links(ctx, nodes, N));                     // (the exchange sizes its writes by the links: the device never sees others)
  HJ_TRY(context_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  return drain(ctx, __func__, debug_vote_exchange(ctx, nodes, N, gain_l, gain_r, out_nodes, info));
}

int hj_debug_vote_gains(hj_context* ctx, const hj_scene_desc* s, size_t paths, uint64_t* gain_l, uint64_t* gain_r, size_t capacity) {
  HJ_TRY(vote_probe_scene_check(ctx, __func__, s, gain_l, gain_r, capacity));
  HJ_TRY(context_gate(ctx, __func__));
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  ctx->tuning = Tuning::from_env();
  return drain(ctx, __func__, debug_vote_gains(ctx, s, paths, gain_l, gain_r));
}

}  // extern "C"
