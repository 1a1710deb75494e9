// Internals shared by the translation units of libhijiki_hip.so (api/*.hip): the context object, device buffers and the
// small helpers every entry point uses.  Nothing here is part of the C ABI (include/hijiki_hip.h).
//
//   api/context.hip       context create / destroy, framebuffer, errors, environment switches, ensure_path_state: the arrays of a
//                         batch's path state (PathState, batch_arrays below) for the slots, the path query and the shade probe  (no kernels)
//   api/scene_upload.hip  hj_scene_upload: validation, host re-layout, emitter records, light grid; one commit at the end  (no kernels)
//   api/scene_relayout.hip the same re-layout on the device (large trees, the tree hj_build_bvh_device left there)
//   api/render.hip        the launches of kernels/hj_kernels.h (the only unit that includes them), walk-statistics readers
//   api/render_calls.hip  batch slots, render calls, hj_reserve, the pipeline, the worker thread, probes (hj_debug_trace,
//                         hj_debug_samples, hj_debug_reconstruct)                                        (no kernels)
//   api/comm.hip          RCCL (dlopen), hj_comm_*, hj_reduce_framebuffers
//   api/lbvh_build.hip    hj_build_bvh_device, hj_refit_bvh_device: host half of kernels/hj_lbvh.h (the only unit that includes it;
//                         api/refit_pass.hpp: the refit's stages for a caller that brings its own link set)
//   api/scene_update.hip  hj_scene_update_shapes: the uploaded scene's boxes, triangle and emitter records recomputed in place
//   api/tree_vote.hip     hj_tune_bvh_device: host half of kernels/hj_vote.h (child order voted by sampled rays)
//                         and its probes hj_debug_vote_cast / _exchange / _gains (k_debug_cast: the vote's closest and cast on given rays)
//   api/tree_reinsert.hip hj_optimize_bvh_device: the tree left on the device optimised by parallel reinsertion (its kernels, around the
//                         per-node steps of api/tree_reinsert.h; includes no kernel header but hj_num.h's)
//   api/texture.hip       image textures: the checks and the device buffer of hj_scene_upload_textured, hj_debug_texture_lookup
//   api/environment.hip   environment lighting: the checks and the alias table of hj_scene_upload_env, hj_debug_env_*
//   api/step_probe.hip    hj_debug_num: the functions of kernels/hj_num.h on caller-given inputs (includes no other kernel header);
//                         hj_debug_shade_step: one launch_shade over a fabricated batch in a PathState of its own  (host code)
//   api/ray_query.hip     hj_trace_rays: caller-given rays through the uploaded tree (includes the kernel headers up to hj_stages.h and
//                         defines its own kernels beside the path kernels: the persistent walk with a fetch / finish of its own)
//   api/path_query.hip    hj_trace_paths: path-traced radiance along caller-given rays (includes the kernel headers up to hj_stages.h and
//                         defines its own kernels beside the path kernels: the round loop of api/query_round_loop.h with a top-up from a
//                         ray array); its path state is hj_context::PathQuery, a PathState.  Also the host code the queries share:
//                         path_query_plan / path_query_pass, query_render_opts, query_gate, per_lane, QueryStats, fixed_spp_query (below)
//   api/query_round.h     the tail threshold, register budget and group deal of the queries' path kernels
//   api/query_round_loop.h the text of their round loop: no include guard, included inside the bodies of k_pq_paths and k_gq_paths
//   api/path_adaptive.hip hj_trace_paths_adaptive: rounds of that path kernel (path_query_pass) over the rays still active, with the
//                         k_pa_* kernels between them (running sums and stop rule; the order-preserving compaction is
//                         kernels/hj_compact.h's text); includes that header and hj_num.h only.  Also adaptive_query (below), the
//                         round loop both adaptive queries enter
//   api/adaptive_stop.h   the stop rule of the adaptive queries (pa_stops): one text for k_pa_accumulate and k_ga_accumulate
//   api/gather_query.hip  hj_trace_irradiance: gather queries at caller-given points (includes the kernel headers up to hj_stages.h and
//                         defines its own kernels beside the path kernels: the same round loop with a top-up that draws a direction
//                         at a point, and the per-point reduction); its host half behind the checks is fixed_spp_query
//   api/gather_adaptive.hip hj_trace_irradiance_adaptive: adaptive_query over gather points (gather_query_pass for a round's launches,
//                         k_ga_accumulate between them: the running sums with the first segments' hit count and nearest hit), and
//                         k_ga_scatter, the scatter of hj_bake_lightmap_adaptive with its per-texel scale and sample map (includes
//                         adaptive_stop.h and hj_num.h only)
//   api/lightmap.hip      hj_lightmap_texels, hj_bake_lightmap: the uploaded triangles' UVs rasterised into gather points, the gather's
//                         records scattered into an atlas and dilated (includes kernels/hj_lightmap.h; beside it hj_compact.h and
//                         hj_num.h alone: the path kernels' machine code does not depend on it).  The gather itself is
//                         hj_trace_irradiance's, entered through that entry point with device arrays.  hj_bake_lightmap_filtered: the same
//                         host routine with the filter between scatter and dilation; hj_bake_lightmap_adaptive: the same routine
//                         with hj_trace_irradiance_adaptive as its gather and api/gather_adaptive.hip's scatter
//   api/lightmap_filter.hip hj_filter_lightmap: the edge-avoiding a-trous filter over an atlas, and lightmap_filter_check /
//                         lightmap_filter_enqueue (below) for the bake (includes kernels/hj_lightmap_filter.h and hj_num.h alone)
//   api/probe_volume.hip  hj_probe_points, hj_bake_probes, hj_sample_probes: a grid of probes as gather points, the sphere gather's SH
//                         sums resolved to irradiance coefficients with a validity weight (k_pv_points, k_pv_resolve; the gather is
//                         hj_trace_irradiance's, entered through that entry point with device arrays), and the trilinear look-up of a
//                         volume at caller-given points (includes kernels/hj_probes.h; beside it hj_sh9.h - the SH basis, which
//                         api/gather_query.hip includes too - and hj_num.h alone); probe_desc_check (below) for the unit behind it
//   api/probe_visibility.hip hj_probe_visibility_rays, hj_bake_probe_visibility, hj_sample_probes_visible: per probe an octahedral
//                         atlas of distance moments - in slabs: k_pvv_rays, hj_trace_rays through that entry point with device arrays,
//                         k_pvv_reduce - and the look-up with back-face and Chebyshev weights (includes kernels/hj_probe_vis.h; beside
//                         it hj_probes.h, hj_sh9.h and hj_num.h alone); probe_vis_bake_check, probe_vis_rays_enqueue (below)
//   api/probe_update.hip  hj_update_probes, hj_update_probe_visibility: a window of probes re-baked under a frame's seeds and folded
//                         into what the caller holds - k_pv_points and hj_trace_irradiance, then k_pu_resolve (resolve and blend in
//                         one pass); per slab k_pvv_rays and hj_trace_rays, then k_pu_reduce (moments, blend and border in one pass)
//                         (includes kernels/hj_probe_update.h; beside it the functions of hj_probes.h and hj_probe_vis.h, without
//                         their kernels, and hj_num.h alone)
//   api/probe_place.hip   hj_place_probes: per probe an offset and an active / inactive state from a slab's rays, hits and surface
//                         records (k_pp_rays, hj_trace_rays, k_pp_reduce: one wave per probe); hj_update_probes_placed,
//                         hj_update_probe_visibility_placed: the updates over the window's active probes, compacted in order
//                         (k_pp_count, k_pp_scan, k_pp_scatter; k_pp_points, k_pp_resolve; k_pp_rays, k_pp_blend);
//                         hj_sample_probes_visible_placed (k_pp_sample) (includes kernels/hj_probe_place.h; beside it the functions
//                         of hj_probe_update.h, hj_probe_vis.h and hj_probes.h without their kernels, hj_compact.h and hj_num.h alone)
//   api/closest_query.hip hj_closest_points, hj_distance_field: the nearest surface point to caller-given points, one lane per point
//                         over the second copy of the uploaded tree (k_cq_walk), and a grid of such distances (k_pv_points through
//                         probe_points_enqueue, k_cq_pack, k_cq_walk, k_cq_resolve) (includes kernels/hj_closest.h; beside it
//                         hj_intersect.h, the grid struct of hj_probes.h and hj_num.h alone)
//   api/multi_hit.hip     hj_trace_rays_all, hj_points_inside: every hit along caller-given rays, one lane per ray over the second
//                         copy of the uploaded tree with the range never shrunk (k_mh_walk: the K nearest in LDS, the count, the
//                         signed crossing sum), and containment of points by three such counts (k_mh_inside) (includes
//                         kernels/hj_multihit.h; beside it hj_intersect.h and hj_num.h alone)
//   api/aov.hip           hj_eval_materials, hj_render_aovs, hj_render_aovs_frame: the material of (hit, surface) records, and a
//                         frame's albedo / normal / depth sums from its own primary rays (includes kernels/hj_aov.h, which includes
//                         the kernel headers up to hj_stages.h and edits none: k_mat_eval; k_aov_walk, the persistent walk with a
//                         fetch that builds the camera ray from the sample index; k_aov_resolve, run by run of disjoint blocks)
//   api/follow.hip        hj_follow_specular, and the follow rounds of hj_render_aovs_followed / hj_render_aovs_frame_followed (whose entry
//                         points, checks and camera walk are api/aov.hip's): the chain through mirror and glass as a deterministic
//                         query (includes kernels/hj_follow.h, which includes hj_aov.h and hj_chain.h and edits none: k_follow;
//                         k_chain_count / k_chain_scan - the one copy, chain_count_enqueue below - and k_af_scatter, the live chains
//                         in order; k_aov_follow, the persistent walk with a fetch that continues a chain from its state;
//                         k_aov_resolve_followed)
//   api/chain_rounds.h    the host side of a chain's rounds for api/follow.hip and api/motion_follow.hip: ChainBufs' reserve and the
//                         loop count -> scan -> live count to the host -> scatter -> round (the kernels' shared bodies:
//                         kernels/hj_chain.h, on kernels/hj_walk_segment.h, the shell of the flat segment walks)
//   api/probe_lit.hip     hj_render_probe_lit, hj_render_probe_lit_frame: hj_render_aovs_followed's samples lit at their last diffuse hit by a
//                         probe volume - aov_render (api/aov.hip) with an AovStage: behind each walk launch and its follow rounds
//                         k_pl_points, the volume's own look-up kernel over those points (probe_sample_enqueue,
//                         probe_vis_sample_enqueue: the units that hold the kernels launch them) and per run k_pl_resolve (includes
//                         kernels/hj_probe_lit.h, which includes hj_follow.h without its kernels and edits none); for the next unit the
//                         stage's volume, its checks, staging, reserve and points hook (api/probe_lit_volume.h)
//   api/direct_lit.hip    hj_render_direct_lit, hj_render_direct_lit_frame: the probe-lit frame with one traced next-event sample at each
//                         chain's last diffuse hit - the same AovStage with, behind lit_points, k_dl_sample, the compaction of the
//                         slots that want a shadow ray (k_dl_count, k_dl_scan, the count to the host, k_dl_scatter), k_dl_shadow over
//                         the list and per run k_dl_resolve (includes kernels/hj_direct_lit.h, which includes hj_probe_lit.h without
//                         its kernels and edits none)
//   api/denoise.hip       hj_denoise_frame: the variance-guided a-trous filter over a frame's albedo-demodulated light, guided by the
//                         frame's AOV sums (includes kernels/hj_denoise.h and hj_num.h alone: k_dn_prepare, k_dn_variance, the
//                         iteration as k_dn_filter_lds or k_dn_filter_direct, k_dn_finish); the checks, the buffers, the prepare
//                         stage and the iterations for both denoiser calls (denoise_check ... denoise_filter_enqueue below)
//   api/denoise_temporal.hip  hj_denoise_frame_temporal: reprojected history in front of that filter - k_dt_accumulate (reproject, blend,
//                         history record), k_dt_variance (spatial or temporal variance), k_dt_feedback (the first iteration's light
//                         into the history) between api/denoise.hip's stages (includes kernels/hj_denoise_temporal.h; beside it the
//                         functions of hj_denoise.h, without its kernels, and hj_num.h alone); hj_denoise_frame_temporal_motion: the same
//                         host routine with k_dt_accumulate<true>, which api/motion.hip instantiates (dt_accumulate_motion_enqueue below)
//   api/motion.hip        hj_render_motion: per pixel where the surface point its centre ray sees was in the previous frame - k_mv_walk,
//                         the persistent walk with a fetch that builds the centre ray from the pixel, its raw hit into the pixel's
//                         record; k_mv_resolve, the previous point from the previous shape arrays projected into the previous camera,
//                         in place (includes kernels/hj_motion.h, which includes the kernel headers up to hj_stages.h and the functions
//                         of hj_denoise_temporal.h and edits none); and the one instantiation of k_dt_accumulate<true>; motion_render, the
//                         host routine of both motion calls
//   api/motion_follow.hip hj_render_motion_followed: the motion image through mirrors and glass - between k_mv_walk and the resolve the
//                         rounds api/follow.hip's count and scan, k_mf_scatter, the live pixels in order, and k_mf_follow, the
//                         persistent walk with a fetch that continues a chain from its state and carries the product of its
//                         reflections; k_mf_resolve (includes kernels/hj_motion_follow.h, which includes hj_motion.h and hj_chain.h
//                         without their kernels and edits none)
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/hijiki_hip.h"
#include "hj_tuning.h"
#include "../host/blockgen.hpp"
#include "../kernels/hj_device.h"

namespace hjapi {

extern std::atomic<size_t> g_dev_bytes;   // device memory held through DevBuf by every context of the process

// One device allocation and its owner: move-only, freed by release() or with the object.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(bytes, o.bytes); } return *this; }
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      (void)hipFree(p);
      g_dev_bytes.fetch_sub(bytes, std::memory_order_relaxed);
    }
    p = nullptr;
    bytes = 0;
  }
};

int dev_alloc(hj_context* ctx, DevBuf& b, size_t bytes);

// The buffers of a specular chain's rounds over n slots (api/chain_rounds.h): per slot the chain state (32 bytes) and the list of
// live slots (4 bytes), and a count per tile of 256 slots with the total behind them.
struct ChainBufs { DevBuf state, counts, list; };

// The device buffers a call (or the scene, or a batch slot) owns: freed together with the set unless moved on first - a call
// allocates into a set of its own and hands it over when everything it needed has succeeded.  ctx: where allocation errors go
// (a set that only receives buffers needs none).
struct DevBufs {
  hj_context* ctx = nullptr;
  std::vector<DevBuf> bufs;
  explicit DevBufs(hj_context* c = nullptr) : ctx(c) {}
  // `count` elements of T, at least 16 bytes, plus `slack` bytes
  template <class T>
  int alloc(T*& out, size_t count, size_t slack = 0) {
    bufs.emplace_back();
    const int rc = dev_alloc(ctx, bufs.back(), std::max<size_t>(sizeof(T) * count + slack, 16));
    out = static_cast<T*>(bufs.back().p);
    return rc;
  }
  DevBuf take(const void* p) {                        // moves the buffer that starts at p out of the set (none: an empty DevBuf)
    DevBuf out;
    for (auto& b : bufs) if (p && b.p == p) { out = std::move(b); break; }
    return out;
  }
  void move_into(DevBufs& to) {                       // every buffer of this set joins `to`
    for (auto& b : bufs) if (b.p) to.bufs.push_back(std::move(b));
    bufs.clear();
  }
  void clear() { bufs.clear(); }
};

// Pinned host staging of `count` Ts: move-only, freed with the object; grow-only like dev_alloc.
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t count = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), count(o.count) { o.p = nullptr; o.count = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(count, o.count); } return *this; }
  ~PinnedBuf() { release(); }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; count = 0; }
  // room for `need` Ts: a buffer that is too small is replaced by one of max(need, grow) Ts
  hipError_t reserve(size_t need, size_t grow = 0) {
    if (p && count >= need) return hipSuccess;
    release();
    const size_t n = std::max(need, grow);
    const hipError_t e = hipHostMalloc((void**)&p, sizeof(T) * n, hipHostMallocDefault);
    if (e == hipSuccess) count = n; else p = nullptr;
    return e;
  }
};

// One HIP stream or event and its owner: move-only, destroyed with the object.  Created through out(), used as the handle.
template <class H, hipError_t (*destroy)(H)>
struct HipHandle {
  H h = nullptr;
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
  HipHandle& operator=(HipHandle&& o) noexcept { if (this != &o) { reset(); std::swap(h, o.h); } return *this; }
  ~HipHandle() { reset(); }
  void reset() { if (h) (void)destroy(h); h = nullptr; }
  H* out() { reset(); return &h; }                    // for hipStreamCreate* / hipEventCreate*
  operator H() const { return h; }
};
using Stream = HipHandle<hipStream_t, hipStreamDestroy>;
using Event = HipHandle<hipEvent_t, hipEventDestroy>;

// HJ_*_TIMING: a call's stage times on stderr (fmt: a "%s" and a "%f"), each since the previous mark, after draining `sync` if set
struct StageClock {
  bool on;
  const char* fmt;
  hipStream_t sync = nullptr;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void mark(const char* what) {
    if (!on) return;
    if (sync) (void)hipStreamSynchronize(sync);
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, fmt, what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

struct EventPair { Event a, b; int kind; };

// A batch's statistics read-back: one array of num_wg words per statistic (BatchState::acc_closest and the four after it, one
// allocation), behind the split path's two arrays of per-workgroup ray counts (one per round parity) in BatchSlot::h_counts.
enum StatWord : uint32_t { kStatClosest, kStatShadow, kStatHits, kStatUnoccluded, kStatDirect, kStatWords };
constexpr uint32_t kSplitCounts = 2;

// BatchState's arrays (kernels/hj_device.h), each with its number of elements per sample, per path-state position (both round
// parities where it has two) or per workgroup: f(pointer, Per, elements).  ensure_path_state allocates them, run_begin sums them.
// extinction: the scene has tinted dielectrics, or the caller writes ext[] whatever the scene (hj_debug_shade_step).
enum class Per { Sample, Position, Workgroup };
inline uint32_t hit_bins(bool env) { return hj::kNumTags + (env ? 1u : 0u); }   // (an environment: the miss bin, kernels/hj_stages.h kMissBin)
template <class F>
void batch_arrays(hj::BatchState& st, bool extinction, bool env, F&& f) {
  f(st.smp_rgb, Per::Sample, 1);
  f(st.smp_nd, Per::Sample, 1);
  for (int par = 0; par < 2; par++) {
    f(st.ray_o[par], Per::Position, 1);
    f(st.ray_d[par], Per::Position, 1);
    f(st.thr[par], Per::Position, 1);
    if (extinction) f(st.ext[par], Per::Position, 1);   // (only tinted dielectrics read it)
    else st.ext[par] = nullptr;
  }
  f(st.hit, Per::Position, 1);
  f(st.hit_tag, Per::Position, 1);
  f(st.q_hit, Per::Position, hit_bins(env));
  f(st.sh_o, Per::Position, 1);
  f(st.sh_d, Per::Position, 1);
  f(st.sh_c, Per::Position, 1);
  f(st.cnt_ray[0], Per::Workgroup, 1);
  f(st.cnt_ray[1], Per::Workgroup, 1);
  f(st.cnt_hit, Per::Workgroup, hit_bins(env));
  f(st.cnt_shadow, Per::Workgroup, 1);
  f(st.acc_closest, Per::Workgroup, kStatWords);   // acc_closest .. acc_direct (StatWord): one read-back
}

// A batch's path state and its owner: what a batch slot, the path query (hj_context::PathQuery) and hj_debug_shade_step's
// fabricated batch hand to the kernels, sized by ensure_path_state and freed with the object.
struct PathState {
  hj::BatchState st{};
  DevBufs state, samples;               // path-state arrays + queues + per-workgroup arrays; per-sample buffers (batch_arrays)
  size_t alloc_positions = 0;           // record positions the path-state arrays hold (workgroups x pool)
  uint32_t alloc_wgs = 0;               // workgroups the per-workgroup arrays hold
  bool env_bins = false;                // ... and the queues hold the miss bin of an environment (hit_bins)
};

// Launches of `G` workgroups: num_wg, and acc_shadow .. acc_direct at stride G behind acc_closest (as the read-back expects them).
inline void set_num_wg(hj::BatchState& st, uint32_t G) {
  st.num_wg = G;
  st.acc_shadow = st.acc_closest + (size_t)kStatShadow * G;
  st.acc_hits = st.acc_closest + (size_t)kStatHits * G;
  st.acc_unoccluded = st.acc_closest + (size_t)kStatUnoccluded * G;
  st.acc_direct = st.acc_closest + (size_t)kStatDirect * G;
}

// ... and that read-back (kStatWords arrays of G words), folded into a call's statistics
inline void add_stat_words(hj_render_stats& stats, const uint32_t* h_acc, size_t G) {
  for (size_t i = 0; i < G; i++) {
    stats.closest_rays += h_acc[kStatClosest * G + i];
    stats.shadow_rays += h_acc[kStatShadow * G + i];
    stats.hits += h_acc[kStatHits * G + i];
    stats.unoccluded_shadow_rays += h_acc[kStatUnoccluded * G + i];
    stats.shadow_rays_proven_free += h_acc[kStatDirect * G + i];
  }
}

}  // namespace hjapi

using hjapi::DevBuf;
using hjapi::DevBufs;
using hjapi::EventPair;
using hjapi::Event;
using hjapi::PinnedBuf;
using hjapi::Stream;

constexpr uint32_t kMaxSlots = 4;

struct hj_context {
  int device = 0;
  Stream stream;
  std::string error;
  int num_cus = 256;

  // scene
  bool have_scene = false;
  hj::DeviceScene scene{};
  DevBufs scene_bufs;
  uint32_t num_textures = 0;             // of the scene (scene.textures holds them: kernels/hj_texture.h)
  // hj_scene_update_shapes (api/scene_update.hip).  What the upload keeps for it: per node i of the uploaded array where its record
  // went in the re-laid-out copy (x) and where its guard record is (y), kNoRecord for none - a collapsed node, a pair's leaf, a leaf
  // without a guard (record root2 + i of the second copy needs no map).  What the first update adds: its own link set (the uploaded
  // topology's links, parents and counters - hj_context::refit_links is another caller's), the scratch records of the bottom-up pass,
  // staging for shape arrays that come from the host.  Every pointer is a buffer of scene_bufs: release_scene forgets them.
  struct SceneUpdate {
    static constexpr uint32_t kNoRecord = 0xFFFFFFFFu;
    const uint2* node_map = nullptr;     // [nodes0]
    size_t nodes0 = 0;                   // records of the uploaded array
    size_t num_vertices = 0, num_pairs = 0;
    bool ready = false;                  // the fields below are allocated and the links verified
    uint2* links = nullptr;              // [nodes0] (shape_index, exit_index)
    uint32_t* parent = nullptr;          // [nodes0]
    uint32_t* arrived = nullptr;         // [nodes0] zero between passes
    float4* scratch = nullptr;           // [2 * nodes0] the refitted skip-link records
    double* partial = nullptr;           // the cost's partial sums, one per 256 records
    uint32_t* verdict = nullptr;         // [4] the check kernel's word
    float4* in_spheres = nullptr;        // staging of host arrays
    float4* in_quads = nullptr;
    hj_vertex* in_vertices = nullptr;
    hj_emitter* in_emitters = nullptr;
  } update;

  // framebuffer
  float4* accum = nullptr;
  bool accum_owned = false;
  uint32_t width = 0, height = 0;

  // Batch slots: batch k runs on slot k mod num_slots (own state arrays, own stream), so the latency-bound tail of
  // one batch (a few long paths) overlaps the throughput phase of the next ones.
  struct BatchSlot : hjapi::PathState {
    DevBuf d_blocks, d_tiles;
    PinnedBuf<uint32_t> h_tiles;          // pinned staging of the per-tile block lists
    Stream stream;
    Stream rstream;                       // the reconstruction's stream (high priority: see hj_context_create)
    Event ev_path;                        // this slot's path kernel has finished (the reconstruction stream waits for it)
    PinnedBuf<hj_image_block> h_blocks;   // pinned staging of the block list
    PinnedBuf<uint32_t> h_counts;         // pinned read-back: kSplitCounts + kStatWords arrays of num_wg words
    Event ev_count[2];
    Event ev_recon;                       // this slot's reconstruction has run (orders framebuffer updates)
    Event ev_done;                        // batch complete, statistics copied back
    bool pending = false, recon_recorded = false;
    uint32_t nb_in_flight = 0;            // ImageBlocks of the batch in flight (progress reporting)
    uint32_t g_in_flight = 0;             // workgroups of the batch in flight (statistics read-back)
  } slots[kMaxSlots];
  uint32_t num_slots = 3;
  uint32_t slots_eff = 3;                // ... the current render call rotates through (1 when device memory is very short)
  uint32_t num_wg = 2048;                // grid size of the path kernels of a large render call (= queue segments), and the most a call uses
  uint32_t num_wg_small = 1536;          // ... of a small one (run_begin)
  uint32_t num_wg_eff = 2048;            // ... of the current call
  uint32_t pool = 32768;                 // path slots per workgroup of the fused kernel (HJ_POOL)
  uint32_t pool_eff = 32768;             // ... as the current render call uses it (lowered when device memory is short)

  // timing
  std::vector<EventPair> events;
  size_t events_used = 0;

  // progress (hj_set_progress_callback): called from the thread that drives the render, when a batch has completed
  hj_progress_fn progress = nullptr;
  void* progress_user = nullptr;
  uint32_t progress_interval = 128;
  uint64_t blocks_total = 0, blocks_done = 0, blocks_reported = 0;

  // hj_render_frame_async: ONE persistent worker thread per context (started by the first asynchronous frame) runs the
  // blocking render; hj_sync waits for it.  `busy` is what every other entry point checks (HJ_ERR_STATE while a frame is
  // in flight); the last frame's result stays retrievable (hj_sync) until the next asynchronous frame starts.
  std::thread worker;
  std::mutex job_mu;
  std::condition_variable job_cv;
  struct AsyncJob { uint32_t spp, pass_begin, pass_end, rank, world; uint64_t master_seed; hj_render_opts opts; } job{};
  bool job_posted = false, worker_exit = false;
  std::atomic<bool> busy{false};
  bool async_valid = false;               // async_rc / async_stats hold a finished frame's result
  int async_rc = HJ_OK;
  hj_render_stats async_stats{};

  // Frames back to back WITHOUT draining the batch pipeline between them (HJ_RENDER_NO_DRAIN, hj_pipeline_wait): one event per
  // frame submitted (recorded behind its last batch), the statistics accumulated since the last full drain, the slot rotation
  // carried from frame to frame.
  std::vector<Event> frame_events;        // oldest first: frames submitted, not yet waited for
  std::vector<Event> frame_event_pool;
  bool pipe_active = false;               // something submitted with HJ_RENDER_NO_DRAIN has not been drained yet
  hj_render_stats pipe_stats{};
  size_t pipe_k = 0;
  std::chrono::steady_clock::time_point pipe_wall0;

  // The tree hj_build_bvh_device built last, still on the device together with the shape arrays it was built over: hj_scene_upload
  // with scene->bvh == NULL takes it over (no trip through the host), hj_bvh_device_read copies it out.  Released by the next
  // build, by the upload that consumes it, and with the context.
  struct ResidentTree {
    hjapi::DevBuf nodes, spheres, quads, triangles, vertices;
    size_t total = 0, ns = 0, nq = 0, nt = 0, nv = 0;
    uint64_t shapes_hash = 0;                    // hjapi::shape_arrays_hash of the arrays the tree was built over
    bool valid = false;
    void release() { nodes.release(); spheres.release(); quads.release(); triangles.release(); vertices.release(); total = 0; valid = false; }
  } resident;

  // hj_refit_bvh_device: the topology of the last refit that brought one - (shape_index, exit_index) per record, 8 bytes each -,
  // kept for the refits that follow (scene->bvh == NULL).  Replaced by the next refit that brings a topology, freed with the context;
  // builds and uploads neither read nor drop it.
  struct KeptLinks {
    hjapi::DevBuf links;
    hjapi::DevBuf parent, arrived;               // derived from the links once: parent of every record, the climb's counters (all zero
                                                 // between refits), 4 bytes per record each
    size_t shapes = 0;                           // the links are 2 * shapes - 1 records
    bool valid = false;
  } refit_links;

  // hj_trace_rays (api/ray_query.hip): device staging of host arrays - one chunk of rays, their hit records and surface records.
  // Grown on demand (dev_alloc keeps a buffer that is large enough), reused by every call, freed with the context.
  struct RayQuery { hjapi::DevBuf rays, hits, surface; } query;

  // hj_trace_paths (api/path_query.hip): its own path state - num_wg x pool positions, per-workgroup arrays for HJ_PATHS_WGS
  // workgroups, one chunk of samples (ensure_path_state: a set that is too short is freed and allocated again, whole) - and the
  // device staging of host arrays (grown on demand).  Never the batch slots': a query between two frames leaves them and the
  // framebuffer alone.  Reused by every call, freed with the context.
  // hj_trace_paths_adaptive (api/path_adaptive.hip) runs its rounds in the same path state and adds, per ray of a call: the running
  // sums, the active flags, two index lists and one compacted ray array (ping-pong of the compaction), and the moments' staging.
  // hj_trace_irradiance (api/gather_query.hip) runs in the same path state and stages host arrays in in_rays (a chunk of points) and
  // out_samples (their records: 32 bytes a point, 144 with HJ_GATHER_SH9).
  // hj_trace_irradiance_adaptive (api/gather_adaptive.hip) is the adaptive query over points: the same buffers, and 8 bytes a point more.
  struct PathQuery : hjapi::PathState {
    hjapi::DevBuf in_rays, out_samples;   // staging: one chunk of rays (adaptive: all rays of the call), their sample records
    hjapi::DevBuf pa_sums, pa_s2;         // adaptive: float4 (R, G, B, S1) and float S2 per ray
    hjapi::DevBuf pa_flags;               // ... uint32 per entry of a round's list: the ray is still active
    hjapi::DevBuf pa_src[2];              // ... uint32 per entry: the list's ray indices, this round's and the next's
    hjapi::DevBuf pa_rays;                // ... the next round's rays: the active rays in order, seeds advanced
    hjapi::DevBuf pa_counts;              // ... per workgroup of the compaction its active count / offset, then the total
    hjapi::DevBuf pa_moments;             // ... staging of host moments
    hjapi::DevBuf pa_state;               // ... the query's own running state per record (the adaptive gather: hit count, nearest hit)
    hjapi::PinnedBuf<uint32_t> pa_active; // ... the total as the host reads it after a round
  } paths;

  // hj_lightmap_texels / hj_bake_lightmap (api/lightmap.hip): the owner map (a word per texel), per 64 triangles the mask of those
  // whose texel box is left to whole waves, the scan's tile counts and their
  // total, staging of host-side points; the bake's points, gather records and its two ping-pong images.  Grown on demand
  // (dev_alloc keeps a buffer that is large enough), reused by every call, freed with the context.
  // hj_filter_lightmap (api/lightmap_filter.hip): guide, 32 bytes per texel (position, valid word, normal); it shares points (staging
  // of host arrays) and the two images
  // hj_bake_lightmap_adaptive: sample_map, the staging of a host-side sample map (a word per texel)
  struct Lightmap { hjapi::DevBuf owner, masks, counts, points, records, image[2], guide, sample_map; } lightmap;

  // hj_probe_points / hj_bake_probes / hj_sample_probes (api/probe_volume.hip): the bake's gather points (32 bytes a probe) and the
  // gather's SH records (144 bytes a probe); staging of a host-side volume (112 bytes a probe), of host-side sample points (32 bytes
  // a point) and of their results (16 bytes a point).  Grown on demand, reused by every call, freed with the context.
  // hj_update_probes (api/probe_update.hip) uses points, records and - for host arrays - volume, each for the probes of its window alone.
  struct Probes { hjapi::DevBuf points, records, volume, in_points, out; } probes;

  // hj_probe_visibility_rays / hj_bake_probe_visibility / hj_sample_probes_visible (api/probe_visibility.hip): one slab's rays (32
  // bytes a ray) and hits (16 bytes a ray), at most HJ_PROBE_VIS_SLAB_RAYS of them; staging of a host-side atlas (the bake: one
  // slab's part, the look-up: whole), volume, sample points and results.  Grown on demand, reused by every call, freed with the context.
  // hj_update_probe_visibility (api/probe_update.hip) uses rays, hits and - for host arrays - atlas, each for one slab of its window.
  struct ProbeVis { hjapi::DevBuf rays, hits, atlas, volume, in_points, out; } probe_vis;

  // hj_place_probes and the placed calls (api/probe_place.hip): one slab's surface records (64 bytes a ray) beside probe_vis' rays
  // and hits; the staging of a host-side placement (16 bytes a probe: a slab's, a window's, the look-up's whole); the tile counts and
  // the list of a window's active probes (4 bytes a probe).  The placed updates use probes' and probe_vis' buffers as the updates do,
  // a host-side atlas staged for the whole window.  Grown on demand, reused by every call, freed with the context.
  struct ProbePlace { hjapi::DevBuf surface, placement, counts, list; } probe_place;

  // hj_closest_points / hj_distance_field (api/closest_query.hip): device staging of host arrays - one chunk of points (16 bytes a
  // point) and their records (32 bytes a point) -, the statistics' partial sums (16 bytes a workgroup); the field's gather points (32
  // bytes a point of a chunk) and the staging of a host-side field (4 bytes a point).  The sibling of RayQuery: grown on demand,
  // reused by every call, freed with the context.
  struct ClosestQuery { hjapi::DevBuf points, out, partial, grid, field; } closest;

  // hj_trace_rays_all / hj_points_inside (api/multi_hit.hip): device staging of host arrays - one chunk of rays (32 bytes a ray; of
  // points: 16 bytes a point), their count pairs (8 bytes a ray or point) and their hit lists (16 * max_hits bytes a ray).  The
  // sibling of RayQuery: grown on demand, reused by every call, freed with the context.
  struct AllHits { hjapi::DevBuf rays, counts, hits; } allhits;

  // hj_eval_materials / hj_render_aovs (api/aov.hip): the call's block list (40 bytes a block), the hit records of one walk launch
  // (16 bytes a sample slot, 16384 slots a block), the staging of a host-side AOV image (48 bytes a pixel); hj_eval_materials' staging
  // of host arrays - one chunk of hit records, surface records and material records (16, 64 and 32 bytes a record).  The sibling of
  // RayQuery: grown on demand, reused by every call, freed with the context.  Never the batch slots' or the framebuffer.
  // hj_render_aovs_followed (api/follow.hip) adds the rounds' buffers over the sample slots of one walk launch (chain: 36 bytes a slot
  // and a count per tile); hj_follow_specular the staging of host-side rays in and out (32 bytes a record each).
  struct Aov { hjapi::DevBuf blocks, hits, image, in_hits, in_surface, out, in_rays, out_rays; hjapi::ChainBufs chain; } aov;

  // hj_render_probe_lit (api/probe_lit.hip): per sample slot of one walk launch 64 bytes - the look-up point (32), the look-up's
  // record (16), the side record (16) -; the staging of a host-side volume, atlas and placement, once a call.  The block list, the hit
  // records, the chain state and a host-side image's staging (16 bytes a pixel) are Aov's.  Grown on demand, freed with the context.
  struct ProbeLit { hjapi::DevBuf points, lookup, side, volume, atlas, placement; } probe_lit;

  // hj_render_direct_lit (api/direct_lit.hip): per sample slot of one walk launch 48 bytes - the shadow ray (32) and the pending direct
  // term (16).  The list of the slots that want a ray and its tile counts are Aov's chain buffers (the rounds of a launch are over
  // before its shadow rays are listed); everything else is ProbeLit's and Aov's.  Grown on demand, freed with the context.
  struct DirectLit { hjapi::DevBuf rays; } direct_lit;

  // hj_denoise_frame (api/denoise.hip): the guide (48 bytes a pixel: normal and depth, albedo and valid word, depth slope) and the
  // two working images (16 bytes a pixel each); the staging of host arrays - beauty, AOV image, result (16, 48 and 16 bytes a
  // pixel).  Grown on demand, reused by every call, freed with the context.  The framebuffer is read, never written.
  // hj_denoise_frame_temporal (api/denoise_temporal.hip) adds the staging of the two histories (48 bytes a pixel each).
  // hj_denoise_frame_temporal_motion adds the staging of a host-side motion image (16 bytes a pixel).
  struct Denoise { hjapi::DevBuf guide, image[2], in_beauty, in_aov, out, in_history, out_history, in_motion; } denoise;

  // hj_render_motion (api/motion.hip): the staging of host-side previous shape arrays (16 / 48 / 32 bytes a sphere / quad / vertex)
  // and of a host-side motion image (16 bytes a pixel).  Grown on demand, reused by every call, freed with the context.
  // hj_render_motion_followed (api/motion_follow.hip) adds the rounds' buffers over the pixels of the image (chain: 36 bytes a pixel
  // and a count per tile) and, per pixel, the product of the chain's reflections (48 bytes).
  struct Motion { hjapi::DevBuf spheres, quads, vertices, image, mat; hjapi::ChainBufs chain; } motion;

  // the library's environment switches (api/hj_tuning.h) as the entry point in progress read them: hj_context_create, then every
  // hj_scene_upload / render call / BVH build refreshes the copy at its start; nothing below an entry point reads the environment
  hjapi::Tuning tuning;

  // hj_last_error: the worker thread writes `error` while the caller's thread may read it
  std::mutex err_mu;
};

namespace hjapi {

int set_error(hj_context* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
std::string get_error(hj_context* ctx);
// A fingerprint of a scene's shape arrays (counts + 4096 evenly spaced 16-byte pieces of each): guards the hand-over of a tree that
// stayed on the device against an upload of OTHER geometry with the same counts (an accident, not an adversary).
uint64_t shape_arrays_hash(const hj_scene_desc* s);
void put_error(hj_context* ctx, const std::string& text);
std::mutex& alloc_mutex();                           // process-wide: a context sizing its batch slots (api/render_calls.hip run_submit)
// api/scene_upload.hip: every invariant an upload checks; HJ_MAT_DIFFUSE_TEXTURED indices must be < num_textures
int validate_scene(hj_context* ctx, const hj_scene_desc* s, size_t num_textures);
// ... and its check of the links alone: bvh[N] is a pre-order skip-link tree (shape words are not read but for HJ_BVH_INNER)
int validate_tree_links(hj_context* ctx, const hj_bvh_node* bvh, size_t N);
// api/environment.hip: an environment's checks (hj_scene_upload_env) and its sampling distribution, built on the host before anything
// is allocated; upload_environment copies the table and fills DeviceScene's env_* fields (env == NULL: nothing)
struct EnvTable { std::vector<float4> rec; std::vector<double> prob, omega; double weight_sum = 0.0; };
int validate_environment(hj_context* ctx, const hj_scene_desc* s, const hj_texture_set* t, const hj_environment* env, EnvTable& out);
int upload_environment(DevBufs& bufs, const hj_texture_set* t, const hj_environment* env, const EnvTable& table, hj::DeviceScene& d);
int validate_textures(hj_context* ctx, const hj_texture_set* t);             // api/texture.hip
int upload_textures(DevBufs& bufs, const hj_texture_set* t, const float4** out);
void release_scene(hj_context* ctx);
// api/scene_upload.hip: the light-shaft grid of `s` (all arrays on the host, or the tree at d_tree) into a new buffer of `bufs` and
// d's lg_* fields; no grid (by size, by HJ_LIGHT_GRID, or because none could be proven) leaves d alone and returns HJ_OK
int upload_light_grid(DevBufs& bufs, const hj_scene_desc* s, const Tuning& tn, const hj_bvh_node* d_tree, hj::DeviceScene& d);
// Room for `samples` samples and G x pool positions (per-workgroup arrays for Gmax >= G workgroups) in ps, and ps.st's pointers,
// pool and num_wg set for a launch of G workgroups.  A set that is too short - or lacks ext[] / the miss bin the scene now
// needs - is freed first, then allocated whole; on failure the caller releases ps (or lets it go).  (api/context.hip)
int ensure_path_state(hj_context* ctx, PathState& ps, size_t samples, uint32_t G, uint32_t Gmax, uint32_t pool, bool extinction, bool env);
void release_path_state(PathState& ps);
void release_batch(hj_context* ctx);
// api/path_query.hip: the shape of a fixed-spp pass over at most n rays as hj_trace_paths lays it out - rays and samples of the
// largest launch, its workgroups and positions per workgroup - and one launch of the path kernel over cnt device rays into st's
// sample arrays (smp_rgb / smp_nd of sample ray * spp + k; the statistics per workgroup behind st.acc_closest, st.num_wg of them)
struct PathQueryPlan { size_t chunk_rays, most_rays, most_samples; uint32_t G, pool; };
PathQueryPlan path_query_plan(const Tuning& tn, size_t n, uint32_t spp);
void path_query_pass(hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_rays, uint32_t cnt, uint32_t spp,
                     const hj_render_opts& o, hipStream_t s);
// api/path_query.hip: what the query entry points share; `fn` is the entry point's name, for the messages.
//   query_render_opts  opts (NULL: the defaults) into o and the refusals of the path-type queries: max_bounces, use_bvh, HJ_RENDER_* bits
//   query_gate         every query, behind its argument checks: a null context (HJ_ERR_DEVICE without a HIP device, HJ_ERR_INVALID
//                      otherwise), an asynchronous frame in flight, frames in the pipeline, no scene
//   context_gate       query_gate without its last check, for the calls that need a context but no scene
int query_render_opts(hj_context* ctx, const char* fn, const hj_render_opts* opts, hj_render_opts& o);
int query_gate(hj_context* ctx, const char* fn);
int context_gate(hj_context* ctx, const char* fn);
}  // namespace hjapi
namespace hj { struct PvGrid; struct PvvMap; }   // kernels/hj_probes.h, kernels/hj_probe_vis.h
namespace hjapi {
// api/probe_volume.hip: what every probe entry point refuses of a desc, without a device, in the header's order -> g, n = the probes;
// and the enqueue, on the context's stream, of the gather points of the probes first ... first + n - 1 (n > 0) under `seed`.
// probe_desc_check alone knows the mask of a desc's flags; probe_gather_flags: what the calls that gather (hj_bake_probes,
// hj_update_probes, hj_update_probes_placed) hand hj_trace_irradiance - sphere, SH9, device arrays, and HJ_GATHER_INDIRECT for a
// desc with HJ_PROBES_INDIRECT_ONLY
uint32_t probe_gather_flags(const hj_probe_desc* d);
int probe_desc_check(hj_context* ctx, const char* fn, const hj_probe_desc* d, hj::PvGrid& g, uint32_t& n);
void probe_points_enqueue(hj_context* ctx, const hj::PvGrid& g, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t n, float4* d_points);
// api/probe_visibility.hip: what hj_bake_probe_visibility refuses of the two descs, in the header's order -> g, n, v; and the enqueue
// of the bake's rays for the probes first ... first + probes - 1 (at most a slab's) under `seed`
int probe_vis_bake_check(hj_context* ctx, const char* fn, const hj_probe_desc* d, const hj_probe_vis_desc* vis, hj::PvGrid& g, uint32_t& n, hj::PvvMap& v);
// ... and the host side of hj_sample_probes_visible, which api/probe_place.hip's placed look-up enters with its placement and a launch
// of its own kernel (placed == nullptr: no placement); probe_place_check_offsets: a host-side placement's offsets must be finite
using ProbeVisSampleLaunch = void (*)(hipStream_t s, uint32_t blocks, const hj::PvGrid& g, const hj::PvvMap& v, const float4* d_probes, const float2* d_atlas,
                                      const float4* d_place, const float4* d_points, uint32_t m, float4* d_out);
int probe_vis_sample(hj_context* ctx, const char* fn, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes, const float* atlas,
                     const float* points, size_t m, float* out, const float* placement, ProbeVisSampleLaunch placed);
int probe_place_check_offsets(hj_context* ctx, const char* fn, const float* placement, uint32_t first, uint32_t num);
// api/probe_update.hip: what the updates refuse of an hj_probe_update behind the descs' refusals, in the header's order (n: the volume's probes)
int probe_update_check(hj_context* ctx, const char* fn, const hj_probe_update* u, uint32_t n);
void probe_vis_rays_enqueue(hj_context* ctx, const hj::PvGrid& g, const hj::PvvMap& v, uint32_t seed, uint32_t seed_stride, uint32_t first, uint32_t probes,
                            float4* d_rays);
// The light-map filter for both of its entry points (api/lightmap_filter.hip):
//   lightmap_filter_check    what both refuse of a filter, without a device: unknown flag bits, iterations, sigmas
//   lightmap_filter_enqueue  guide from the `count` device points, then f.iterations iterations from img[cur] into img[cur ^ 1], cur
//                            flipped by each: the result is in img[cur] on return.  Enqueues on the context's stream only.
//   lightmap_atlas_check     the atlas every light-map entry point accepts (the limits are here alone)
constexpr uint32_t kLightmapMaxSide = 16384u;
constexpr uint64_t kLightmapMaxTexels = 1ull << 26;
inline int lightmap_atlas_check(hj_context* ctx, const char* fn, uint32_t w, uint32_t h) {
  if (w == 0 || h == 0 || w > kLightmapMaxSide || h > kLightmapMaxSide || (uint64_t)w * h > kLightmapMaxTexels)
    return set_error(ctx, HJ_ERR_INVALID, "%s: atlas %u x %u: 1 ... 16384 each and at most 2^26 texels", fn, w, h);
  return HJ_OK;
}
int lightmap_filter_check(hj_context* ctx, const char* fn, const hj_lightmap_filter* f);
int lightmap_filter_enqueue(hj_context* ctx, const hj_lightmap_filter& f, uint32_t W, uint32_t H, const float4* d_points, uint32_t count, float4* const img[2],
                            uint32_t& cur);
// The frame denoiser for both of its entry points (api/denoise.hip):
//   denoise_check            what both refuse of (opts, width, height) behind their null checks, without a device
//   denoise_begin            the gate (no scene is needed), beauty == NULL against the framebuffer, the context's buffers, the staging
//                            of host arrays: on HJ_OK f holds the call's device arrays and f.e the first error of the copies enqueued
//   denoise_prepare_enqueue  k_dn_prepare: the guide's first two records, (I, 0) or (c, 0) into f.work[1]
//   denoise_filter_enqueue   iterations [i0, i1) from f.work[cur], cur flipped by each; finish: the last of them stores the remodulated
//                            result into f.out, and with none to run (i0 == i1) f.work[cur] is remodulated alone
constexpr uint32_t kDenoiseMaxSide = 16384u;
struct DenoiseFrame {
  uint32_t W, H;
  const float4 *beauty, *aov;
  float4 *guide, *work[2], *out;
  hipError_t e;
};
int denoise_check(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, const hj_denoise_opts* opts);
int denoise_begin(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, const float* beauty, const float* aov, float* out, bool on_device,
                  DenoiseFrame& f);
void denoise_prepare_enqueue(hj_context* ctx, const DenoiseFrame& f);
void denoise_filter_enqueue(hj_context* ctx, const hj_denoise_opts& o, const DenoiseFrame& f, uint32_t& cur, uint32_t i0, uint32_t i1, bool finish);
// A camera both temporal calls and hj_render_motion accept: finite position and rotation, a fov inside (0, 180)
inline bool camera_ok(const hj_camera& c) {
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(c.position[k])) return false;
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(c.rotation[k])) return false;
  return std::isfinite(c.fov) && c.fov > 0.0f && c.fov < 180.0f;
}
// api/follow.hip, for api/aov.hip's aov_render with max_follow > 0: room for walk launches of at most `slots` sample slots; the follow
// rounds behind a walk launch of nb blocks (-> followed: a round ran and the launch's runs resolve through aov_follow_resolve); and
// that resolve's launch for blocks [b0, b0 + cnt) of the launch
// api/follow.hip, which alone holds kernels/hj_chain.h's count and scan kernels, for api/chain_rounds.h's loop in any unit: over n slots
// k_chain_count<first> (the live chains per tile of 256 into d_counts) and k_chain_scan (their offsets in place, the total at
// d_counts[tiles]) on the context's stream
void chain_count_enqueue(hj_context* ctx, bool first, const float4* d_hits, const float4* d_state, uint32_t n, uint32_t max_follow, uint32_t* d_counts);
int aov_follow_reserve(hj_context* ctx, size_t slots);
hipError_t aov_follow_rounds(hj_context* ctx, const hj_image_block* d_blocks, uint32_t nb, float4* d_hits, uint32_t max_follow, bool& followed);
void aov_follow_resolve(hj_context* ctx, const hj_image_block* d_blocks, uint32_t nb, uint32_t b0, uint32_t cnt, const float4* d_hits, uint32_t width,
                        uint32_t height, float4* d_aov);
// api/aov.hip, for api/probe_lit.hip: the AOV calls' refusals (aov_check), the frame forms' block list (aov_frame_blocks) and their
// host routine (aov_render) with a stage that takes the resolves' place.  stage == nullptr: the AOV calls themselves.
//   words    floats a pixel of the stage's image (the AOV image: HJ_AOV_WORDS)
//   reserve  room for walk launches of at most `slots` sample slots, before anything of the call is enqueued
//   points   behind the camera walk and the follow rounds of a walk launch of nb blocks (followed: a round ran, the chain state is set)
//   resolve  in k_aov_resolve's / aov_follow_resolve's place, for blocks [b0, b0 + cnt) of that launch: a run's part
struct AovStage {
  uint32_t words;
  int (*reserve)(hj_context* ctx, const AovStage& st, size_t slots);
  hipError_t (*points)(hj_context* ctx, const AovStage& st, const hj_image_block* d_blocks, uint32_t nb, const float4* d_hits, bool followed);
  void (*resolve)(hj_context* ctx, const AovStage& st, const hj_image_block* d_blocks, uint32_t nb, uint32_t b0, uint32_t cnt, const float4* d_hits,
                  bool followed, uint32_t width, uint32_t height, float4* d_image);
  void* self;
};
int aov_check(hj_context* ctx, const char* fn, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t flags,
              const float* aov);
int aov_frame_blocks(hj_context* ctx, const char* fn, uint32_t width, uint32_t height, uint64_t master_seed, uint32_t pass_begin, uint32_t pass_end,
                     std::vector<hj_image_block>& blocks);
int aov_render(hj_context* ctx, const char* fn, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t flags,
               float* aov, uint32_t max_follow, const AovStage* stage);
// The look-ups' launches for api/probe_lit.hip, each by the unit that holds the kernel, over m (> 0) device points on the context's
// stream: api/probe_volume.hip's k_pv_sample; api/probe_visibility.hip's k_pvv_sample, or with `placed` (api/probe_place.hip's
// probe_place_sample_launch) and d_place k_pp_sample.  The launch shape is the public calls' own: they enter here too.
void probe_sample_enqueue(hj_context* ctx, const hj::PvGrid& g, const float4* d_probes, const float4* d_points, uint32_t m, float4* d_out);
void probe_vis_sample_enqueue(hj_context* ctx, const hj::PvGrid& g, const hj::PvvMap& v, const float4* d_probes, const float2* d_atlas, const float4* d_place,
                              const float4* d_points, uint32_t m, float4* d_out, ProbeVisSampleLaunch placed);
void probe_place_sample_launch(hipStream_t s, uint32_t blocks, const hj::PvGrid& g, const hj::PvvMap& v, const float4* d_probes, const float2* d_atlas,
                               const float4* d_place, const float4* d_points, uint32_t m, float4* d_out);
// api/probe_visibility.hip: what hj_sample_probes_visible (placed: hj_sample_probes_visible_placed) refuses of a volume - the descs, the
// probes, the atlas, the placement - in that call's order, the points and `out` aside -> g, n, v, reads_atlas.  any: the call has points
// (the look-ups accept null arrays without).
int probe_vis_volume_check(hj_context* ctx, const char* fn, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes, const float* atlas,
                           const float* placement, bool placed, bool any, hj::PvGrid& g, uint32_t& n, hj::PvvMap& v, bool& reads_atlas);
}  // namespace hjapi
namespace hj { struct DtArgs; }                  // kernels/hj_denoise_temporal.h
namespace hjapi {
// api/motion.hip: k_dt_accumulate<true> over a's image on the context's stream (hj_denoise_frame_temporal_motion; the temporal unit
// itself holds the <false> instantiation alone)
void dt_accumulate_motion_enqueue(hj_context* ctx, const hj::DtArgs& a);
// api/motion.hip: the host routine of hj_render_motion (max_follow == 0) and hj_render_motion_followed, behind the name fn
int motion_render(hj_context* ctx, const char* fn, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t max_follow, uint32_t flags,
                  float* motion);
}  // namespace hjapi
namespace hj { struct MvPrev; }                  // kernels/hj_motion.h
namespace hjapi {
// api/motion_follow.hip, for motion_render with max_follow > 0: room for the rounds over an image of `pixels` pixels; the follow rounds
// behind k_mv_walk, whose raw hits are at d_motion (-> followed: a round ran, every pixel's chain state is set and the image resolves
// through motion_follow_resolve); and that resolve's launch
int motion_follow_reserve(hj_context* ctx, size_t pixels);
hipError_t motion_follow_rounds(hj_context* ctx, uint32_t width, uint32_t height, float4* d_motion, uint32_t max_follow, bool& followed);
void motion_follow_resolve(hj_context* ctx, const hj::MvPrev& prev, uint32_t width, uint32_t height, float4* d_motion);
// The statistics read-back of a pass's launches (kStatWords x G words each), summed on the host once the stream has drained.
// on == false (the caller wants no statistics): every member does nothing.
struct QueryStats {
  bool on;
  uint32_t G = 0;
  std::vector<uint32_t> h_acc;
  explicit QueryStats(bool on_) : on(on_) {}
  int reserve(hj_context* ctx, const char* fn, size_t launches, uint32_t G);   // HJ_ERR_NOMEM: behind a synchronise of ctx->stream
  hipError_t enqueue(size_t launch, const hj::BatchState& st, hipStream_t s);  // the copy of the launch st was just set up for
  // ... of a pass over `len` rays in launches of chunk_rays at spp samples each, added to `to`
  void add(hj_render_stats& to, size_t chunk_rays, size_t len, uint32_t spp) const;
};
// A fixed-spp query behind its entry point's checks (n > 0): hj_trace_paths and hj_trace_irradiance.  fixed_spp_query owns the plan,
// the path state (hj_context::paths) and the staging of host arrays, the chunk loop - H2D, `chunk`, D2H, statistics copy -, the ONE
// hipStreamSynchronize and the statistics; `chunk` enqueues the path launch and the resolve of cnt records at d_in into d_out.
struct FixedSppQuery {
  const char* name;                      // the entry point
  const float* in;                       // n records of two float4: rays or points
  size_t n;
  uint32_t spp;
  size_t rec;                            // float4 of an output record
  bool on_device;                        // in / out are device arrays, used in place
  float* out;
  hj_render_stats* stats;                // may be NULL
  hj_render_opts o;
  void (*chunk)(const FixedSppQuery& q, hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_in, uint32_t cnt, float4* d_out,
                hipStream_t s);
  uint32_t flags;                        // the entry point's own, for `chunk`
};
int fixed_spp_query(hj_context* ctx, const FixedSppQuery& q);
// api/gather_query.hip: the gather's counterpart of path_query_pass - one launch of k_gq_paths over cnt device points at spp samples
// each into st's sample arrays, without the resolve (flags: HJ_GATHER_SPHERE, HJ_GATHER_INDIRECT) - and the check of host points' normals in
// hemisphere mode (finite, not all zero), for both gather entry points
void gather_query_pass(hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_pts, uint32_t cnt, uint32_t spp, const hj_render_opts& o,
                       uint32_t flags, hipStream_t s);
int gather_normals_check(hj_context* ctx, const char* fn, const float* points, size_t n);
// An adaptive query behind its entry point's checks (n > 0): hj_trace_paths_adaptive and hj_trace_irradiance_adaptive
// (api/path_adaptive.hip).  adaptive_query owns the plans, the path state, the per-record buffers (hj_context::PathQuery pa_*), the
// round loop - per chunk `pass` and `accumulate`, then the compaction of the list (k_pa_count / k_pa_scan / k_pa_scatter) -, the ONE
// hipStreamSynchronize per round, the staging of host arrays and the statistics.  `pass` enqueues the path launch of cnt records at
// d_in with c samples each; `accumulate` enqueues the kernel that continues the running sums over that launch's samples, evaluates
// the stop rule, writes the active flags and a stopping record's output (AdaptiveLaunch says where everything is).
struct AdaptiveLaunch {
  const uint32_t* src;                   // the launch's entries of the round's list (NULL in round 0: record first + j)
  uint32_t first, cnt, c, n_before;      // its place in the list, its records, samples a record this round and before it
  uint32_t spp_max;                      // the stop rule's constants
  float rel_error, floor;
  float4* sums;                          // per record of the call: (R, G, B, S1)
  float* s2;                             // ... S2
  void* state;                           // ... state_bytes of the query's own running state (NULL: none)
  uint32_t* flags;                       // per entry of the launch: still active
  float4* out;                           // two float4 per record of the call
  float4* moments;                       // may be NULL
};
struct AdaptiveQuery {
  const char* name;                      // the entry point
  const char* what;                      // "rays" / "points", for a message
  const float* in;                       // n records of two float4, the seed in word 6
  size_t n;
  hj_adaptive_opts a;                    // checked (adaptive_opts_check)
  bool on_device;                        // in / out / moments are device arrays, used in place
  float* out;
  float* moments;                        // may be NULL
  hj_render_stats* stats;                // may be NULL
  hj_render_opts o;
  void (*pass)(const AdaptiveQuery& q, hj::BatchState& st, const hj::DeviceScene& sc, uint32_t G, const float4* d_in, uint32_t cnt, uint32_t c, hipStream_t s);
  void (*accumulate)(const AdaptiveQuery& q, const hj::BatchState& st, const AdaptiveLaunch& l, hipStream_t s);
  uint32_t flags;                        // the entry point's own, for the callbacks
  size_t state_bytes;                    // running state per record beside the sums (0: none)
};
int adaptive_opts_check(hj_context* ctx, const char* fn, const hj_adaptive_opts* aopts, hj_adaptive_opts& a);
int adaptive_query(hj_context* ctx, const AdaptiveQuery& q);
// api/gather_adaptive.hip: the adaptive bake's scatter - `n` gather records whose word 3 is (float)n_i, into the zeroed image at the
// texel word 7 of the point names, scaled by 3.14159274f / (float)n_i; sample_map (may be NULL) gets n_i at that texel
void lightmap_scatter_adaptive(const float4* d_points, const float4* d_records, uint32_t n, float4* d_image, uint32_t* d_sample_map, hipStream_t s);
int sync_all(hj_context* ctx);                       // drains the context's streams (api/context.hip)
// The closing tail of an entry point that enqueued on the context's stream (fn: its name): the stream is synchronised whatever was
// enqueued and whatever failed - nothing of the call stays in flight - and the first error is the call's.  rc: the status so far, or
// e: the first hipError_t of the enqueue chain, refused as "fn: text".  (api/context.hip)
int drain(hj_context* ctx, const char* fn, int rc);
int drain(hj_context* ctx, const char* fn, hipError_t e);
void drop_cached_comms(hj_context* ctx);             // api/comm.hip: the communicators hj_reduce_framebuffers made for ctx

// api/render.hip: the launches of kernels/hj_kernels.h, on `s` (a failed launch surfaces at the render call's hipGetLastError)
void launch_path_wavefront(const hj::BatchState& st, const hj::DeviceScene& sc, const hj_render_opts& o, size_t lds_bytes, hipStream_t s);
void launch_gen_camera(const hj::BatchState& st, const hj::DeviceScene& sc, hipStream_t s);
void launch_trace_closest(const hj::BatchState& st, const hj::DeviceScene& sc, bool bvh, uint32_t parity, hipStream_t s);
void launch_shade(const hj::BatchState& st, const hj::DeviceScene& sc, uint32_t parity, const hj_render_opts& o, hipStream_t s);
void launch_trace_shadow(const hj::BatchState& st, const hj::DeviceScene& sc, bool bvh, hipStream_t s);
// tiles: the per-tile block lists (CSR: tiles_x * tiles_y + 1 offsets, then the block indices)
void launch_reconstruct(const hj::BatchState& st, float stddev, const uint32_t* tiles, uint32_t tiles_x, uint32_t tiles_y,
                        float4* accum, uint32_t width, uint32_t height, hipStream_t s);
void launch_debug_trace(const hj::DeviceScene& sc, const float* rays, uint32_t n, bool bvh, bool any_hit, float4* hits, hipStream_t s);

// The blocks of passes [p0, p1) of a frame that `rank` of `world` renders, in the frame's order (pass by pass, raster order inside a
// pass), appended to `out`: ONE text for hj_render_frame (api/render_calls.hip) and hj_render_aovs_frame (api/aov.hip, world 1).
inline void frame_blocks_append(const hijiki::BlockGrid& grid, uint64_t master_seed, uint32_t p0, uint32_t p1, uint32_t rank, uint32_t world,
                                bool static_deal, std::vector<hj_image_block>& out) {
  const uint32_t per_pass = grid.per_pass();
  for (uint32_t p = p0; p < p1; p++)
    for (uint32_t j = 0; j < per_pass; j++)
      if (grid.owner(static_deal ? 0u : p, j, world) == rank) out.push_back(grid.make(master_seed, p, j));
}

// The scene as a render call's kernels see it: the light-shaft grid (api/light_grid.cpp) answers "no shape of the TREE lies
// between this cell and that emitter", so it is taken away from a linear-scan render (scene.glsl:134-158 tests every shape of
// the arrays, in the tree or not) and from a call that asks for every shadow ray to be walked (HJ_RENDER_NO_LIGHT_GRID).
inline hj::DeviceScene scene_for(const hj_context* ctx, const hj_render_opts& o) {
  hj::DeviceScene sc = ctx->scene;
  if (!o.use_bvh || (o.flags & HJ_RENDER_NO_LIGHT_GRID)) sc.light_grid = nullptr;
  return sc;
}

}  // namespace hjapi

// Entry points that touch the context's device state refuse to run while an asynchronous frame is in flight on it
// (the worker thread owns the slots, the streams and the framebuffer until hj_sync).
// (fn: the entry point's name where a helper checks on its behalf)
#define HJ_NOT_BUSY_IN(ctx, fn)                                                                                   \
  do {                                                                                                            \
    if ((ctx)->busy.load(std::memory_order_acquire))                                                              \
      return set_error(ctx, HJ_ERR_STATE, "%s: an asynchronous frame is in flight on this context: call hj_sync first", fn); \
  } while (0)
#define HJ_NOT_BUSY(ctx) HJ_NOT_BUSY_IN(ctx, __func__)

// ... and while frames submitted with HJ_RENDER_NO_DRAIN are still in flight (hj_pipeline_wait(ctx, 0, ...) drains them).
#define HJ_NOT_PIPELINED_IN(ctx, fn)                                                                              \
  do {                                                                                                            \
    if ((ctx)->pipe_active)                                                                                       \
      return set_error(ctx, HJ_ERR_STATE, "%s: frames submitted with HJ_RENDER_NO_DRAIN are in flight: call hj_pipeline_wait(ctx, 0, ...) first", fn); \
  } while (0)
#define HJ_NOT_PIPELINED(ctx) HJ_NOT_PIPELINED_IN(ctx, __func__)

#define HJ_HIP(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return set_error(ctx, e_ == hipErrorOutOfMemory ? HJ_ERR_NOMEM : HJ_ERR_DEVICE, "%s: %s", #call, \
                       hipGetErrorString(e_));                                                    \
  } while (0)

// a step that returns an HJ_* status: a failure ends the calling function with it
#define HJ_TRY(expr) do { const int rc_ = (expr); if (rc_ != HJ_OK) return rc_; } while (0)

namespace hjapi {

// `count` elements of T from the host into a new buffer of `bufs`
template <class T>
int upload(DevBufs& bufs, const T* src, size_t count, const T** out) {
  T* p = nullptr;
  // 64 bytes of slack: the walk's merged step reads two 16-byte parts of every shape record, a sphere has one
  int rc = bufs.alloc(p, count, 64);
  if (rc != HJ_OK) return rc;
  if (count) HJ_HIP(bufs.ctx, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return HJ_OK;
}

// Device arrays must be 16-byte aligned (the kernels read and write them as float4 / uint4): true when a pointer is not; null
// pointers - an optional array the caller left out - do not count.
template <class... P>
bool misaligned(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & 15u) != 0; }

// The grid of a kernel with one lane per element and workgroups of kBlockThreads (api/path_query.hip)
dim3 per_lane(uint32_t n);
// Rays (or sample slots) per workgroup of a persistent walk over n of them: k_rq_walk and k_aov_walk (api/ray_query.hip)
uint32_t walk_wg_rays(const hj_context* ctx, uint32_t n);

// A flat per-element query behind its entry point's argument checks and its gate (n > 0): hj_trace_rays, hj_trace_rays_all,
// hj_points_inside, hj_closest_points, hj_eval_materials.  One lane per element, in launches of HJ_TRACE_CHUNK elements, which bounds
// the staging buffers of host arrays; device arrays take the same loop and the same launches, element `at` of the caller's own
// pointer used in place, and nothing is allocated.  chunked_query owns hipSetDevice, the staging allocations - every one before
// anything is enqueued, in the table's order -, the loop, the copies up and down and the ONE hipStreamSynchronize (drain): a failed
// upload or launch ends the loop and the call still drains.  `launch` enqueues the kernels of one chunk on ctx->stream - d[i]: where
// array i's cnt elements are on the device, nullptr for an absent one; k: the launch's index - and returns hipGetLastError() or the
// first error of what it enqueued behind the kernels.
struct QueryArray {
  const void* user;                      // the caller's array; nullptr: absent - no buffer, no copy
  DevBuf* stage;                         // the context's staging buffer for it (host arrays)
  size_t bytes;                          // per element; 0: absent
  bool out;                              // copied down behind the launch; otherwise up in front of it
};
template <size_t N, class L>
int chunked_query(hj_context* ctx, const char* fn, size_t n, bool on_device, const QueryArray (&arrays)[N], L&& launch) {
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  const size_t chunk = (size_t)ctx->tuning.trace_chunk;
  char* user[N];
  void* d[N] = {};
  for (size_t i = 0; i < N; i++) {
    const QueryArray& a = arrays[i];
    user[i] = a.bytes ? static_cast<char*>(const_cast<void*>(a.user)) : nullptr;
    if (on_device || !user[i]) continue;
    HJ_TRY(dev_alloc(ctx, *a.stage, std::min(n, chunk) * a.bytes));
    d[i] = a.stage->p;
  }
  hipError_t e = hipSuccess;
  size_t k = 0;
  for (size_t at = 0; at < n && e == hipSuccess; at += chunk, k++) {
    const uint32_t cnt = (uint32_t)std::min(chunk, n - at);
    for (size_t i = 0; i < N && e == hipSuccess; i++) {
      if (!user[i]) continue;
      const QueryArray& a = arrays[i];
      if (on_device) d[i] = user[i] + at * a.bytes;
      else if (!a.out) e = hipMemcpyAsync(d[i], user[i] + at * a.bytes, cnt * a.bytes, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e != hipSuccess) break;
    e = launch(d, cnt, k);
    for (size_t i = 0; i < N && e == hipSuccess; i++) {
      const QueryArray& a = arrays[i];
      if (!on_device && user[i] && a.out) e = hipMemcpyAsync(user[i] + at * a.bytes, d[i], cnt * a.bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
  }
  return drain(ctx, fn, e);
}

}  // namespace hjapi
