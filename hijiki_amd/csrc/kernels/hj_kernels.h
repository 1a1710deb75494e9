// Wavefront path-tracing kernels for gfx950 (wave64).
//
// One batch = up to `capacity` camera paths (many ImageBlocks of many passes).  Every path workgroup owns one
// private segment of every queue (hj_device.h) and advances ITS paths one bounce per round:
//
//   per round (hj_stages.h):
//     stage_camera_packets render.glsl:26-36,149-162         NEW camera paths: 64-ray packets built from the sample index (kernels
//                                                            without the packet stage: stage_gen_camera writes explicit records)
//     stage_trace_merged   scene.glsl:92-133                 skip-link BVH walk (hj_walk.h) of the closest-hit rays (-> hit record)
//                                                            and of the previous round's shadow rays (any-hit, boolean-
//                                                            equivalent to the reference's closest-hit; adds NEE radiance)
//     compact_hits_by_tag                                    hits binned by MATERIAL TAG in queue order (wave ballots)
//     stage_shade          scene.glsl:160-175, render.glsl:102-144, material.glsl
//                                                            populate, emission, NEE sample, BSDF sample (hj_shade.h),
//                                                            roulette -> next ray queue + shadow queue
//   k_reconstruct (hj_reconstruct.h)  reconstruction.glsl:22-66
//
// Files: hj_device.h (scene / batch views) <- hj_intersect.h (shape tests, node step) <- hj_walk.h (persistent walk),
// hj_shade.h (populate, emitters) <- hj_stages.h (the stages + their call wrappers) <- this file (the kernels).
//
// k_path_wavefront runs all stages of a batch in ONE persistent launch (workgroup barriers only): the kernel's own code
// is the walk (trace_persistent: in-wave ray replacement, merged first step, bounded burst), the other stages are
// CALLED device functions (stage_*_call<.., ENV>, compact_hits_call<.., ENV>: register-allocated on their own, so the walk
// stays free of spills; inlined they made the walk spill - rounds 2-3, profiles/NOTES.md); `rp` = the round timing of the statistics build (hj_walk_probe.h);
// k_gen_camera / k_trace_closest / k_shade / k_trace_shadow launch the stages one by one (diagnostic path).
// No stage uses a global atomic: appends are wave ballot + one LDS atomic.
//
// Every path owns its RNG state, so queue order never changes results; the per-path order of radiance
// additions is the reference's (emission, then NEE, bounce by bounce) because a workgroup's stages are
// separated by barriers (fused) or kernel boundaries (split).
#pragma once
#include <type_traits>
#include "hj_stages.h"
#include "hj_reconstruct.h"

#pragma clang fp contract(off)

namespace hj {

// ------------------------------------------------------------------ kernels

// The whole life of a batch in ONE launch.  Every workgroup walks through ITS samples (64-sample groups g, g + G, ...):
// rounds of { top-up: new camera paths behind the continuing ones -> ONE walk phase for the closest-hit rays of the
// paths in flight and the shadow rays of the previous round -> hits compacted by material tag -> shade, which writes
// the continuing paths compacted into the other parity's arrays } on its private segments.  Workgroups never
// exchange data, so there is no grid barrier, no host round trip and no per-stage launch; while one workgroup shades
// (memory bound) its CU neighbours walk the BVH (latency bound).  Path regeneration keeps ~pool paths in flight per
// workgroup until its samples run out; only then do the rounds shrink, and once a round fits one wave the other
// waves leave the kernel (their registers and wave slots start workgroups of the next batch) and wave 0 finishes the
// long paths alone, without barriers.
// Exit condition every wave reaches: no rays, no shadow rays and no samples left (every path ends: a bounce ends it
// with probability >= 1 % from bounce rr_start on, and max_bounces caps it).
#ifndef HJ_TAIL1
#define HJ_TAIL1 128u    // rays of a round at which the workgroup shrinks to one wave (sweep 64..256: within 1 %)
#endif
#ifndef HJ_PATH_WAVES
#define HJ_PATH_WAVES 7   // 72 VGPRs; measured on the compacted-record kernel: 6 waves (80 VGPRs) -6 %, 8 waves (64 VGPRs) -2 %, 5 waves -5 %
#endif
// The kernel's text is hj_path_kernel.h, instantiated twice: k_path_wavefront, and k_path_wavefront_env for a scene with an
// environment (ENV: a miss bin in the compaction, environment light in shade).  Two kernels of one text rather than a fourth template
// flag, so that the first keeps its name and its code.  (One HJ_DEV body template with ENV as a fourth parameter, called from two thin
// kernels, was tried: every path kernel comes out a few instructions different, profiles/NOTES.md "Environment twins folded".)
#define HJ_PATH_KERNEL k_path_wavefront
#define HJ_PATH_ENV false
#include "hj_path_kernel.h"
#undef HJ_PATH_KERNEL
#undef HJ_PATH_ENV
#define HJ_PATH_KERNEL k_path_wavefront_env
#define HJ_PATH_ENV true
#include "hj_path_kernel.h"
#undef HJ_PATH_KERNEL
#undef HJ_PATH_ENV

// ---- split-kernel path (HJ_RENDER_SPLIT_KERNELS): the same stage functions, one launch per stage per bounce, for
// per-stage timing and counters.  No regeneration: the pool holds every sample of the workgroup (api/render.hip sizes
// it so) and k_gen_camera starts them all.

__global__ __launch_bounds__(kBlockThreads) void k_gen_camera(BatchState st, DeviceScene sc) {
  __shared__ WgShared sh;
  const uint32_t g = blockIdx.x;
  if (threadIdx.x == 0) sh.n_gen = 0;
  __syncthreads();
  stage_gen_camera<false>(st, sc, g, sh, 0, 0, 0, wg_num_groups(st, g), blockDim.x >> 6);
  __syncthreads();
  if (threadIdx.x == 0) {
    st.cnt_ray[0][g] = sh.n_gen;
    st.cnt_shadow[g] = 0;
    st.acc_closest[g] = 0;
    st.acc_shadow[g] = 0;
    st.acc_hits[g] = 0;
    st.acc_unoccluded[g] = 0;
    st.acc_direct[g] = 0;
  }
}

// ENV: st.cnt_hit holds kNumTags + 1 words per workgroup, the miss bin last.
template <bool USE_BVH, bool ENV>
HJ_DEV void trace_closest(const BatchState& st, const DeviceScene& sc, uint32_t parity) {
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
  const uint32_t g = blockIdx.x;
  const uint32_t n = st.cnt_ray[parity][g];
  if (threadIdx.x == 0) { sh.head = 0; sh.n_unocc = 0; }
  if (threadIdx.x < kNumTags) sh.cnt_hit[threadIdx.x] = 0;
  if (USE_BVH && n != 0) load_hot_nodes(sc, sh);
  __syncthreads();
  stage_trace_merged<USE_BVH, true, false>(st, sc, g, parity, n, 0, sh);
  compact_hits_by_tag<false, 4u, ENV>(st, sc, g, n, sh, blockDim.x >> 6);
  __syncthreads();
  constexpr uint32_t kBins = kNumTags + (ENV ? 1u : 0u);
  if (threadIdx.x < kNumTags) st.cnt_hit[g * kBins + threadIdx.x] = sh.cnt_hit[threadIdx.x];
  if (ENV && threadIdx.x == kMissBin) st.cnt_hit[g * kBins + kMissBin] = static_cast<WgSharedEnv&>(sh).cnt_miss;
  if (threadIdx.x == 0) {
    st.acc_closest[g] += n;
    uint32_t hits = 0;
    for (uint32_t k = 0; k < kNumTags; k++) hits += sh.cnt_hit[k];
    st.acc_hits[g] += hits;
  }
}

template <bool USE_BVH>
__global__ __launch_bounds__(kBlockThreads) void k_trace_closest(BatchState st, DeviceScene sc, uint32_t parity) {
  trace_closest<USE_BVH, false>(st, sc, parity);
}
template <bool USE_BVH>
__global__ __launch_bounds__(kBlockThreads) void k_trace_closest_env(BatchState st, DeviceScene sc, uint32_t parity) {
  trace_closest<USE_BVH, true>(st, sc, parity);
}

template <bool USE_BVH>
__global__ __launch_bounds__(kBlockThreads) void k_trace_shadow(BatchState st, DeviceScene sc) {
  __shared__ WgShared sh;
  const uint32_t g = blockIdx.x;
  const uint32_t ns = st.cnt_shadow[g];
  if (threadIdx.x == 0) { sh.head = 0; sh.n_unocc = 0; }
  if (USE_BVH && ns != 0) load_hot_nodes(sc, sh);
  __syncthreads();
  stage_trace_merged<USE_BVH, true, false>(st, sc, g, 0, 0, ns, sh);
  __syncthreads();
  if (threadIdx.x == 0) st.acc_unoccluded[g] += sh.n_unocc;
}

template <bool ENV>
HJ_DEV void shade(const BatchState& st, const DeviceScene& sc, uint32_t parity, uint32_t max_bounces, uint32_t rr_start) {
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
  const uint32_t g = blockIdx.x;
  constexpr uint32_t kBins = kNumTags + (ENV ? 1u : 0u);
  if (threadIdx.x == 0) { sh.n_ray[parity ^ 1u] = 0; sh.n_shadow = 0; sh.n_direct = 0; sh.cam_first = 0xFFFFFFFFu; sh.cam_k0 = 0; }   // (every camera path has records here)
  if (threadIdx.x < kNumTags) sh.cnt_hit[threadIdx.x] = st.cnt_hit[g * kBins + threadIdx.x];
  if (ENV && threadIdx.x == kMissBin) static_cast<WgSharedEnv&>(sh).cnt_miss = st.cnt_hit[g * kBins + kMissBin];
  __syncthreads();
  stage_shade<false, ENV>(st, sc, g, parity, max_bounces, rr_start, sh, blockDim.x >> 6);
  __syncthreads();
  if (threadIdx.x == 0) {
    st.cnt_ray[parity ^ 1u][g] = sh.n_ray[parity ^ 1u];
    st.cnt_shadow[g] = sh.n_shadow;
    st.acc_shadow[g] += sh.n_shadow + sh.n_direct;
    st.acc_unoccluded[g] += sh.n_direct;
    st.acc_direct[g] += sh.n_direct;
  }
}

__global__ __launch_bounds__(kBlockThreads) void k_shade(BatchState st, DeviceScene sc, uint32_t parity,
                                                         uint32_t max_bounces, uint32_t rr_start) {
  shade<false>(st, sc, parity, max_bounces, rr_start);
}
__global__ __launch_bounds__(kBlockThreads) void k_shade_env(BatchState st, DeviceScene sc, uint32_t parity,
                                                             uint32_t max_bounces, uint32_t rr_start) {
  shade<true>(st, sc, parity, max_bounces, rr_start);
}

// Probe kernel behind hj_debug_trace: arbitrary rays -> raw hit records.
template <bool USE_BVH, bool ANYHIT>
__global__ __launch_bounds__(kBlockThreads) void k_debug_trace(DeviceScene sc, const float* __restrict__ rays, uint32_t n,
                                                               float4* __restrict__ hits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r8 = rays + (size_t)i * 8;
  Ray r; r.o = V(r8[0], r8[1], r8[2]); r.d = V(r8[3], r8[4], r8[5]); r.tmin = r8[6]; r.tmax = r8[7];
  RawHit h; h.t = 0.f; h.u = 0.f; h.v = 0.f;
  const bool hit = traverse<USE_BVH, ANYHIT>(sc, r, h);
  hits[i] = make_float4(__int_as_float(hit ? h.id : -1), hit ? h.t : 0.f, hit ? h.u : 0.f, hit ? h.v : 0.f);
}

}  // namespace hj
