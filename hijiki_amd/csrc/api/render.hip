// The launches of the kernels (kernels/hj_kernels.h): the path kernel, the split path's stages, the reconstruction, the trace
// probe, and the readers of the walk-statistics counters.  The only unit that includes the kernels; the render calls around
// these launches (batch slots, hj_render_*, the worker) are host code in api/render_calls.hip.
#include "hj_internal.h"
#include "../kernels/hj_kernels.h"

#pragma clang fp contract(off)

namespace hjapi {

// Default path: ONE persistent launch per batch.  A scene with an environment takes the instantiations with the miss bin.
using PathKernel = void (*)(hj::BatchState, hj::DeviceScene, uint32_t, uint32_t);
template <bool USE_BVH, bool PAIRS, bool NT>
static PathKernel path_kernel(bool env) { return env ? hj::k_path_wavefront_env<USE_BVH, PAIRS, NT> : hj::k_path_wavefront<USE_BVH, PAIRS, NT>; }

void launch_path_wavefront(const hj::BatchState& st, const hj::DeviceScene& sc, const hj_render_opts& o, size_t lds_bytes, hipStream_t s) {
  const bool pairs = sc.has_pairs != 0, nt = sc.stream_state != 0, env = sc.env_alias != nullptr;
  const PathKernel k = !o.use_bvh ? path_kernel<false, false, false>(env)
                       : pairs ? (nt ? path_kernel<true, true, true>(env) : path_kernel<true, true, false>(env))
                               : (nt ? path_kernel<true, false, true>(env) : path_kernel<true, false, false>(env));
  hipLaunchKernelGGL(k, dim3(st.num_wg), dim3(hj::kBlockThreads), lds_bytes, s, st, sc, o.max_bounces, o.rr_start);
}

// Diagnostic path (HJ_RENDER_SPLIT_KERNELS): one launch per stage per bounce.
void launch_gen_camera(const hj::BatchState& st, const hj::DeviceScene& sc, hipStream_t s) {
  hipLaunchKernelGGL(hj::k_gen_camera, dim3(st.num_wg), dim3(hj::kBlockThreads), 0, s, st, sc);
}

void launch_trace_closest(const hj::BatchState& st, const hj::DeviceScene& sc, bool bvh, uint32_t parity, hipStream_t s) {
  const dim3 blk(hj::kBlockThreads), grid(st.num_wg);
  if (sc.env_alias && bvh) hipLaunchKernelGGL(hj::k_trace_closest_env<true>, grid, blk, 0, s, st, sc, parity);
  else if (sc.env_alias) hipLaunchKernelGGL(hj::k_trace_closest_env<false>, grid, blk, 0, s, st, sc, parity);
  else if (bvh) hipLaunchKernelGGL(hj::k_trace_closest<true>, grid, blk, 0, s, st, sc, parity);
  else hipLaunchKernelGGL(hj::k_trace_closest<false>, grid, blk, 0, s, st, sc, parity);
}

void launch_shade(const hj::BatchState& st, const hj::DeviceScene& sc, uint32_t parity, const hj_render_opts& o, hipStream_t s) {
  if (sc.env_alias) hipLaunchKernelGGL(hj::k_shade_env, dim3(st.num_wg), dim3(hj::kBlockThreads), 0, s, st, sc, parity, o.max_bounces, o.rr_start);
  else hipLaunchKernelGGL(hj::k_shade, dim3(st.num_wg), dim3(hj::kBlockThreads), 0, s, st, sc, parity, o.max_bounces, o.rr_start);
}

void launch_trace_shadow(const hj::BatchState& st, const hj::DeviceScene& sc, bool bvh, hipStream_t s) {
  const dim3 blk(hj::kBlockThreads), grid(st.num_wg);
  if (bvh) hipLaunchKernelGGL(hj::k_trace_shadow<true>, grid, blk, 0, s, st, sc);
  else hipLaunchKernelGGL(hj::k_trace_shadow<false>, grid, blk, 0, s, st, sc);
}

// One workgroup per 16x16 pixel tile.
void launch_reconstruct(const hj::BatchState& st, float stddev, const uint32_t* tiles, uint32_t tiles_x, uint32_t tiles_y,
                        float4* accum, uint32_t width, uint32_t height, hipStream_t s) {
  hipLaunchKernelGGL(hj::k_reconstruct, dim3(tiles_x, tiles_y), dim3(256), 0, s, st, stddev, tiles,
                     tiles + (size_t)tiles_x * tiles_y + 1, accum, width, height);
}

void launch_debug_trace(const hj::DeviceScene& sc, const float* rays, uint32_t n, bool bvh, bool any_hit, float4* hits, hipStream_t s) {
  const dim3 grid((n + hj::kBlockThreads - 1) / hj::kBlockThreads), blk(hj::kBlockThreads);
  if (bvh && any_hit) hipLaunchKernelGGL((hj::k_debug_trace<true, true>), grid, blk, 0, s, sc, rays, n, hits);
  else if (bvh) hipLaunchKernelGGL((hj::k_debug_trace<true, false>), grid, blk, 0, s, sc, rays, n, hits);
  else if (any_hit) hipLaunchKernelGGL((hj::k_debug_trace<false, true>), grid, blk, 0, s, sc, rays, n, hits);
  else hipLaunchKernelGGL((hj::k_debug_trace<false, false>), grid, blk, 0, s, sc, rays, n, hits);
}

}  // namespace hjapi

#ifdef HJ_WALK_STATS
extern "C" {
__attribute__((visibility("default"))) int hj_debug_round_stats(unsigned long long out[32], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hj::g_round_stats), 32 * sizeof(unsigned long long)) != hipSuccess) return HJ_ERR_DEVICE;
  if (reset) {
    unsigned long long z[32] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(hj::g_round_stats), z, sizeof z) != hipSuccess) return HJ_ERR_DEVICE;
  }
  return HJ_OK;
}
__attribute__((visibility("default"))) int hj_debug_walk_stats(unsigned long long out[16], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hj::g_walk_stats), 16 * sizeof(unsigned long long)) != hipSuccess) return HJ_ERR_DEVICE;
  if (reset) {
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(hj::g_walk_stats), z, sizeof z) != hipSuccess) return HJ_ERR_DEVICE;
  }
  return HJ_OK;
}
}  // extern "C"
#endif
