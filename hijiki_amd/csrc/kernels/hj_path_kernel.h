// The fused path kernel, meant to be included more than once (no include guard): hj_kernels.h instantiates it twice, HJ_PATH_KERNEL = the
// kernel's name, HJ_PATH_ENV = the environment flag.
template <bool USE_BVH, bool PAIRS, bool NT>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(HJ_PATH_WAVES, 8))) void HJ_PATH_KERNEL(BatchState st, DeviceScene sc, uint32_t max_bounces,
                                                                  uint32_t rr_start) {
  constexpr bool ENV = HJ_PATH_ENV;
  // NT (large trees): the path state is streamed past the caches (ldp / stp)
  __shared__ std::conditional_t<ENV, WgSharedEnv, WgShared> sh;
  const uint32_t g = blockIdx.x;
  // (the called stages read the batch and scene descriptions from this kernel's argument segment and reach `sh` through its LDS address)
  const uint64_t ka_ = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t ka_lo = (uint32_t)ka_, ka_hi = (uint32_t)(ka_ >> 32), sh_lds = (uint32_t)(uintptr_t)(WgSharedLds)&sh;
  // Camera paths without records: kernels that have the packet stage (BVH walk over a tree with pair nodes)
  constexpr bool IMPLICIT = USE_BVH && PAIRS;
  RoundProbe rp;
  uint32_t groups_left = wg_num_groups(st, g);
  uint32_t total_closest = 0, total_shadow = 0, total_hits = 0, total_unocc = 0, total_direct = 0;   // (thread 0's copies are published)
  if (groups_left != 0) {
    uint32_t k_next = 0;                     // next group of this workgroup's sample sequence
    if (threadIdx.x == 0) { sh.n_ray[0] = 0; sh.n_ray[1] = 0; sh.n_gen = 0; sh.n_shadow = 0; sh.n_unocc = 0; sh.n_direct = 0; sh.cam_first = 0xFFFFFFFFu; sh.cam_k0 = 0; sh.n_cam_dead = 0; }
    if (USE_BVH) load_hot_nodes(sc, sh);
    uint32_t waves = blockDim.x >> 6;
    wg_sync(waves);
    for (uint32_t parity = 0;; parity ^= 1u) {
      // top-up: new camera paths behind the continuing ones, whole 64-sample groups while they fit.  IMPLICIT (kernels with
      // the packet stage): nothing is written - positions [n0, n0 + 64 * ngen) simply ARE the samples of groups k0 ... of the
      // workgroup's sequence; the packet stage builds their rays and shade rebuilds the paths that hit (camera_ray).
      const uint32_t n0 = uni(sh.n_ray[parity]);
      const uint32_t ngen = min(groups_left, (st.pool - n0) >> 6);
      const uint32_t k0 = k_next;
      if (ngen != 0) {
        if (!IMPLICIT) {
          rp.gen_begin();
          stage_gen_camera_call<NT, ENV>(ka_lo, ka_hi, g, sh_lds, parity, n0, k_next, ngen, waves);
          wg_sync(waves);
          rp.gen_end(waves);
        }
        k_next += ngen;
        groups_left -= ngen;
      }
      const uint32_t n = IMPLICIT ? n0 + 64u * ngen : n0 + uni(sh.n_gen), ns = uni(sh.n_shadow);
      // next-event samples of the previous round's shade that the light-shaft grid answered (intersectScene(shadowRay) == false
      // without a walk): shadow rays of the statistics all the same
      { const uint32_t nd = uni(sh.n_direct); total_shadow += nd; total_unocc += nd; total_direct += nd; }
      if (n + ns == 0) {
        if (groups_left == 0) break;
        // every sample of the new groups lay outside its block: next groups.  The other parity's path count is the one the
        // round before last left behind (only a round that reaches the reset below clears it): it must not be found again.
        if (threadIdx.x == 0) { sh.n_ray[parity ^ 1u] = 0; sh.n_direct = 0; }   // (n_direct: counted above, by thread 0, whose totals are the ones published)
        wg_sync(waves);
        continue;
      }
      // Tail of the workgroup: one wave can hold every ray of a round and the counts never grow again.
      if (waves > 1u && groups_left == 0 && n + ns <= HJ_TAIL1) {
        wg_sync(waves);                      // (everyone has read the counts)
        if (threadIdx.x >= 64u) return;
        waves = 1u;
      }
      rp.round_begin(n + ns);
      wg_sync(waves);                        // everyone has read the counts before they are reset
      if (threadIdx.x == 0) {
        sh.head = 0; sh.head_cam = 0; sh.n_ray[parity ^ 1u] = 0; sh.n_gen = 0; sh.n_shadow = 0; sh.n_unocc = 0; sh.n_direct = 0;
        sh.cam_first = (IMPLICIT && ngen != 0) ? n0 : 0xFFFFFFFFu; sh.cam_k0 = k0; sh.n_cam_dead = 0;
      }
      if (threadIdx.x < kNumTags) sh.cnt_hit[threadIdx.x] = 0;
      wg_sync(waves);
      rp.walk_begin();
      // the round's new camera rays are the LAST entries of the closest-hit queue: they are walked as packets of 64
      // (stage_camera_packets: one group of a block row each), the merged walk takes the continuing paths and the shadow rays
      uint32_t cam = 0;
      if (IMPLICIT && ngen != 0) {
        cam = 64u * ngen;
        stage_camera_packets_call<NT, ENV>(ka_lo, ka_hi, g, parity, n0, ngen, k0, sh_lds);
      }
      stage_trace_merged<USE_BVH, PAIRS, NT>(st, sc, g, parity, n - cam, ns, sh);
      rp.walk_end(waves);
      compact_hits_call<NT, 4u, ENV>(ka_lo, ka_hi, g, n, sh_lds, waves);
      wg_sync(waves);
      rp.compact_end();
      if (n != 0) {
        stage_shade_call<NT, ENV>(ka_lo, ka_hi, g, parity, max_bounces, rr_start, sh_lds, waves);
      }
      total_closest += n - uni(sh.n_cam_dead);   // (positions of ragged blocks' groups that hold no sample are not rays)
      total_shadow += ns;
      for (uint32_t k = 0; k < kNumTags; k++) total_hits += uni(sh.cnt_hit[k]);
      total_unocc += uni(sh.n_unocc);
      wg_sync(waves);
      rp.round_end(waves);
    }
  }
  if (threadIdx.x == 0) {
    st.acc_closest[g] = total_closest;
    st.acc_shadow[g] = total_shadow;
    st.acc_hits[g] = total_hits;
    st.acc_unoccluded[g] = total_unocc;
    st.acc_direct[g] = total_direct;
  }
}
