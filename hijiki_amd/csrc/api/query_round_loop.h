// The round loop of a query's path kernel, meant to be included more than once (no include guard), INSIDE a kernel body: k_pq_paths
// (api/path_query.hip) and k_gq_paths (api/gather_query.hip) are their `__shared__ ... sh;` line and this file.  The including body has
//   PAIRS, ENV            its template parameters
//   st, sc, q             its arguments: BatchState, DeviceScene, and the query's own (src, spp, num_samples, max_bounces, rr_start)
//   sh                    the workgroup's WgShared / WgSharedEnv
//   HJ_QUERY_TOP_UP       the top-up, a called stage: (ka_lo, ka_hi, src_lo, src_hi, spp, num_samples, g, sh_lds, parity, n0, k0, ngen,
//                         waves); the includer #undef's it behind the include
// One text compiled in each kernel's own body, not a device function both call: blockDim.x is read with the kernel's launch bound
// only there, and where it is read decides how the prologue is scheduled ("One text for the round loop").
//
// The whole life of a chunk of samples in ONE launch: the round loop of kernels/hj_path_kernel.h for explicit records (its
// non-IMPLICIT form), with the includer's top-up.  Path regeneration keeps about `pool` paths in flight per workgroup until its
// samples run out.  sh.cam_first stays 0xFFFFFFFF in every round: no path is implicit, so no stage reads st.blocks (null here).
// Exit condition every wave reaches, exactly as in the path kernel: the counts a round's decisions depend on (n_ray, n_gen,
// n_shadow in LDS, groups_left in every thread alike) are read by all waves between two workgroup barriers, so all waves take the
// same branch; the loop ends when there are no rays, no shadow rays and no groups left, and every path ends - a bounce ends it with
// probability >= 1 % from bounce rr_start on, and max_bounces caps it.  A wave that leaves at the one-wave tail leaves for good: the
// counts never grow again once groups_left is 0.
// No global atomic, no inline assembly; ordinary loads and stores (NT = false).  The statistics are per workgroup, summed on the host.
  const uint32_t g = blockIdx.x;
  // (the called stages read the batch and scene descriptions from this kernel's argument segment and reach `sh` through its LDS address)
  const uint64_t ka_ = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t ka_lo = (uint32_t)ka_, ka_hi = (uint32_t)(ka_ >> 32), sh_lds = (uint32_t)(uintptr_t)(WgSharedLds)&sh;
  const uint32_t src_lo = (uint32_t)(uintptr_t)q.src, src_hi = (uint32_t)((uint64_t)(uintptr_t)q.src >> 32);
  uint32_t groups_left = query_num_groups(q.num_samples, st.num_wg, g);
  uint32_t total_closest = 0, total_shadow = 0, total_hits = 0, total_unocc = 0, total_direct = 0;   // (thread 0's copies are published)
  if (groups_left != 0) {
    uint32_t k_next = 0;                     // next group of this workgroup's sample sequence
    if (threadIdx.x == 0) { sh.n_ray[0] = 0; sh.n_ray[1] = 0; sh.n_gen = 0; sh.n_shadow = 0; sh.n_unocc = 0; sh.n_direct = 0; sh.cam_first = 0xFFFFFFFFu; sh.cam_k0 = 0; sh.n_cam_dead = 0; }
    load_hot_nodes(sc, sh);
    uint32_t waves = blockDim.x >> 6;
    wg_sync(waves);
    for (uint32_t parity = 0;; parity ^= 1u) {
      // top-up: new paths behind the continuing ones, whole 64-sample groups while they fit
      const uint32_t n0 = uni(sh.n_ray[parity]);
      const uint32_t ngen = min(groups_left, (st.pool - n0) >> 6);
      if (ngen != 0) {
        HJ_QUERY_TOP_UP(ka_lo, ka_hi, src_lo, src_hi, q.spp, q.num_samples, g, sh_lds, parity, n0, k_next, ngen, waves);
        wg_sync(waves);
        k_next += ngen;
        groups_left -= ngen;
      }
      const uint32_t n = n0 + uni(sh.n_gen), ns = uni(sh.n_shadow);
      // next-event samples of the previous round's shade that the light-shaft grid answered: shadow rays of the statistics all the same
      { const uint32_t nd = uni(sh.n_direct); total_shadow += nd; total_unocc += nd; total_direct += nd; }
      if (n + ns == 0) {
        if (groups_left == 0) break;
        // (not reached - every group below the chunk's count holds a sample -, kept as the path kernel has it)
        if (threadIdx.x == 0) { sh.n_ray[parity ^ 1u] = 0; sh.n_direct = 0; }
        wg_sync(waves);
        continue;
      }
      // Tail of the workgroup: one wave can hold every ray of a round and the counts never grow again.
      if (waves > 1u && groups_left == 0 && n + ns <= kQueryTail) {
        wg_sync(waves);                      // (everyone has read the counts)
        if (threadIdx.x >= 64u) return;
        waves = 1u;
      }
      wg_sync(waves);                        // everyone has read the counts before they are reset
      if (threadIdx.x == 0) {
        sh.head = 0; sh.head_cam = 0; sh.n_ray[parity ^ 1u] = 0; sh.n_gen = 0; sh.n_shadow = 0; sh.n_unocc = 0; sh.n_direct = 0;
        sh.cam_first = 0xFFFFFFFFu; sh.cam_k0 = 0; sh.n_cam_dead = 0;
      }
      if (threadIdx.x < kNumTags) sh.cnt_hit[threadIdx.x] = 0;
      wg_sync(waves);
      stage_trace_merged<true, PAIRS, false>(st, sc, g, parity, n, ns, sh);
      compact_hits_call<false, 4u, ENV>(ka_lo, ka_hi, g, n, sh_lds, waves);
      wg_sync(waves);
      if (n != 0) {
        stage_shade_call<false, ENV>(ka_lo, ka_hi, g, parity, q.max_bounces, q.rr_start, sh_lds, waves);
      }
      total_closest += n;
      total_shadow += ns;
      for (uint32_t k = 0; k < kNumTags; k++) total_hits += uni(sh.cnt_hit[k]);
      total_unocc += uni(sh.n_unocc);
      wg_sync(waves);
    }
  }
  if (threadIdx.x == 0) {
    st.acc_closest[g] = total_closest;
    st.acc_shadow[g] = total_shadow;
    st.acc_hits[g] = total_hits;
    st.acc_unoccluded[g] = total_unocc;
    st.acc_direct[g] = total_direct;
  }
