// The rounds of a specular chain ("Followed AOVs", "Followed motion"): THE text of what the followed AOVs
// (kernels/hj_follow.h) and the followed motion image (kernels/hj_motion_follow.h) do between their first walk and their resolve.  The
// continuation is hj_follow.h's (follow_continue_branch, follow_live), the compaction hj_compact.h's, the walk's shell
// hj_walk_segment.h's - included here and edited nowhere.  No global atomics, no inline assembly of its own.
//   k_chain_count / _scan    the live chains of n slots, per tile of kChainThreads, and their offsets; ONE copy in the library:
//                            api/follow.hip instantiates them, every other unit defines HJ_CHAIN_NO_KERNELS and launches them through
//                            chain_count_enqueue (api/hj_internal.h)
//   chain_scatter<FIRST>     the body of k_af_scatter / k_mf_scatter: the live slots in ascending order as a list; the first round's
//                            also sets every slot's chain state from the ray its caller's hook gives
//   chain_round<PAIRS>       the body of k_aov_follow / k_mf_follow: the persistent walk over the list with a fetch that continues a
//                            chain from its state and last hit - no ray array exists - and a finish that stores the new hit
// The chain state of a slot, two float4 beside its hit record: (segment origin.xyz, depth so far) (segment direction.xyz,
// continuations taken as bits).
#pragma once
#ifndef HJ_FOLLOW_NO_KERNELS
#define HJ_FOLLOW_NO_KERNELS   // the functions of hj_follow.h alone (api/follow.hip enters here from behind them)
#endif
#include "hj_follow.h"
#include "hj_compact.h"
#include "hj_walk_segment.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kChainThreads = 256u;            // threads of a count / scan / scatter workgroup: a compaction tile

#ifndef HJ_CHAIN_NO_KERNELS

// The live slots of n in tiles of kChainThreads (the last may be ragged: follow_live says no beyond n); counts: a word per tile and
// the total behind them (the host reads it: it sizes the round's grid).
template <bool FIRST>
__global__ __launch_bounds__(kChainThreads) void k_chain_count(DeviceScene sc, const float4* __restrict__ hits, const float4* __restrict__ state, uint32_t n,
                                                               uint32_t max_follow, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kChainThreads / 64u];
  (void)compact_wave_counts(follow_live<FIRST>(sc, hits, state, blockIdx.x * kChainThreads + threadIdx.x, n, max_follow), wave_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = compact_tile_count<kChainThreads>(wave_cnt);
}

__global__ __launch_bounds__(kChainThreads) void k_chain_scan(uint32_t* __restrict__ counts, uint32_t nb) { compact_scan_tiles<kChainThreads>(counts, nb); }

#endif  // HJ_CHAIN_NO_KERNELS

// One workgroup of kChainThreads per tile.  FIRST: behind the first walk no state exists yet; first_ray(slot, o, d) gives the ray that
// walk took for slot (< n), or false for a slot without one, and the slot's state becomes that ray, depth 0, no continuation - so the
// resolve reads one kind of record for every slot with a ray -; listed(slot) is the caller's own first-round work for a live slot.
template <bool FIRST, class FirstRay, class Listed>
HJ_DEV void chain_scatter(const DeviceScene& sc, const float4* __restrict__ hits, float4* __restrict__ state, uint32_t n, uint32_t max_follow,
                          const uint32_t* __restrict__ offsets, uint32_t* __restrict__ list, FirstRay first_ray, Listed listed) {
  __shared__ uint32_t wave_cnt[kChainThreads / 64u];
  const uint32_t slot = blockIdx.x * kChainThreads + threadIdx.x;
  if (FIRST && slot < n) {
    v3 o = V(0.f, 0.f, 0.f), d = o;
    if (first_ray(slot, o, d)) {
      state[2 * (size_t)slot] = make_float4(o.x, o.y, o.z, 0.f);
      state[2 * (size_t)slot + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(0u));
    }
  }
  const bool keep = follow_live<FIRST>(sc, hits, state, slot, n, max_follow);
  const unsigned long long mask = compact_wave_counts(keep, wave_cnt);
  if (!keep) return;
  if (FIRST) listed(slot);
  HJ_COMPACT_RANK(pos, offsets[blockIdx.x], wave_cnt, mask);
  list[pos] = slot;
}

// One round over the `count` live slots of list: workgroup g walks list entries [g * wg_rays, ...) (walk_segment).  fetch: the
// chain's state and last hit -> follow_continue_branch -> the walk's ray (p, wo, eps, +inf); the state becomes the new segment's
// (p, depth + t | wo, continuations + 1) and the hit record what on_continue(slot, n, reflected) returns - what the caller's resolve
// needs of the surface that was left should the new segment hit nothing; the hook also does the caller's own work for the slot.  The
// walk's finish hook sees the hit and not the ray, so the segment is stored here, in the service phase, where the walk issues its
// stores anyway.  finish: a hit replaces the record; a miss leaves it.  A slot is in the list once, so one lane reads and writes its
// records; which lane or workgroup carried a chain shows in no result.
template <bool PAIRS, class OnContinue>
HJ_DEV void chain_round(const DeviceScene& sc, const uint32_t* __restrict__ list, uint32_t count, uint32_t wg_rays, float4* __restrict__ hits,
                        float4* __restrict__ state, OnContinue on_continue) {
  auto fetch = [&](uint32_t q, uint32_t& slot, Ray& r, bool& any, RawHit& h) {
    slot = list[q];
    any = false;
    const float4 s0 = state[2 * (size_t)slot], s1 = state[2 * (size_t)slot + 1];
    const float4 hr = hits[slot];
    v3 p = V(0.f, 0.f, 0.f), wo = p, nrm = p;
    bool reflected = false;
    const bool go = follow_continue_branch(sc, xyz(s0), xyz(s1), hr, p, wo, nrm, reflected);   // (true for every entry the scatter listed)
    r.o = p;
    r.d = wo;
    walk_empty_range(r, go);
    if (go) {
      state[2 * (size_t)slot] = make_float4(p.x, p.y, p.z, s0.w + hr.y);
      state[2 * (size_t)slot + 1] = make_float4(wo.x, wo.y, wo.z, __uint_as_float(__float_as_uint(s1.w) + 1u));
      hits[slot] = on_continue(slot, nrm, reflected);
    }
    walk_reset(h);
  };
  auto finish = [&](bool done, uint32_t slot, const RawHit& h, bool) {
    if (done && h.id >= 0) hits[slot] = walk_hit_record(h);
  };
  walk_segment<0, PAIRS>(sc, count, wg_rays, fetch, finish);
}

}  // namespace hj
