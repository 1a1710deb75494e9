// Order-preserving compaction of a list in tiles of one workgroup each: THE text of its three pieces, for the k_pa_* kernels of
// api/path_adaptive.hip (the active entries of a round's list) and the k_lm_* kernels of kernels/hj_lightmap.h (the owned texels).
//   count    one workgroup per tile: compact_wave_counts, then counts[tile] = compact_tile_count
//   scan     ONE workgroup: compact_scan_tiles
//   scatter  one workgroup per tile: compact_wave_counts again, then a kept entry goes to HJ_COMPACT_RANK
// Three launches: no workgroup ever waits for another.  kThreads: the threads of the workgroup = the entries of a tile, whole waves.
// Ordinary loads and stores, workgroup barriers, no inline assembly, no global atomic.
#pragma once
#include "hj_num.h"

namespace hj {

// Per wave the ballot of `keep` and its popcount: wave_cnt[kThreads / 64] in LDS, complete behind the ONE barrier every thread of
// the workgroup reaches here.  -> the own wave's ballot
HJ_DEV unsigned long long compact_wave_counts(bool keep, uint32_t* wave_cnt) {
  const unsigned long long mask = __ballot(keep);
  if ((threadIdx.x & 63u) == 0u) wave_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
  __syncthreads();
  return mask;
}

// The kept entries of the tile
template <uint32_t kThreads>
HJ_DEV uint32_t compact_tile_count(const uint32_t* wave_cnt) {
  uint32_t sum = wave_cnt[0];
#pragma unroll
  for (uint32_t w = 1; w < kThreads / 64u; w++) sum += wave_cnt[w];
  return sum;
}

// counts[0, nb) -> their exclusive prefix sums in place, counts[nb] = the total (the caller sees to it that it fits a uint32).
// One workgroup: thread t owns the `per` consecutive counts from t * per, sums them, the kThreads partial sums are scanned in LDS
// (Hillis-Steele, workgroup barriers only), and every thread walks its counts again.
template <uint32_t kThreads>
HJ_DEV void compact_scan_tiles(uint32_t* __restrict__ counts, uint32_t nb) {
  __shared__ uint32_t part[2][kThreads];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nb + kThreads - 1u) / kThreads;
  const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
  uint32_t sum = 0;
  for (uint32_t b = lo; b < hi; b++) sum += counts[b];
  uint32_t cur = 0;
  part[0][t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {
    part[cur ^ 1u][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0u);
    cur ^= 1u;
    __syncthreads();
  }
  uint32_t run = part[cur][t] - sum;          // (exclusive)
  for (uint32_t b = lo; b < hi; b++) {
    const uint32_t v = counts[b];
    counts[b] = run;
    run += v;
  }
  if (t == kThreads - 1u) counts[nb] = part[cur][t];
}

// The rank of a lane that keeps its entry, declared as `pos`: the tile's offset + the kept entries below the lane in its own wave's
// ballot + those of the earlier waves.  wave_cnt, mask: compact_wave_counts'.  A macro: the text is compiled in the kernel's own body,
// as api/query_round_loop.h's is - as an inlined device function it turned a branch of k_pa_scatter around ("Adaptive
// path queries").
#define HJ_COMPACT_RANK(pos, tile_offset, wave_cnt, mask)                                               \
  uint32_t pos = (tile_offset) + (uint32_t)__popcll((mask) & ((1ull << (threadIdx.x & 63u)) - 1ull));   \
  for (uint32_t w_ = 0; w_ < (threadIdx.x >> 6); w_++) pos += (wave_cnt)[w_]

}  // namespace hj
