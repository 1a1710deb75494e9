// Direct-lit frames ("Direct-lit frames"; include/hijiki_hip.h hj_render_direct_lit): hj_render_probe_lit's samples with one
// traced next-event sample at each chain's last diffuse hit.  The sample is the shade stage's (sample_emitter<ENV>, kernels/hj_shade.h),
// its value the shade stage's at throughput 1, its shadow ray the shade stage's (tMin = 2 eps, tMax = stmax, any-hit).  The segment, the
// side record and the compose of Lp are kernels/hj_probe_lit.h's, the compaction hj_compact.h's, the walk's shell hj_walk_segment.h's -
// included here and edited nowhere.  No global atomics, no inline assembly of its own.
//   k_dl_sample<ENV>      one lane per sample slot of a walk launch: the slot's shadow ray and its pending D, or a record that says none
//   k_dl_count / _scan    the slots that want a ray, per tile of kDlThreads, and their offsets
//   k_dl_scatter          those slots in ascending order as a list
//   k_dl_shadow<PAIRS>    the persistent any-hit walk over the list: a hit clears the slot's pending D
//   k_dl_resolve          k_pl_resolve with L = Lp + D where D still stands
// The record of a slot, three float4: (p.xyz, 0) (sdir.xyz, stmax) (D.rgb, kDlPending or kDlNone as bits).
#pragma once
#define HJ_PROBE_LIT_NO_KERNELS   // the functions of hj_probe_lit.h (and through it of hj_follow.h and hj_aov.h), no kernel of theirs
#include "hj_probe_lit.h"
#include "hj_compact.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kDlThreads = 256u;   // threads of a count / scan / scatter workgroup: a compaction tile
constexpr uint32_t kDlNone = 0u;        // word 3 of a slot's third record: no direct term, or its shadow ray found something
constexpr uint32_t kDlPending = 1u;     // ... D stands unless the shadow ray finds something
static_assert(kSlotsPerBlock % kDlThreads == 0, "a launch's sample slots are whole tiles");

// rays: three float4 per slot.  The hit point, the normal and the albedo are the ones k_pl_points and aov_record build (populate_* on
// fma(t, d, o) over the chain's last segment, eval_material); rng = rng_seed(block.seed + lx + ly * dimension.x), the state camera_ray
// leaves for a slot pl_segment has accepted; the condition and D = ((albedo * dot(n, sdir)) * kInvPi) * imp are stage_shade's
// (hj_stages.h:539-543) with T = 1.  The light-shaft grid is not asked: every wanted ray is walked.
template <bool ENV>
__global__ __launch_bounds__(kBlockThreads) void k_dl_sample(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                             const float4* __restrict__ hits, const float4* __restrict__ state,
                                                             float4* __restrict__ rays) {
  const uint32_t smp = blockIdx.x * blockDim.x + threadIdx.x;
  if (smp >= num_blocks * kSlotsPerBlock) return;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = make_float4(0.f, 0.f, 0.f, __uint_as_float(kDlNone));
  v3 o, d;
  if (pl_segment(sc, blocks, num_blocks, state, smp, o, d)) {
    const float4 hr = hits[smp];
    const uint32_t id = __float_as_uint(hr.x);
    if (id < sc.ns + sc.nq + sc.nt) {
      const uint32_t tag = sc.materials[id] >> HJ_MATERIAL_TAG_SHIFT;
      if (tag == HJ_MAT_DIFFUSE || tag == HJ_MAT_DIFFUSECBOARD || tag == HJ_MAT_DIFFUSE_TEXTURED) {
        Its its;
        its.p = V(fmaf(hr.y, d.x, o.x), fmaf(hr.y, d.y, o.y), fmaf(hr.y, d.z, o.z));
        if (id < sc.ns) populate_sphere(sc.spheres[id], its);
        else if (id < sc.ns + sc.nq) populate_quad(sc, id - sc.ns, hr.z, hr.w, its);
        else populate_triangle(sc, id - sc.ns - sc.nq, hr.z, hr.w, its);
        v3 albedo, emission;
        uint32_t word;
        eval_material(sc, id, its.u, its.v, albedo, emission, word);
        const hj_image_block b = blocks[smp / kSlotsPerBlock];
        const uint32_t lx = smp & (HJ_BLOCK_SIZE - 1u), ly = (smp / HJ_BLOCK_SIZE) & (HJ_BLOCK_SIZE - 1u);
        uint32_t rng = rng_seed(b.seed + lx + ly * b.dimension[0]);                       // render.glsl:156
        v3 sdir = V(0.f, 0.f, 0.f);
        float stmax = 0.f;
        uint32_t em = 0;
        const v3 imp = sample_emitter<ENV>(sc, its.p, rng, sdir, stmax, em);
        if (len3(imp) > kEps && dot3(sdir, its.n) > 0.0f) {
          const float cs = dot3(its.n, sdir);
          const v3 f = (albedo * cs) * kInvPi;
          const v3 D = f * imp;
          r0 = make_float4(its.p.x, its.p.y, its.p.z, 0.f);
          r1 = make_float4(sdir.x, sdir.y, sdir.z, stmax);
          r2 = make_float4(D.x, D.y, D.z, __uint_as_float(kDlPending));
        }
      }
    }
  }
  rays[3 * (size_t)smp] = r0;
  rays[3 * (size_t)smp + 1] = r1;
  rays[3 * (size_t)smp + 2] = r2;
}

// does slot (of n, whole tiles) want a shadow ray?
HJ_DEV bool dl_wants(const float4* __restrict__ rays, uint32_t slot, uint32_t n) {
  return slot < n && __float_as_uint(rays[3 * (size_t)slot + 2].w) == kDlPending;
}

// counts: a word per tile and the total behind them (the host reads it: it sizes the walk's grid)
__global__ __launch_bounds__(kDlThreads) void k_dl_count(const float4* __restrict__ rays, uint32_t n, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kDlThreads / 64u];
  (void)compact_wave_counts(dl_wants(rays, blockIdx.x * kDlThreads + threadIdx.x, n), wave_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = compact_tile_count<kDlThreads>(wave_cnt);
}

__global__ __launch_bounds__(kDlThreads) void k_dl_scan(uint32_t* __restrict__ counts, uint32_t nb) { compact_scan_tiles<kDlThreads>(counts, nb); }

// One workgroup per tile: the slots that want a ray, in ascending order, at the tile's offset
__global__ __launch_bounds__(kDlThreads) void k_dl_scatter(const float4* __restrict__ rays, uint32_t n, const uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ list) {
  __shared__ uint32_t wave_cnt[kDlThreads / 64u];
  const uint32_t slot = blockIdx.x * kDlThreads + threadIdx.x;
  const bool keep = dl_wants(rays, slot, n);
  const unsigned long long mask = compact_wave_counts(keep, wave_cnt);
  if (!keep) return;
  HJ_COMPACT_RANK(pos, offsets[blockIdx.x], wave_cnt, mask);
  list[pos] = slot;
}

// The walk over the `count` listed slots: workgroup g walks list entries [g * wg_rays, ...) (walk_segment), any-hit - the walk's
// MODE 1, which ends a ray at the first shape it accepts; MODE 0 does not read the fetch's flag.  A slot is in the list once, so one
// lane writes its record; a hit clears the pending D, a miss leaves it.  Which lane or workgroup carried a ray shows in no result.
template <bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_dl_shadow(DeviceScene sc, const uint32_t* __restrict__ list, uint32_t count, uint32_t wg_rays,
                                                             float4* __restrict__ rays) {
  auto fetch = [&](uint32_t q, uint32_t& slot, Ray& r, bool& any, RawHit& h) {
    slot = list[q];
    any = true;
    const float4 a = rays[3 * (size_t)slot], b = rays[3 * (size_t)slot + 1];
    r.o = xyz(a);
    r.d = xyz(b);
    r.tmin = 2.0f * kEps;                                            // render.glsl:132; scene.glsl:85 (stage_trace_merged's shadow rays)
    r.tmax = b.w;
    walk_reset(h);
  };
  auto finish = [&](bool done, uint32_t slot, const RawHit& h, bool) {
    if (done && h.id >= 0) rays[3 * (size_t)slot + 2] = make_float4(0.f, 0.f, 0.f, __uint_as_float(kDlNone));
  };
  walk_segment<1, PAIRS>(sc, count, wg_rays, fetch, finish);
}

// k_pl_resolve over a run, with the direct term: Lp is k_pl_resolve's (lookup == nullptr - no volume -: the side record's alone), and
// L = Lp + D, one rounding a channel, where the slot's D still stands; otherwise L = Lp and no addition is taken.
__global__ __launch_bounds__(kBlockThreads) void k_dl_resolve(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                              uint32_t b0, uint32_t nb, const float4* __restrict__ hits,
                                                              const float4* __restrict__ state, const float4* __restrict__ lookup,
                                                              const float4* __restrict__ side, const float4* __restrict__ rays, uint32_t width,
                                                              uint32_t height, float4* __restrict__ image) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb * kSlotsPerBlock) return;
  const uint32_t smp = b0 * kSlotsPerBlock + j;
  v3 o, d;
  if (!pl_segment(sc, blocks, num_blocks, state, smp, o, d)) return;
  uint32_t px, py;
  if (!aov_pixel(blocks, smp, width, height, px, py)) return;
  const float4 sd = side[smp];
  v3 L = xyz(sd);
  if (lookup != nullptr && __float_as_uint(sd.w) == kPlDiffuse) L = pl_compose(sc, o, d, hits[smp], sd, lookup[smp]);
  const float4 dr = rays[3 * (size_t)smp + 2];
  if (__float_as_uint(dr.w) == kDlPending) L = V(L.x + dr.x, L.y + dr.y, L.z + dr.z);
  float4* p = image + ((size_t)py * width + px);
  float4 a = *p;
  a.x += L.x; a.y += L.y; a.z += L.z; a.w += 1.0f;
  *p = a;
}

}  // namespace hj
