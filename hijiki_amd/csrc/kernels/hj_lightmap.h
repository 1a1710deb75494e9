// Light-map baking ("Light-map baking"): the uploaded scene's triangle UVs rasterised into gather points, and the
// gather's records scattered back into an atlas image.  include/hijiki_hip.h (hj_lightmap_texels, hj_bake_lightmap) spells the
// arithmetic out; every operation here is float32, one rounding each, uncontracted, in that order.
//   lm_covers       THE text of the coverage predicate and its edge values: the owner kernel and the emit kernel both call it
//   k_lm_owner      per triangle its clamped, widened texel box; a small box is walked by the triangle's lane: atomicMin of the
//                   triangle index into every texel it covers; a large one is marked for
//   k_lm_owner_wide the marked boxes, each walked by whole waves of many grid rows
//   k_lm_count      per texel: the owner's normal; a texel whose normal is not finite or all zero loses its owner; owned texels
//                   counted per workgroup tile
//   k_lm_scan       ONE workgroup: the tiles' counts become exclusive offsets, the total behind them (the second level)
//   k_lm_emit       one thread per owned texel: its record at its rank, the owner map to the caller
//   k_lm_scatter    one thread per gather record: the scaled sum to the texel word 7 of its point names
//   k_lm_dilate     one gutter pass from one image into another
// Ordinary loads and stores and no inline assembly; the atomicMin of the two owner kernels is the one global atomic.  The compaction
// of count, scan and emit is kernels/hj_compact.h's text.
#pragma once
#include "hj_lightmap_const.h"
#include "hj_compact.h"

#pragma clang fp contract(off)

namespace hj {

struct LmUv { float au, av, bu, bv, cu, cv; };
struct LmEdges { float e0, e1, e2, s; };

struct LmArgs {
  const hj_triangle* tris;
  const hj_vertex* verts;
  uint32_t first, count;        // triangles [first, first + count)
  uint32_t W, H;
  uint32_t lane_texels;         // k_lm_owner: a box of at most this many texels is walked by one lane, a larger one by k_lm_owner_wide
  uint32_t seed, seed_stride;
  float offset;
};

HJ_DEV bool lm_finite(float x) { return __builtin_fabsf(x) < kInf; }

HJ_DEV LmUv lm_load_uv(const LmArgs& a, uint32_t tri) {
  const hj_triangle t = a.tris[tri];
  const hj_vertex* __restrict__ v = a.verts;
  return LmUv{v[t.v[0]].u, v[t.v[0]].v, v[t.v[1]].u, v[t.v[1]].v, v[t.v[2]].u, v[t.v[2]].v};
}

HJ_DEV float lm_centre(uint32_t i, uint32_t n) { return ((float)i + 0.5f) / (float)n; }

HJ_DEV float lm_edge(float su, float sv, float tu, float tv, float pu, float pv) { return (tu - su) * (pv - sv) - (tv - sv) * (pu - su); }

// Does the triangle cover the centre of texel (x, y)?  E: the edge values there, whatever the answer.
HJ_DEV bool lm_covers(const LmUv& t, uint32_t x, uint32_t y, uint32_t W, uint32_t H, LmEdges& E) {
  const float pu = lm_centre(x, W), pv = lm_centre(y, H);
  E.e0 = lm_edge(t.bu, t.bv, t.cu, t.cv, pu, pv);
  E.e1 = lm_edge(t.cu, t.cv, t.au, t.av, pu, pv);
  E.e2 = lm_edge(t.au, t.av, t.bu, t.bv, pu, pv);
  E.s = (E.e0 + E.e1) + E.e2;
  const bool finite = lm_finite(t.au) && lm_finite(t.av) && lm_finite(t.bu) && lm_finite(t.bv) && lm_finite(t.cu) && lm_finite(t.cv);
  const bool in_u = f_min(f_min(t.au, t.bu), t.cu) <= pu && pu <= f_max(f_max(t.au, t.bu), t.cu);
  const bool in_v = f_min(f_min(t.av, t.bv), t.cv) <= pv && pv <= f_max(f_max(t.av, t.bv), t.cv);
  const bool side = (E.e0 >= 0.f && E.e1 >= 0.f && E.e2 >= 0.f) || (E.e0 <= 0.f && E.e1 <= 0.f && E.e2 <= 0.f);
  return finite && in_u && in_v && side && E.s != 0.f;
}

// The texels [lo, hi] of one axis whose centres can lie in [vmin, vmax]: centre i is at (i + 0.5) / n, so i >= vmin * n - 0.5 and
// i <= vmax * n - 0.5.  The products and the centres round (a few 1e-7 of n <= 16384: under 0.01 texel), the range is widened by one
// whole texel on each side, so it holds every texel the closed comparison of lm_covers accepts; then clamped to the atlas.
HJ_DEV bool lm_axis_range(float vmin, float vmax, uint32_t n, int& lo, int& hi) {
  const float fn = (float)n;
  const float a = f_min(f_max(vmin * fn - 0.5f, -2.0f), fn + 2.0f), b = f_min(f_max(vmax * fn - 0.5f, -2.0f), fn + 2.0f);
  lo = max((int)__builtin_floorf(a) - 1, 0);
  hi = min((int)__builtin_ceilf(b) + 1, (int)n - 1);
  return lo <= hi;
}

HJ_DEV bool lm_box(const LmUv& t, uint32_t W, uint32_t H, int& x0, int& x1, int& y0, int& y1) {
  if (!(lm_finite(t.au) && lm_finite(t.av) && lm_finite(t.bu) && lm_finite(t.bv) && lm_finite(t.cu) && lm_finite(t.cv))) return false;
  const bool bx = lm_axis_range(f_min(f_min(t.au, t.bu), t.cu), f_max(f_max(t.au, t.bu), t.cu), W, x0, x1);
  const bool by = lm_axis_range(f_min(f_min(t.av, t.bv), t.cv), f_max(f_max(t.av, t.bv), t.cv), H, y0, y1);
  return bx && by;
}

// The owner map must hold kLmNone everywhere before the two launches.  Wave w takes the 64-triangle groups w, w + waves, ...; a triangle
// whose box holds at most lane_texels texels is walked by its lane, here; the larger ones of group g are left, as a bit each of
// masks[g], to k_lm_owner_wide.  The minimum does not depend on the order, so neither the grid nor the split shows in the map.
// (A texel index is below 2^26, a box below 2^28 texels.)
__global__ __launch_bounds__(kLmThreads) void k_lm_owner(LmArgs a, uint32_t* owner, unsigned long long* __restrict__ masks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (kLmThreads / 64u);
  for (uint64_t base = ((uint64_t)blockIdx.x * (kLmThreads / 64u) + (threadIdx.x >> 6)) * 64u; base < a.count; base += waves * 64u) {
    const uint64_t j = base + lane;
    LmUv t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    bool has = false;
    if (j < a.count) {
      t = lm_load_uv(a, a.first + (uint32_t)j);
      has = lm_box(t, a.W, a.H, x0, x1, y0, y1);
    }
    const uint32_t area = has ? (uint32_t)(x1 - x0 + 1) * (uint32_t)(y1 - y0 + 1) : 0u;
    const bool by_lane = has && area <= a.lane_texels;
    const unsigned long long big = __ballot(has && !by_lane);
    if (lane == 0u) masks[base >> 6] = big;
    if (by_lane) {
      const uint32_t idx = a.first + (uint32_t)j;
      LmEdges E;
      for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++)
          if (lm_covers(t, (uint32_t)x, (uint32_t)y, a.W, a.H, E)) atomicMin(&owner[(uint32_t)y * a.W + (uint32_t)x], idx);
    }
  }
}

// The boxes k_lm_owner left: grid (gx, rows).  Wave w of every row reads the masks of 64 groups at a time - a lane each, groups
// 64 w, 64 (w + waves), ... - so a row that finds nothing to do has made a load or two per wave, and walks each marked triangle's box
// with the whole wave: texel k of the box (row-major) is lane k % 64's in row (k / 64) % rows.  So one chart over the whole atlas is
// spread over all rows however many small triangles surround it.
__global__ __launch_bounds__(kLmThreads) void k_lm_owner_wide(LmArgs a, const unsigned long long* __restrict__ masks, uint32_t groups, uint32_t* owner) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (kLmThreads / 64u);
  const uint32_t row = blockIdx.y, rows = gridDim.y;
  for (uint32_t g0 = (blockIdx.x * (kLmThreads / 64u) + (threadIdx.x >> 6)) * 64u; g0 < groups; g0 += waves * 64u) {   // (groups <= 2^26: no wrap)
    const unsigned long long mine = g0 + lane < groups ? masks[g0 + lane] : 0ull;
    unsigned long long any = __ballot(mine != 0ull);
    while (any) {
      const int gl = __ffsll((long long)any) - 1;
      any &= any - 1ull;
      unsigned long long big = ((unsigned long long)(uint32_t)__shfl((int)(mine >> 32), gl) << 32) | (uint32_t)__shfl((int)(mine & 0xFFFFFFFFull), gl);
      while (big) {
        const uint32_t src = (uint32_t)__ffsll((long long)big) - 1u;
        big &= big - 1ull;
        const uint32_t idx = a.first + (g0 + (uint32_t)gl) * 64u + src;   // (group * 64 + src is below a.count)
        const LmUv t = lm_load_uv(a, idx);
        int x0, x1, y0, y1;
        if (!lm_box(t, a.W, a.H, x0, x1, y0, y1)) continue;               // (never: the bit says it has one)
        const uint32_t bw = (uint32_t)(x1 - x0 + 1), area = bw * (uint32_t)(y1 - y0 + 1);
        LmEdges E;
        for (uint32_t k = row * 64u + lane; k < area; k += rows * 64u) {
          const uint32_t ry = k / bw, x = (uint32_t)x0 + (k - ry * bw), y = (uint32_t)y0 + ry;
          if (lm_covers(t, x, y, a.W, a.H, E)) atomicMin(&owner[y * a.W + x], idx);
        }
      }
    }
  }
}

// The record of texel t under its owner `tri`, from the edge values lm_covers gives there: hu = e1 / s, hv = e2 / s, l0 = (1 - hu) -
// hv; position and normal interpolated in populate_triangle's expressions (kernels/hj_shade.h).  false: the normal has a
// non-finite component or is all zero - the texel has no owner.
HJ_DEV bool lm_record(const LmArgs& a, uint32_t tri, uint32_t t, float4& r0, float4& r1) {
  const hj_triangle ix = a.tris[tri];
  const hj_vertex A = a.verts[ix.v[0]], B = a.verts[ix.v[1]], C = a.verts[ix.v[2]];
  const LmUv uv{A.u, A.v, B.u, B.v, C.u, C.v};
  const uint32_t y = t / a.W, x = t - y * a.W;
  LmEdges E;
  (void)lm_covers(uv, x, y, a.W, a.H, E);
  const float hu = E.e1 / E.s, hv = E.e2 / E.s;
  const float l0 = (1.0f - hu) - hv;
  const v3 P = (V(A.pos[0], A.pos[1], A.pos[2]) * l0 + V(B.pos[0], B.pos[1], B.pos[2]) * hu) + V(C.pos[0], C.pos[1], C.pos[2]) * hv;
  const v3 n = normalize3((V(A.normal[0], A.normal[1], A.normal[2]) * l0 + V(B.normal[0], B.normal[1], B.normal[2]) * hu) +
                          V(C.normal[0], C.normal[1], C.normal[2]) * hv);
  if (!(lm_finite(n.x) && lm_finite(n.y) && lm_finite(n.z)) || (n.x == 0.f && n.y == 0.f && n.z == 0.f)) return false;
  const v3 p = P + n * a.offset;
  r0 = make_float4(p.x, p.y, p.z, n.x);
  r1 = make_float4(n.y, n.z, __uint_as_float(a.seed + t * a.seed_stride), __uint_as_float(t));
  return true;
}

// One thread per texel (n = W * H): a texel whose record fails for its normal gets its owner word reset; counts[workgroup] = the
// texels of the tile that keep an owner.
__global__ __launch_bounds__(kLmThreads) void k_lm_count(LmArgs a, uint32_t n, uint32_t* __restrict__ owner, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[kLmThreads / 64u];
  const uint32_t t = blockIdx.x * kLmThreads + threadIdx.x;
  bool owned = false;
  if (t < n) {
    const uint32_t o = owner[t];
    if (o != kLmNone) {
      float4 r0, r1;
      owned = lm_record(a, o, t, r0, r1);
      if (!owned) owner[t] = kLmNone;
    }
  }
  (void)compact_wave_counts(owned, wave_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = compact_tile_count<kLmThreads>(wave_cnt);
}

// The tiles' counts -> their exclusive offsets, the total behind them.  (A total is at most W * H <= 2^26.)
__global__ __launch_bounds__(kLmThreads) void k_lm_scan(uint32_t* __restrict__ counts, uint32_t nb) { compact_scan_tiles<kLmThreads>(counts, nb); }

// One thread per texel: an owned texel writes its record at rank offsets[tile] + the owned texels of the tile before it, so the
// records stand in ascending texel order.  Nothing is written when the total (offsets[nb]) exceeds `capacity`: the caller learns
// the count and is refused.  points == NULL: no records; owner_out == NULL: no copy of the map.
__global__ __launch_bounds__(kLmThreads) void k_lm_emit(LmArgs a, uint32_t n, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ offsets,
                                                        uint32_t nb, uint64_t capacity, float4* __restrict__ points, uint32_t* __restrict__ owner_out) {
  __shared__ uint32_t wave_cnt[kLmThreads / 64u];
  const uint32_t t = blockIdx.x * kLmThreads + threadIdx.x;
  const uint32_t o = t < n ? owner[t] : kLmNone;
  const bool owned = o != kLmNone;
  const unsigned long long mask = compact_wave_counts(owned, wave_cnt);
  if (points && (uint64_t)offsets[nb] > capacity) return;
  if (owner_out && t < n) owner_out[t] = o;
  if (!owned || !points) return;
  HJ_COMPACT_RANK(pos, offsets[blockIdx.x], wave_cnt, mask);
  float4 r0, r1;
  (void)lm_record(a, o, t, r0, r1);
  points[2 * (size_t)pos] = r0;
  points[2 * (size_t)pos + 1] = r1;
}

// One thread per gather record i (api/gather_query.hip: words 0-2 the sums): texel = word 7 of point i; the image holds zeros before.
__global__ __launch_bounds__(kLmThreads) void k_lm_scatter(const float4* __restrict__ points, const float4* __restrict__ records, uint32_t n, float scale,
                                                           float4* __restrict__ image) {
  const uint32_t i = blockIdx.x * kLmThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = __float_as_uint(points[2 * (size_t)i + 1].w);
  const float4 r = records[2 * (size_t)i];
  image[t] = make_float4(r.x * scale, r.y * scale, r.z * scale, 1.0f);
}

// One gutter pass: a texel with alpha == 0 and at least one 8-neighbour with alpha > 0 becomes the mean of those neighbours' rgb
// (summed from +0 in the order dy = -1, 0, 1 outer, dx = -1, 0, 1 inner; one division per channel) with alpha 0.5; every other
// texel is copied.  Neighbours outside the atlas do not exist.
__global__ __launch_bounds__(kLmThreads) void k_lm_dilate(const float4* __restrict__ in, float4* __restrict__ out, uint32_t W, uint32_t H) {
  const uint32_t t = blockIdx.x * kLmThreads + threadIdx.x;
  if (t >= W * H) return;
  const int y = (int)(t / W), x = (int)(t - (uint32_t)y * W);
  float4 c = in[t];
  if (c.w == 0.f) {
    float r = 0.f, g = 0.f, b = 0.f;
    uint32_t k = 0;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int xx = x + dx, yy = y + dy;
        if ((dx == 0 && dy == 0) || xx < 0 || yy < 0 || xx >= (int)W || yy >= (int)H) continue;
        const float4 v = in[(uint32_t)yy * W + (uint32_t)xx];
        if (v.w > 0.f) { r += v.x; g += v.y; b += v.z; k++; }
      }
    if (k != 0u) c = make_float4(r / (float)k, g / (float)k, b / (float)k, 0.5f);
  }
  out[t] = c;
}

}  // namespace hj
