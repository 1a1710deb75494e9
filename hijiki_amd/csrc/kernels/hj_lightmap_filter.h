// The light-map filter ("Light-map filter"; include/hijiki_hip.h: hj_filter_lightmap), for the unit
// api/lightmap_filter.hip: an edge-avoiding a-trous filter over an atlas, guided by the gather points' positions and normals.
//   k_lm_guide          one thread per point: position, normal and a valid word to the dense per-texel guide (zeroed before)
//   k_lm_filter_direct  one a-trous iteration, one thread per texel, every tap loaded from memory
//   k_lm_filter_lds     the same iteration on the lattice of one residue class modulo the step: tile and apron staged in LDS
// Both forms call lm_tap, THE text of a tap, in the same order, so which one ran never shows in a bit.  Every operation is float32,
// one rounding each, uncontracted.  Ordinary loads and stores, no inline assembly, no global atomic.
#pragma once
#include "hj_lightmap_const.h"

#pragma clang fp contract(off)

namespace hj {

// The guide: two float4 per texel t - [2 t] = (P, valid word: 0 = not guided), [2 t + 1] = (n, 0) - so a tap is one aligned 32-byte
// read beside its 16 bytes of colour, and a texel that is not guided costs the valid word alone.
struct LmFilterArgs {
  const float4* guide;
  const float4* in;             // the iteration's input image I ...
  float4* out;                  // ... and its output O (never the same buffer)
  uint32_t W, H, s;             // s: the step, 1 << i
  float ip, in_, ic;            // 1 / sigma^2 of position, normal and this iteration's colour stop; 0 = off
};

constexpr uint32_t kLfTX = 32u, kLfTY = 8u;                   // texels of a workgroup's tile: 256 threads, a wave is two rows
constexpr uint32_t kLfCX = kLfTX + 4u, kLfCY = kLfTY + 4u;    // ... with its apron of two taps on every side (k_lm_filter_lds)

struct LmAcc { float r, g, b, w; };

HJ_DEV float lm_sq(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
HJ_DEV float lm_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One tap q of the texel (P, n, c), spline weight h: include/hijiki_hip.h's steps 3 - 6
HJ_DEV void lm_tap(LmAcc& acc, v3 P, v3 n, v3 c, v3 Pq, v3 nq, v3 cq, float h, const LmFilterArgs& a) {
  const float e = (lm_sq(Pq - P) * a.ip + lm_sq(nq - n) * a.in_) + lm_sq(cq - c) * a.ic;
  const float w = h * hj_exp(-e);
  acc.r = acc.r + cq.x * w;
  acc.g = acc.g + cq.y * w;
  acc.b = acc.b + cq.z * w;
  acc.w = acc.w + w;
}

HJ_DEV bool lm_guided(const float4* guide, uint32_t t) { return reinterpret_cast<const uint32_t*>(guide)[8u * (size_t)t + 3u] != 0u; }

// One thread per point; the guide holds zeros before.  A word 7 that names no texel of the atlas is skipped.
__global__ __launch_bounds__(kLmThreads) void k_lm_guide(const float4* __restrict__ points, uint32_t count, uint32_t n, float4* __restrict__ guide) {
  const uint32_t i = blockIdx.x * kLmThreads + threadIdx.x;
  if (i >= count) return;
  const float4 r0 = points[2 * (size_t)i], r1 = points[2 * (size_t)i + 1];
  const uint32_t t = __float_as_uint(r1.w);
  if (t >= n) return;
  guide[2 * (size_t)t] = make_float4(r0.x, r0.y, r0.z, __uint_as_float(1u));
  guide[2 * (size_t)t + 1] = make_float4(r0.w, r1.x, r1.y, 0.0f);
}

// Grid (ceil(W / 32), ceil(H / 8)): thread (i, j) of a workgroup is texel (32 bx + i, 8 by + j).  Every tap is loaded from memory:
// the valid word first, guide and colour only behind it; the lanes of a row read contiguous segments at every step.
__global__ __launch_bounds__(kLfTX * kLfTY) void k_lm_filter_direct(LmFilterArgs a) {
  const uint32_t x = blockIdx.x * kLfTX + (threadIdx.x & (kLfTX - 1u)), y = blockIdx.y * kLfTY + threadIdx.x / kLfTX;
  if (x >= a.W || y >= a.H) return;
  const uint32_t t = y * a.W + x;
  const float4 ci = a.in[t];
  if (!lm_guided(a.guide, t)) {
    a.out[t] = ci;
    return;
  }
  const float4 g0 = a.guide[2 * (size_t)t], g1 = a.guide[2 * (size_t)t + 1];
  const v3 P = xyz(g0), n = xyz(g1), c = xyz(ci);
  LmAcc acc{0.f, 0.f, 0.f, 0.f};
  const int s = (int)a.s;
  for (int dy = -2; dy <= 2; dy++) {
    const int yy = (int)y + dy * s;
    if (yy < 0 || yy >= (int)a.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int xx = (int)x + dx * s;
      if (xx < 0 || xx >= (int)a.W) continue;
      const uint32_t q = (uint32_t)yy * a.W + (uint32_t)xx;
      if (!lm_guided(a.guide, q)) continue;
      const float4 q0 = a.guide[2 * (size_t)q], q1 = a.guide[2 * (size_t)q + 1], cq = a.in[q];
      lm_tap(acc, P, n, c, xyz(q0), xyz(q1), xyz(cq), lm_k(dx) * lm_k(dy), a);
    }
  }
  a.out[t] = make_float4(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, ci.w);
}

// The texels with x = rx, y = ry modulo s form a lattice on which the taps of step s are the taps of step 1: a workgroup takes a
// 32 x 8 tile of ONE lattice and stages the tile and its apron of two - guide and rgb, 40 bytes a cell, 17 280 bytes a workgroup at
// every step - in LDS.  Grid (s * tiles_x, s * tiles_y), tiles_x = ceil(ceil(W / s) / 32), tiles_y = ceil(ceil(H / s) / 8): block
// (rx * tiles_x + tx, ry * tiles_y + ty).  A cell outside the atlas or not guided holds a zero valid word (and read nothing more).
__global__ __launch_bounds__(kLfTX * kLfTY) void k_lm_filter_lds(LmFilterArgs a, uint32_t tiles_x, uint32_t tiles_y) {
  __shared__ float4 s_p[kLfCX * kLfCY];       // (P, valid word)
  __shared__ float4 s_n[kLfCX * kLfCY];       // (n, c.r)
  __shared__ float2 s_c[kLfCX * kLfCY];       // (c.g, c.b)
  const uint32_t rx = blockIdx.x / tiles_x, ry = blockIdx.y / tiles_y;
  const int s = (int)a.s;
  const int lx0 = (int)((blockIdx.x - rx * tiles_x) * kLfTX), ly0 = (int)((blockIdx.y - ry * tiles_y) * kLfTY);   // lattice coordinates
  for (uint32_t k = threadIdx.x; k < kLfCX * kLfCY; k += kLfTX * kLfTY) {
    const uint32_t cj = k / kLfCX, ci = k - cj * kLfCX;
    const int xx = (int)rx + s * (lx0 + (int)ci - 2), yy = (int)ry + s * (ly0 + (int)cj - 2);   // (|.| < 2^15 + 34 * 128)
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), nn = p;
    float2 cc = make_float2(0.f, 0.f);
    if (xx >= 0 && yy >= 0 && xx < (int)a.W && yy < (int)a.H) {
      const uint32_t q = (uint32_t)yy * a.W + (uint32_t)xx;
      if (lm_guided(a.guide, q)) {
        const float4 q1 = a.guide[2 * (size_t)q + 1], cq = a.in[q];
        p = a.guide[2 * (size_t)q];
        nn = make_float4(q1.x, q1.y, q1.z, cq.x);
        cc = make_float2(cq.y, cq.z);
      }
    }
    s_p[k] = p;
    s_n[k] = nn;
    s_c[k] = cc;
  }
  __syncthreads();
  const uint32_t i = threadIdx.x & (kLfTX - 1u), j = threadIdx.x / kLfTX;
  const uint32_t x = rx + a.s * ((uint32_t)lx0 + i), y = ry + a.s * ((uint32_t)ly0 + j);
  if (x >= a.W || y >= a.H) return;
  const uint32_t t = y * a.W + x;
  const float4 ci = a.in[t];
  const uint32_t home = (j + 2u) * kLfCX + (i + 2u);
  const float4 g0 = s_p[home];
  if (__float_as_uint(g0.w) == 0u) {
    a.out[t] = ci;
    return;
  }
  const v3 P = xyz(g0), n = xyz(s_n[home]), c = xyz(ci);
  LmAcc acc{0.f, 0.f, 0.f, 0.f};
  for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const uint32_t k = (uint32_t)((int)home + dy * (int)kLfCX + dx);
      const float4 q0 = s_p[k];
      if (__float_as_uint(q0.w) == 0u) continue;
      const float4 q1 = s_n[k];
      const float2 q2 = s_c[k];
      lm_tap(acc, P, n, c, xyz(q0), xyz(q1), V(q1.w, q2.x, q2.y), lm_k(dx) * lm_k(dy), a);
    }
  }
  a.out[t] = make_float4(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, ci.w);
}

}  // namespace hj
