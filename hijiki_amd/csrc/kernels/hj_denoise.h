// The frame denoiser ("Frame denoiser"; include/hijiki_hip.h: hj_denoise_frame), for the unit api/denoise.hip: the
// variance-guided a-trous stage of SVGF over albedo-demodulated light, guided by a frame's AOV sums.
//   k_dn_prepare        one thread per pixel: which pixels are guided (none with a lit pixel in its 5 x 5 window), the dense guide -
//                       (n, z), (A, valid word) - and the working image (I, 0) or (c, 0)
//   k_dn_variance       one thread per pixel: the depth slope into the guide's third record, the 5 x 5 initial variance into word 3
//   k_dn_filter_direct  one a-trous iteration, one thread per pixel, every tap loaded from memory
//   k_dn_filter_lds     the same iteration on the lattice of one residue class modulo the step: tile and apron staged in LDS
//   k_dn_finish         the remodulation alone (iterations == 0; otherwise the last iteration's store does it)
// Both forms of the iteration call dn_centre, THE text of a pixel's own terms (the 3 x 3 variance smoothing at step 1 among them,
// always from memory: the lattice tile carries no step-1 neighbours), and dn_tap, THE text of a tap, in the same order, so which
// one ran never shows in a bit.  Every operation is float32, one rounding each, uncontracted.  Ordinary loads and stores, no
// inline assembly, no global atomic.  Shares no kernel with hj_lightmap_filter.h (its spline and sq are restated here: including
// that header would define its kernels a second time).
//   (the kernels are left out under HJ_DENOISE_NO_KERNELS: hj_denoise_temporal.h takes the functions alone)
#pragma once
#include "../../../include/hijiki_hip.h"
#include "hj_num.h"

#pragma clang fp contract(off)

namespace hj {

// The guide: three float4 per pixel t - [3 t] = (n, z), [3 t + 1] = (A, valid word: 0 = not guided), [3 t + 2] = (gz.x, gz.y, 0, 0)
// - so a tap is one aligned 32-byte read beside its 16 bytes of (I, V), and a pixel that is not guided costs the valid word alone.
struct DnArgs {
  const float4* guide;
  const float4* in;             // the iteration's input (I, V) ...
  float4* out;                  // ... and its output (never the same buffer)
  uint32_t W, H, s;             // s: the step, 1 << i
  float inn, sz, sl, ia;        // 1 / sigma^2 of normal and albedo, the sigmas of depth and luminance; 0 = off
  uint32_t finish;              // the last iteration: store (I' * A, V')
};

constexpr uint32_t kDnThreads = 256u;
constexpr uint32_t kDnTX = 32u, kDnTY = 8u;                   // pixels of a workgroup's tile: 256 threads, a wave is two rows
constexpr uint32_t kDnCX = kDnTX + 4u, kDnCY = kDnTY + 4u;    // ... with its apron of two taps on every side (k_dn_filter_lds)
constexpr float kDnAlbedoFloor = 0.015625f;

struct DnAcc { float r, g, b, vs, ws; };
// a guided pixel's own terms, the same for its 25 taps
struct DnCentre { v3 n, A; float z, lum, gzx, gzy, dl; };

HJ_DEV float dn_sq(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
HJ_DEV float dn_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
HJ_DEV float dn_lum(v3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
HJ_DEV bool dn_guided(const float4* guide, uint32_t t) { return reinterpret_cast<const uint32_t*>(guide)[12u * (size_t)t + 7u] != 0u; }

// The smaller of the forward difference zf - z and the backward difference z - zb; a tie takes the forward one
HJ_DEV float dn_slope(float z, bool has_f, float zf, bool has_b, float zb) {
  const float f = zf - z, b = z - zb;
  if (has_f && has_b) return __builtin_fabsf(b) < __builtin_fabsf(f) ? b : f;
  return has_f ? f : has_b ? b : 0.0f;
}

// The terms of the guided pixel (x, y): guide records g0, g1, its own (I, V) in ci; the 3 x 3 smoothing of V at step 1 from memory
HJ_DEV DnCentre dn_centre(const DnArgs& a, uint32_t x, uint32_t y, float4 g0, float4 g1, float4 ci) {
  float vsum = 0.0f, gsum = 0.0f;
  for (int dy = -1; dy <= 1; dy++) {
    const int yy = (int)y + dy;
    if (yy < 0 || yy >= (int)a.H) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int xx = (int)x + dx;
      if (xx < 0 || xx >= (int)a.W) continue;
      const uint32_t q = (uint32_t)yy * a.W + (uint32_t)xx;
      if (!dn_guided(a.guide, q)) continue;
      const float g = (dx == 0 && dy == 0) ? 0.25f : (dx == 0 || dy == 0) ? 0.125f : 0.0625f;
      vsum = vsum + a.in[q].w * g;
      gsum = gsum + g;
    }
  }
  const float sd = __builtin_sqrtf(vsum / gsum);
  const float4 g2 = a.guide[3 * (size_t)(y * a.W + x) + 2];
  return DnCentre{xyz(g0), xyz(g1), g0.w, dn_lum(xyz(ci)), g2.x, g2.y, a.sl * sd + 1e-6f};
}

// One tap q = p + s * (dx, dy) of the pixel p: include/hijiki_hip.h's steps 1 - 7 (fx = (float)(dx * s), fy = (float)(dy * s))
HJ_DEV void dn_tap(DnAcc& acc, const DnCentre& p, float4 q0, float4 q1, float4 cq, float h, float fx, float fy, const DnArgs& a) {
  const float en = dn_sq(xyz(q0) - p.n) * a.inn;
  const float ez = a.sz != 0.0f ? __builtin_fabsf(q0.w - p.z) / (a.sz * __builtin_fabsf(p.gzx * fx + p.gzy * fy) + 1e-6f) : 0.0f;
  const float el = a.sl != 0.0f ? __builtin_fabsf(dn_lum(xyz(cq)) - p.lum) / p.dl : 0.0f;
  const float ea = dn_sq(xyz(q1) - p.A) * a.ia;
  const float w = h * hj_exp(-(((en + ez) + el) + ea));
  acc.r = acc.r + cq.x * w;
  acc.g = acc.g + cq.y * w;
  acc.b = acc.b + cq.z * w;
  acc.vs = acc.vs + cq.w * (w * w);
  acc.ws = acc.ws + w;
}

HJ_DEV float4 dn_result(const DnAcc& acc, const DnCentre& p, const DnArgs& a) {
  const float r = acc.r / acc.ws, g = acc.g / acc.ws, b = acc.b / acc.ws, v = acc.vs / (acc.ws * acc.ws);
  return a.finish != 0u ? make_float4(r * p.A.x, g * p.A.y, b * p.A.z, v) : make_float4(r, g, b, v);
}

#ifndef HJ_DENOISE_NO_KERNELS   // (hj_denoise_temporal.h takes the functions above and leaves the kernels to api/denoise.hip)

// Grid (ceil(W / 32), ceil(H / 8)), one thread per pixel: aov is three float4 a pixel (albedo sum, samples | normal sum, depth sum |
// emission sum, hits).  A pixel with a lit pixel in its 5 x 5 window - the reach of the framebuffer's reconstruction filter - is
// not guided: the lit flags of the 32 x 8 tile and its apron of two are staged in LDS (one read of the third record a cell), then
// every thread looks at its 25.
__global__ __launch_bounds__(kDnTX * kDnTY) void k_dn_prepare(const float4* __restrict__ aov, const float4* __restrict__ beauty, uint32_t W, uint32_t H,
                                                             float4* __restrict__ guide, float4* __restrict__ img) {
  __shared__ uint32_t s_lit[kDnCX * kDnCY];   // a cell outside the image is not lit
  const uint32_t i = threadIdx.x & (kDnTX - 1u), j = threadIdx.x / kDnTX;
  const int x0 = (int)(blockIdx.x * kDnTX) - 2, y0 = (int)(blockIdx.y * kDnTY) - 2;
  for (uint32_t k = threadIdx.x; k < kDnCX * kDnCY; k += kDnTX * kDnTY) {
    const uint32_t cj = k / kDnCX, ci = k - cj * kDnCX;
    const int xx = x0 + (int)ci, yy = y0 + (int)cj;
    uint32_t l = 0u;
    if (xx >= 0 && yy >= 0 && xx < (int)W && yy < (int)H) {
      const float4 e = aov[3 * (size_t)((uint32_t)yy * W + (uint32_t)xx) + 2];
      l = (e.x > 0.0f || e.y > 0.0f || e.z > 0.0f) ? 1u : 0u;
    }
    s_lit[k] = l;
  }
  __syncthreads();
  const uint32_t x = blockIdx.x * kDnTX + i, y = blockIdx.y * kDnTY + j;
  if (x >= W || y >= H) return;
  const uint32_t t = y * W + x;
  const float4 a0 = aov[3 * (size_t)t], a1 = aov[3 * (size_t)t + 1], a2 = aov[3 * (size_t)t + 2], b = beauty[t];
  const float S = a0.w, Hc = a2.w, bw = b.w;
  v3 c = V(0.0f, 0.0f, 0.0f);
  if (bw > 0.0f) c = V(b.x / bw, b.y / bw, b.z / bw);
  uint32_t lit = 0u;
#pragma unroll
  for (uint32_t dy = 0; dy < 5u; dy++)
#pragma unroll
    for (uint32_t dx = 0; dx < 5u; dx++) lit |= s_lit[(j + dy) * kDnCX + (i + dx)];
  if (!(Hc > 0.0f && bw > 0.0f) || lit != 0u) {
    guide[3 * (size_t)t] = make_float4(0.f, 0.f, 0.f, 0.f);
    guide[3 * (size_t)t + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
    guide[3 * (size_t)t + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
    img[t] = make_float4(c.x, c.y, c.z, 0.0f);
    return;
  }
  const v3 A = V(f_max(a0.x / S, kDnAlbedoFloor), f_max(a0.y / S, kDnAlbedoFloor), f_max(a0.z / S, kDnAlbedoFloor));
  guide[3 * (size_t)t] = make_float4(a1.x / Hc, a1.y / Hc, a1.z / Hc, a1.w / Hc);
  guide[3 * (size_t)t + 1] = make_float4(A.x, A.y, A.z, __uint_as_float(1u));
  img[t] = make_float4(c.x / A.x, c.y / A.y, c.z / A.z, 0.0f);
}

// Grid (ceil(W / 32), ceil(H / 8)).  Reads the guide's first two records and in = (I, 0) of the 5 x 5 neighbourhood; writes the
// pixel's own third record and out = (I, V).
__global__ __launch_bounds__(kDnTX * kDnTY) void k_dn_variance(float4* __restrict__ guide, const float4* __restrict__ in, float4* __restrict__ out,
                                                              uint32_t W, uint32_t H) {
  const uint32_t x = blockIdx.x * kDnTX + (threadIdx.x & (kDnTX - 1u)), y = blockIdx.y * kDnTY + threadIdx.x / kDnTX;
  if (x >= W || y >= H) return;
  const uint32_t t = y * W + x;
  const float4 ci = in[t];
  if (!dn_guided(guide, t)) {
    out[t] = ci;
    return;
  }
  const float z = guide[3 * (size_t)t].w;
  const bool xf = x + 1u < W && dn_guided(guide, t + 1u), xb = x > 0u && dn_guided(guide, t - 1u);
  const bool yf = y + 1u < H && dn_guided(guide, t + W), yb = y > 0u && dn_guided(guide, t - W);
  const float gzx = dn_slope(z, xf, xf ? guide[3 * (size_t)(t + 1u)].w : 0.0f, xb, xb ? guide[3 * (size_t)(t - 1u)].w : 0.0f);
  const float gzy = dn_slope(z, yf, yf ? guide[3 * (size_t)(t + W)].w : 0.0f, yb, yb ? guide[3 * (size_t)(t - W)].w : 0.0f);
  float m1 = 0.0f, m2 = 0.0f, cnt = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int yy = (int)y + dy;
    if (yy < 0 || yy >= (int)H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int xx = (int)x + dx;
      if (xx < 0 || xx >= (int)W) continue;
      const uint32_t q = (uint32_t)yy * W + (uint32_t)xx;
      if (!dn_guided(guide, q)) continue;
      const float l = dn_lum(xyz(in[q]));
      m1 = m1 + l;
      m2 = m2 + l * l;
      cnt = cnt + 1.0f;
    }
  }
  const float mu = m1 / cnt;
  guide[3 * (size_t)t + 2] = make_float4(gzx, gzy, 0.0f, 0.0f);
  out[t] = make_float4(ci.x, ci.y, ci.z, f_max(m2 / cnt - mu * mu, 0.0f));
}

// Grid (ceil(W / 32), ceil(H / 8)): thread (i, j) of a workgroup is pixel (32 bx + i, 8 by + j).  Every tap is loaded from memory:
// the valid word first, guide and (I, V) only behind it; the lanes of a row read contiguous segments at every step.
__global__ __launch_bounds__(kDnTX * kDnTY) void k_dn_filter_direct(DnArgs a) {
  const uint32_t x = blockIdx.x * kDnTX + (threadIdx.x & (kDnTX - 1u)), y = blockIdx.y * kDnTY + threadIdx.x / kDnTX;
  if (x >= a.W || y >= a.H) return;
  const uint32_t t = y * a.W + x;
  const float4 ci = a.in[t];
  if (!dn_guided(a.guide, t)) {
    a.out[t] = ci;
    return;
  }
  const DnCentre p = dn_centre(a, x, y, a.guide[3 * (size_t)t], a.guide[3 * (size_t)t + 1], ci);
  DnAcc acc{0.f, 0.f, 0.f, 0.f, 0.f};
  const int s = (int)a.s;
  for (int dy = -2; dy <= 2; dy++) {
    const int yy = (int)y + dy * s;
    if (yy < 0 || yy >= (int)a.H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int xx = (int)x + dx * s;
      if (xx < 0 || xx >= (int)a.W) continue;
      const uint32_t q = (uint32_t)yy * a.W + (uint32_t)xx;
      if (!dn_guided(a.guide, q)) continue;
      dn_tap(acc, p, a.guide[3 * (size_t)q], a.guide[3 * (size_t)q + 1], a.in[q], dn_k(dx) * dn_k(dy), (float)(dx * s), (float)(dy * s), a);
    }
  }
  a.out[t] = dn_result(acc, p, a);
}

// The pixels with x = rx, y = ry modulo s form a lattice on which the taps of step s are the taps of step 1: a workgroup takes a
// 32 x 8 tile of ONE lattice and stages the tile and its apron of two - (n, z), (A, valid word), (I, V): 48 bytes a cell, 20 736
// bytes a workgroup at every step - in LDS.  Grid (s * tiles_x, s * tiles_y), tiles_x = ceil(ceil(W / s) / 32), tiles_y =
// ceil(ceil(H / s) / 8): block (rx * tiles_x + tx, ry * tiles_y + ty).  A cell outside the image or not guided holds a zero valid
// word (and read nothing more).
__global__ __launch_bounds__(kDnTX * kDnTY) void k_dn_filter_lds(DnArgs a, uint32_t tiles_x, uint32_t tiles_y) {
  __shared__ float4 s_n[kDnCX * kDnCY];       // (n, z)
  __shared__ float4 s_a[kDnCX * kDnCY];       // (A, valid word)
  __shared__ float4 s_c[kDnCX * kDnCY];       // (I, V)
  const uint32_t rx = blockIdx.x / tiles_x, ry = blockIdx.y / tiles_y;
  const int s = (int)a.s;
  const int lx0 = (int)((blockIdx.x - rx * tiles_x) * kDnTX), ly0 = (int)((blockIdx.y - ry * tiles_y) * kDnTY);   // lattice coordinates
  for (uint32_t k = threadIdx.x; k < kDnCX * kDnCY; k += kDnTX * kDnTY) {
    const uint32_t cj = k / kDnCX, ci = k - cj * kDnCX;
    const int xx = (int)rx + s * (lx0 + (int)ci - 2), yy = (int)ry + s * (ly0 + (int)cj - 2);   // (|.| < 2^15 + 34 * 128)
    float4 nn = make_float4(0.f, 0.f, 0.f, 0.f), aa = nn, cc = nn;
    if (xx >= 0 && yy >= 0 && xx < (int)a.W && yy < (int)a.H) {
      const uint32_t q = (uint32_t)yy * a.W + (uint32_t)xx;
      if (dn_guided(a.guide, q)) {
        nn = a.guide[3 * (size_t)q];
        aa = a.guide[3 * (size_t)q + 1];
        cc = a.in[q];
      }
    }
    s_n[k] = nn;
    s_a[k] = aa;
    s_c[k] = cc;
  }
  __syncthreads();
  const uint32_t i = threadIdx.x & (kDnTX - 1u), j = threadIdx.x / kDnTX;
  const uint32_t x = rx + a.s * ((uint32_t)lx0 + i), y = ry + a.s * ((uint32_t)ly0 + j);
  if (x >= a.W || y >= a.H) return;
  const uint32_t t = y * a.W + x;
  const uint32_t home = (j + 2u) * kDnCX + (i + 2u);
  const float4 g1 = s_a[home];
  if (__float_as_uint(g1.w) == 0u) {
    a.out[t] = a.in[t];
    return;
  }
  const DnCentre p = dn_centre(a, x, y, s_n[home], g1, s_c[home]);
  DnAcc acc{0.f, 0.f, 0.f, 0.f, 0.f};
  for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const uint32_t k = (uint32_t)((int)home + dy * (int)kDnCX + dx);
      const float4 q1 = s_a[k];
      if (__float_as_uint(q1.w) == 0u) continue;
      dn_tap(acc, p, s_n[k], q1, s_c[k], dn_k(dx) * dn_k(dy), (float)(dx * s), (float)(dy * s), a);
    }
  }
  a.out[t] = dn_result(acc, p, a);
}

// iterations == 0: out = (I * A, V) for a guided pixel, a copy otherwise
__global__ __launch_bounds__(kDnThreads) void k_dn_finish(const float4* __restrict__ guide, const float4* __restrict__ in, uint32_t n, float4* __restrict__ out) {
  const uint32_t t = blockIdx.x * kDnThreads + threadIdx.x;
  if (t >= n) return;
  const float4 ci = in[t], g1 = guide[3 * (size_t)t + 1];
  out[t] = __float_as_uint(g1.w) != 0u ? make_float4(ci.x * g1.x, ci.y * g1.y, ci.z * g1.z, ci.w) : ci;
}

#endif  // HJ_DENOISE_NO_KERNELS

}  // namespace hj
