// The temporal half of the frame denoiser ("Temporal accumulation"; include/hijiki_hip.h: hj_denoise_frame_temporal),
// for the unit api/denoise_temporal.hip: the history of the last frame reprojected into this one, in front of hj_denoise.h's filter.
//   k_dt_accumulate<MOTION>  one thread per pixel: the guided pixel's world point from its depth and its camera ray, projected into the
//                    previous camera (MOTION: the position and the distance come from the pixel's motion record, hj_motion.h's,
//                    instead); the four bilinear taps of the history that pass the depth and the normal test; the blend of
//                    light and luminance moments; the working image (I, 0) in place and the history record.  The unit launches
//                    <false>; <true> is instantiated by api/motion.hip alone (dt_accumulate_motion_enqueue)
//   k_dt_variance    k_dn_variance's text with one more branch: a pixel whose history is HJ_TEMPORAL_VARIANCE_FRAMES long takes the
//                    variance of its temporal moments, a younger one the 5 x 5 spatial estimate
//   k_dt_feedback    the first iteration's I' into the history record's light (HJ_TEMPORAL_FEEDBACK)
// The camera arithmetic is the shader's (render.glsl:26-36, quaternion.glsl:1-19, as hj_stages.h camera_ray restates it): its dot3
// and cross3 are hj_num.h's, fmaf and all.  Everything else is float32, one rounding each, uncontracted.  Ordinary loads and stores,
// no inline assembly, no global atomic; no LDS: the taps are data dependent, but neighbouring pixels reproject to neighbouring
// texels, so a row's loads stay in a few cache lines.
// HJ_DENOISE_TEMPORAL_NO_KERNELS leaves k_dt_variance and k_dt_feedback out: api/motion.hip takes the camera functions and the
// accumulate template alone.
#pragma once
#define HJ_DENOISE_NO_KERNELS   // the functions of hj_denoise.h; its kernels stay api/denoise.hip's
#include "hj_denoise.h"
#include "hj_num.h"

#pragma clang fp contract(off)

namespace hj {

// A history record: three float4 per pixel t - [3 t] = (I, N), [3 t + 1] = (m1, m2, z, valid word), [3 t + 2] = (n, 0)
struct DtCamera { v3 pos, qv; float qw, tan_half; };
struct DtArgs {
  const float4* guide;
  float4* img;                  // (I_cur, 0) on entry, (I, 0) on return, in place: a thread touches its own pixel alone
  const float4* hist_in;        // nullptr: no history
  const float4* motion;         // MOTION: (sx, sy, zp, id bits or HJ_MOTION_NONE) per pixel; otherwise not read
  float4* hist_out;
  uint32_t W, H;
  DtCamera cam, prev;
  float alpha, alpha_m, ztol, ncos, max_n;
};

// quaternionRotate(v, q) = (q (x) (v, 0)) (x) conj(q), quaternion.glsl:1-19, in camera_ray's operation order
HJ_DEV v3 dt_rotate(v3 vv, v3 qv, float qw) {
  const float tw = qw * 0.0f - dot3(qv, vv);
  const v3 c1 = cross3(qv, vv);
  const v3 txyz = V((c1.x + qv.x * 0.0f) + vv.x * qw, (c1.y + qv.y * 0.0f) + vv.y * qw, (c1.z + qv.z * 0.0f) + vv.z * qw);
  const v3 cq = -qv;
  const v3 c2 = cross3(txyz, cq);
  return V((c2.x + txyz.x * qw) + cq.x * tw, (c2.y + txyz.y * qw) + cq.y * tw, (c2.z + txyz.z * qw) + cq.z * tw);
}

// The normalised direction through the image point (px, py): camera_ray's arithmetic
HJ_DEV v3 dt_camera_dir(const DtCamera& c, float px, float py, float W, float H) {
  float x = px - 0.5f * W, y = py - 0.5f * H;
  x = (x * c.tan_half) / (0.5f * W);
  y = (y * c.tan_half) / (0.5f * W);
  return normalize3(dt_rotate(V(x, -y, -1.0f), c.qv, c.qw));
}

// the host's camera as the kernels take it: tan_half as the upload computes it (api/scene_upload.hip)
inline DtCamera dt_host_camera(const hj_camera& c) {
  return DtCamera{v3{c.position[0], c.position[1], c.position[2]}, v3{c.rotation[0], c.rotation[1], c.rotation[2]}, c.rotation[3],
                  (float)std::tan((double)(0.5f * c.fov) * (3.14159265358979323846 / 180.0))};
}

// Grid (ceil(W / 32), ceil(H / 8)), one thread per pixel.  Per history tap the valid word first, the three records only behind it.
// MOTION: (sx, sy, zp) are words 0, 1, 2 of the pixel's motion record, and a record whose word 3 is 0xFFFFFFFF (HJ_MOTION_NONE) gives
// no history; the text from fx on is one text for both.
template <bool MOTION>
__global__ __launch_bounds__(kDnTX * kDnTY) void k_dt_accumulate(DtArgs a) {
  const uint32_t x = blockIdx.x * kDnTX + (threadIdx.x & (kDnTX - 1u)), y = blockIdx.y * kDnTY + threadIdx.x / kDnTX;
  if (x >= a.W || y >= a.H) return;
  const uint32_t t = y * a.W + x;
  if (!dn_guided(a.guide, t)) {
    a.hist_out[3 * (size_t)t] = make_float4(0.f, 0.f, 0.f, 0.f);
    a.hist_out[3 * (size_t)t + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
    a.hist_out[3 * (size_t)t + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float4 g0 = a.guide[3 * (size_t)t], ci = a.img[t];
  const v3 n = xyz(g0), Ic = xyz(ci);
  const float z = g0.w;
  v3 sI = V(0.f, 0.f, 0.f);
  float sm1 = 0.0f, sm2 = 0.0f, sN = 0.0f, ws = 0.0f;
  if (a.hist_in != nullptr) {
    const float Wf = (float)a.W, Hf = (float)a.H;
    bool front;
    float sx, sy, zp;
    if constexpr (MOTION) {
      const float4 mv = a.motion[t];
      front = __float_as_uint(mv.w) != 0xFFFFFFFFu;
      sx = mv.x; sy = mv.y; zp = mv.z;
    } else {
      const v3 d = dt_camera_dir(a.cam, (float)x + 0.5f, (float)y + 0.5f, Wf, Hf);
      const v3 P = V(a.cam.pos.x + z * d.x, a.cam.pos.y + z * d.y, a.cam.pos.z + z * d.z);
      const v3 v = P - a.prev.pos;
      const v3 c = dt_rotate(v, -a.prev.qv, a.prev.qw);
      front = c.z < 0.0f;
      const float k = (0.5f * Wf) / a.prev.tan_half;
      sx = (c.x / -c.z) * k + 0.5f * Wf;
      sy = (-c.y / -c.z) * k + 0.5f * Hf;
      zp = __builtin_sqrtf(dn_sq(v));
    }
    if (front) {
      const float fx = sx - 0.5f, fy = sy - 0.5f;
      // ix = floorf(fx) in [-1, W - 1], iy likewise: otherwise no tap lies in the image (a NaN fails every comparison)
      if (fx >= -1.0f && fx < Wf && fy >= -1.0f && fy < Hf) {
        const float fix = __builtin_floorf(fx), fiy = __builtin_floorf(fy);
        const float tx = fx - fix, ty = fy - fiy;
        const int ix = (int)fix, iy = (int)fiy;
        const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(a.hist_in);
#pragma unroll
        for (int b = 0; b < 2; b++) {
#pragma unroll
          for (int e = 0; e < 2; e++) {
            const int xx = ix + e, yy = iy + b;
            if (xx < 0 || yy < 0 || xx >= (int)a.W || yy >= (int)a.H) continue;
            const size_t q = (size_t)((uint32_t)yy * a.W + (uint32_t)xx);
            if (hw[12u * q + 7u] == 0u) continue;
            const float4 h0 = a.hist_in[3 * q], h1 = a.hist_in[3 * q + 1], h2 = a.hist_in[3 * q + 2];
            if (!(__builtin_fabsf(h1.z - zp) <= a.ztol * zp)) continue;
            if (!((h2.x * n.x + h2.y * n.y) + h2.z * n.z >= a.ncos)) continue;
            const float w = wx[e] * wy[b];
            sI = V(sI.x + h0.x * w, sI.y + h0.y * w, sI.z + h0.z * w);
            sN = sN + h0.w * w;
            sm1 = sm1 + h1.x * w;
            sm2 = sm2 + h1.y * w;
            ws = ws + w;
          }
        }
      }
    }
  }
  v3 I = Ic;
  float m1 = dn_lum(Ic), N = 1.0f;
  float m2 = m1 * m1;
  if (ws > 0.0f) {
    N = f_min(sN / ws + 1.0f, a.max_n);
    const float al = f_max(a.alpha, 1.0f / N), am = f_max(a.alpha_m, 1.0f / N);
    const float kl = 1.0f - al, km = 1.0f - am;
    I = V((sI.x / ws) * kl + Ic.x * al, (sI.y / ws) * kl + Ic.y * al, (sI.z / ws) * kl + Ic.z * al);
    const float y1 = m1, y2 = m2;
    m1 = (sm1 / ws) * km + y1 * am;
    m2 = (sm2 / ws) * km + y2 * am;
  }
  a.img[t] = make_float4(I.x, I.y, I.z, 0.0f);
  a.hist_out[3 * (size_t)t] = make_float4(I.x, I.y, I.z, N);
  a.hist_out[3 * (size_t)t + 1] = make_float4(m1, m2, z, __uint_as_float(1u));
  a.hist_out[3 * (size_t)t + 2] = make_float4(n.x, n.y, n.z, 0.0f);
}

#ifndef HJ_DENOISE_TEMPORAL_NO_KERNELS

// k_dn_variance's text (hj_denoise.h; that kernel and its machine code stay as they are) with the temporal branch: hist is the
// history k_dt_accumulate wrote for this frame.  Grid (ceil(W / 32), ceil(H / 8)).
__global__ __launch_bounds__(kDnTX * kDnTY) void k_dt_variance(float4* __restrict__ guide, const float4* __restrict__ in, float4* __restrict__ out,
                                                              const float4* __restrict__ hist, uint32_t W, uint32_t H) {
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
  guide[3 * (size_t)t + 2] = make_float4(gzx, gzy, 0.0f, 0.0f);
  if (!(hist[3 * (size_t)t].w < (float)HJ_TEMPORAL_VARIANCE_FRAMES)) {
    const float4 h1 = hist[3 * (size_t)t + 1];
    out[t] = make_float4(ci.x, ci.y, ci.z, f_max(h1.y - h1.x * h1.x, 0.0f));
    return;
  }
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
  out[t] = make_float4(ci.x, ci.y, ci.z, f_max(m2 / cnt - mu * mu, 0.0f));
}

// in: the first iteration's (I', V'); a guided pixel's history keeps its N and takes I'
__global__ __launch_bounds__(kDnThreads) void k_dt_feedback(const float4* __restrict__ guide, const float4* __restrict__ in, uint32_t n, float4* __restrict__ hist) {
  const uint32_t t = blockIdx.x * kDnThreads + threadIdx.x;
  if (t >= n) return;
  if (!dn_guided(guide, t)) return;
  const float4 ci = in[t];
  hist[3 * (size_t)t] = make_float4(ci.x, ci.y, ci.z, hist[3 * (size_t)t].w);
}

#endif  // HJ_DENOISE_TEMPORAL_NO_KERNELS

}  // namespace hj
