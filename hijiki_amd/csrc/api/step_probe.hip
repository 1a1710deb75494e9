// Probes below the frame level (DESIGN.md "Primitive level", "Step level").  hj_debug_num: the functions of kernels/hj_num.h
// themselves - the device text of numeric contract HJ-NUM-1 - on caller-given inputs, one thread per record.  hj_debug_shade_step:
// host code only - it fabricates a batch of path states and raw hits, has api/render.hip launch the shade stage's own kernel over it
// once (launch_shade) and reads back what the stage wrote.  Nothing here restates their arithmetic; this unit includes hj_num.h
// only (the other kernel headers define __global__ functions that render.hip owns), so the path kernels' machine code does not
// depend on it.
#include "hj_internal.h"
#include "../kernels/hj_num.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {
namespace {

HJ_DEV float word_f(uint32_t w) { return __uint_as_float(w); }
HJ_DEV uint32_t f_word(float f) { return __float_as_uint(f); }
HJ_DEV void put3(uint32_t* o, v3 a) { o[0] = f_word(a.x); o[1] = f_word(a.y); o[2] = f_word(a.z); }

}  // namespace

// in: HJ_NUM_IN_WORDS words per record, out: HJ_NUM_OUT_WORDS (include/hijiki_hip.h lists what every op reads and writes)
__global__ void k_debug_num(uint32_t op, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = in + HJ_NUM_IN_WORDS * (size_t)i;
  uint32_t o[HJ_NUM_OUT_WORDS] = {0u, 0u, 0u, 0u};
  const float a = word_f(w[0]), b = word_f(w[1]);
  const v3 p = V(word_f(w[0]), word_f(w[1]), word_f(w[2])), q = V(word_f(w[3]), word_f(w[4]), word_f(w[5]));
  uint32_t s = w[0];
  switch (op) {
    case HJ_NUM_EXP: o[0] = f_word(hj_exp(a)); break;
    case HJ_NUM_SINCOS2PI: { float sn, cs; hj_sincos2pi(a, sn, cs); o[0] = f_word(sn); o[1] = f_word(cs); break; }
    case HJ_NUM_ATAN2: o[0] = f_word(hj_atan2(a, b)); break;
    case HJ_NUM_ASIN: o[0] = f_word(hj_asin(a)); break;
    case HJ_NUM_MIN: o[0] = f_word(f_min(a, b)); break;
    case HJ_NUM_MAX: o[0] = f_word(f_max(a, b)); break;
    case HJ_NUM_DIV: o[0] = f_word(a / b); break;
    case HJ_NUM_SQRT: o[0] = f_word(__builtin_sqrtf(a)); break;
    case HJ_NUM_DOT3: o[0] = f_word(dot3(p, q)); break;
    case HJ_NUM_CROSS3: put3(o, cross3(p, q)); break;
    case HJ_NUM_NORMALIZE3: put3(o, normalize3(p)); break;
    case HJ_NUM_REFLECT3: put3(o, reflect3(p, q)); break;
    case HJ_NUM_RNG_SEED: o[0] = rng_seed(s); break;
    case HJ_NUM_RNG_UINT: o[0] = rng_uint(s); o[1] = s; break;
    case HJ_NUM_RNG_FLOAT: o[0] = f_word(rng_float(s)); o[1] = s; break;
    case HJ_NUM_RAND_COS_HEMISPHERE: put3(o, rand_cos_hemisphere(s)); o[3] = s; break;
    case HJ_NUM_RAND_UNIFORM_SPHERE: put3(o, rand_uniform_sphere(s)); o[3] = s; break;
    case HJ_NUM_RAND_BARYCENTRIC: put3(o, rand_barycentric(s)); o[3] = s; break;
    default: break;
  }
  uint32_t* dst = out + HJ_NUM_OUT_WORDS * (size_t)i;
  for (int k = 0; k < HJ_NUM_OUT_WORDS; k++) dst[k] = o[k];
}

}  // namespace hj

extern "C" {

int hj_debug_num(hj_context* ctx, uint32_t op, const uint32_t* in, size_t n, uint32_t* out) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (op >= HJ_NUM_OPS) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_num: op %u of %u", op, (unsigned)HJ_NUM_OPS);
  if (!in || !out) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_num: null argument");
  if (n == 0) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_num: no records");
  if (n > HJ_NUM_MAX_RECORDS) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_num: %zu records, at most %u a call", n, (unsigned)HJ_NUM_MAX_RECORDS);
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  DevBufs bufs(ctx);
  uint32_t *d_in = nullptr, *d_out = nullptr;
  HJ_TRY(bufs.alloc(d_in, HJ_NUM_IN_WORDS * n));
  HJ_TRY(bufs.alloc(d_out, HJ_NUM_OUT_WORDS * n));
  HJ_HIP(ctx, hipMemcpyAsync(d_in, in, HJ_NUM_IN_WORDS * n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t cnt = (uint32_t)n;
  hipLaunchKernelGGL(hj::k_debug_num, dim3((cnt + 255u) / 256u), dim3(256), 0, ctx->stream, op, static_cast<const uint32_t*>(d_in), cnt,
                     d_out);
  HJ_HIP(ctx, hipGetLastError());
  HJ_HIP(ctx, hipMemcpyAsync(out, d_out, HJ_NUM_OUT_WORDS * n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HJ_OK;
}


// The batch the shade stage reads, fabricated on the host: record i is sample i and sits at the next position of the segment of
// workgroup i % num_wg in the arrays of `parity`; the positions are binned into q_hit in queue order as the hit compaction leaves
// them (kernels/hj_stages.h compact_hits_by_tag: a tag's own bin, textured hits in the checkerboard's, misses behind the material
// bins when the scene has an environment).  The stage then runs exactly as in a split-path round, and its appends are matched back
// to their records by the sample index they carry.
int hj_debug_shade_step(hj_context* ctx, const hj_render_opts* opts, const uint32_t* in, size_t n, uint32_t num_wg, uint32_t parity,
                        uint32_t* out, uint32_t* counters) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "hj_debug_shade_step: no scene uploaded");
  if (!opts || !in || !out || !counters) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: null argument");
  if (n == 0) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: no records");
  if (n > HJ_STEP_MAX_RECORDS) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: %zu records, at most %u a call", n, (unsigned)HJ_STEP_MAX_RECORDS);
  if (num_wg == 0 || num_wg > n) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: %u workgroups for %zu records", num_wg, n);
  if (parity > 1u) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: parity %u", parity);
  const hj::DeviceScene sc = scene_for(ctx, *opts);
  const uint32_t shapes = sc.ns + sc.nq + sc.nt;
  const uint32_t cnt = (uint32_t)n;
  for (uint32_t i = 0; i < cnt; i++) {
    const int32_t id = (int32_t)in[(size_t)i * HJ_STEP_IN_WORDS + 7];
    if (id >= 0 && (uint32_t)id >= shapes) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: record %u hits shape %d of %u", i, id, shapes);
  }
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> materials(shapes);
  if (shapes) HJ_HIP(ctx, hipMemcpy(materials.data(), sc.materials, sizeof(uint32_t) * shapes, hipMemcpyDeviceToHost));

  const bool env = sc.env_alias != nullptr, has_ext = sc.has_extinction != 0;
  const uint32_t G = num_wg, bins = hit_bins(env), miss_bin = hj::kNumTags;
  const uint32_t pool = ((cnt + G - 1u) / G + 63u) / 64u * 64u;
  const size_t P = (size_t)G * pool;
  const uint32_t np = parity ^ 1u;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  std::vector<float4> h_o(P, zero4), h_d(P, zero4), h_t(P, zero4), h_e(P, zero4), h_hit(P, zero4);
  std::vector<uint32_t> h_q((size_t)bins * P, 0u), h_cnt((size_t)G * bins, 0u);
  auto f = [](uint32_t w) { float x; std::memcpy(&x, &w, 4); return x; };
  auto u = [](float x) { uint32_t w; std::memcpy(&w, &x, 4); return w; };
  for (uint32_t i = 0; i < cnt; i++) {
    const uint32_t* w = in + (size_t)i * HJ_STEP_IN_WORDS;
    const uint32_t g = i % G, qpos = i / G;
    const size_t pos = (size_t)g * pool + qpos;
    h_o[pos] = make_float4(f(w[0]), f(w[1]), f(w[2]), f(i));
    h_d[pos] = make_float4(f(w[3]), f(w[4]), f(w[5]), f(w[16]));
    h_hit[pos] = make_float4(f(w[6]), f(w[7]), f(w[8]), f(w[9]));
    h_t[pos] = make_float4(f(w[10]), f(w[11]), f(w[12]), f(w[17]));
    h_e[pos] = make_float4(f(w[13]), f(w[14]), f(w[15]), 0.f);
    const int32_t id = (int32_t)w[7];
    uint32_t bin;
    if (id < 0) {
      if (!env) continue;                                  // (the path is over: nothing refers to it again)
      bin = miss_bin;
    } else {
      const uint32_t tag = materials[id] >> HJ_MATERIAL_TAG_SHIFT;
      bin = tag == HJ_MAT_DIFFUSE_TEXTURED && hj::kNumTags == 5 ? (uint32_t)HJ_MAT_DIFFUSECBOARD : tag;
      if (bin >= hj::kNumTags) return set_error(ctx, HJ_ERR_INVALID, "hj_debug_shade_step: shape %d has material tag %u", id, tag);
    }
    uint32_t& c = h_cnt[(size_t)g * bins + bin];
    h_q[((size_t)bin * G + g) * pool + c] = qpos;
    c++;
  }

  PathState ps;                                            // (freed on return)
  HJ_TRY(ensure_path_state(ctx, ps, cnt, G, G, pool, /*extinction=*/true, env));   // ext[] whatever the scene: set and read back below
  const hj::BatchState& st = ps.st;
  hipStream_t s = ctx->stream;
  const size_t f4 = sizeof(float4), w4 = sizeof(uint32_t);
  HJ_HIP(ctx, hipMemsetAsync(st.smp_rgb, 0, f4 * cnt, s));
  HJ_HIP(ctx, hipMemsetAsync(st.smp_nd, 0, f4 * cnt, s));
  for (float4* a : {st.ray_o[np], st.ray_d[np], st.thr[np], st.ext[np], st.sh_o, st.sh_d, st.sh_c}) HJ_HIP(ctx, hipMemsetAsync(a, 0, f4 * P, s));
  for (uint32_t* a : {st.cnt_ray[0], st.cnt_ray[1], st.cnt_shadow}) HJ_HIP(ctx, hipMemsetAsync(a, 0, w4 * G, s));
  HJ_HIP(ctx, hipMemsetAsync(st.acc_closest, 0, w4 * kStatWords * G, s));   // acc_closest .. acc_direct: one allocation
  HJ_HIP(ctx, hipMemcpyAsync(st.ray_o[parity], h_o.data(), f4 * P, hipMemcpyHostToDevice, s));
  HJ_HIP(ctx, hipMemcpyAsync(st.ray_d[parity], h_d.data(), f4 * P, hipMemcpyHostToDevice, s));
  HJ_HIP(ctx, hipMemcpyAsync(st.thr[parity], h_t.data(), f4 * P, hipMemcpyHostToDevice, s));
  HJ_HIP(ctx, hipMemcpyAsync(st.ext[parity], h_e.data(), f4 * P, hipMemcpyHostToDevice, s));
  HJ_HIP(ctx, hipMemcpyAsync(st.hit, h_hit.data(), f4 * P, hipMemcpyHostToDevice, s));
  HJ_HIP(ctx, hipMemcpyAsync(st.q_hit, h_q.data(), w4 * h_q.size(), hipMemcpyHostToDevice, s));
  HJ_HIP(ctx, hipMemcpyAsync(st.cnt_hit, h_cnt.data(), w4 * h_cnt.size(), hipMemcpyHostToDevice, s));
  launch_shade(st, sc, parity, *opts, s);
  HJ_HIP(ctx, hipGetLastError());

  std::vector<float4> r_o(P), r_d(P), r_t(P), r_e(P), r_so(P), r_sd(P), r_sc(P), r_rgb(cnt), r_nd(cnt);
  std::vector<uint32_t> c_ray(G), c_sh(G), c_dir(G);
  HJ_HIP(ctx, hipMemcpyAsync(r_o.data(), st.ray_o[np], f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_d.data(), st.ray_d[np], f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_t.data(), st.thr[np], f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_e.data(), st.ext[np], f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_so.data(), st.sh_o, f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_sd.data(), st.sh_d, f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_sc.data(), st.sh_c, f4 * P, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_rgb.data(), st.smp_rgb, f4 * cnt, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(r_nd.data(), st.smp_nd, f4 * cnt, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(c_ray.data(), st.cnt_ray[np], w4 * G, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(c_sh.data(), st.cnt_shadow, w4 * G, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipMemcpyAsync(c_dir.data(), st.acc_direct, w4 * G, hipMemcpyDeviceToHost, s));
  HJ_HIP(ctx, hipStreamSynchronize(s));

  std::memset(out, 0, sizeof(uint32_t) * HJ_STEP_OUT_WORDS * n);
  for (uint32_t g = 0; g < G; g++) {
    counters[3 * g] = c_ray[g]; counters[3 * g + 1] = c_sh[g]; counters[3 * g + 2] = c_dir[g];
    if (c_ray[g] > pool || c_sh[g] > pool) return set_error(ctx, HJ_ERR_DEVICE, "hj_debug_shade_step: workgroup %u appended %u rays, %u shadow rays to %u positions", g, c_ray[g], c_sh[g], pool);
    for (uint32_t k = 0; k < c_ray[g]; k++) {
      const size_t pos = (size_t)g * pool + k;
      const uint32_t smp = u(r_o[pos].w) & ~hj::kCameraFlag;
      if (smp >= cnt) return set_error(ctx, HJ_ERR_DEVICE, "hj_debug_shade_step: a continuing path carries sample %u of %u", smp, cnt);
      uint32_t* o = out + (size_t)smp * HJ_STEP_OUT_WORDS;
      o[0] += 1u;                                          // (2: the stage wrote this sample's record twice)
      o[1] = u(r_o[pos].x); o[2] = u(r_o[pos].y); o[3] = u(r_o[pos].z);
      o[4] = u(r_d[pos].x); o[5] = u(r_d[pos].y); o[6] = u(r_d[pos].z);
      o[7] = u(r_t[pos].x); o[8] = u(r_t[pos].y); o[9] = u(r_t[pos].z);
      o[10] = u(r_t[pos].w);
      o[11] = u(r_d[pos].w);
      if (has_ext) { o[12] = u(r_e[pos].x); o[13] = u(r_e[pos].y); o[14] = u(r_e[pos].z); }
    }
    for (uint32_t k = 0; k < c_sh[g]; k++) {
      const size_t pos = (size_t)g * pool + k;
      const uint32_t smp = u(r_sc[pos].w);
      if (smp >= cnt) return set_error(ctx, HJ_ERR_DEVICE, "hj_debug_shade_step: a shadow record carries sample %u of %u", smp, cnt);
      uint32_t* o = out + (size_t)smp * HJ_STEP_OUT_WORDS;
      o[15] += 1u;
      o[16] = u(r_so[pos].x); o[17] = u(r_so[pos].y); o[18] = u(r_so[pos].z);
      o[19] = u(r_sd[pos].x); o[20] = u(r_sd[pos].y); o[21] = u(r_sd[pos].z);
      o[22] = u(r_sd[pos].w);
      o[23] = u(r_sc[pos].x); o[24] = u(r_sc[pos].y); o[25] = u(r_sc[pos].z);
    }
  }
  for (uint32_t i = 0; i < cnt; i++) {
    uint32_t* o = out + (size_t)i * HJ_STEP_OUT_WORDS;
    o[26] = u(r_rgb[i].x); o[27] = u(r_rgb[i].y); o[28] = u(r_rgb[i].z);
    o[29] = u(r_nd[i].x); o[30] = u(r_nd[i].y); o[31] = u(r_nd[i].z); o[32] = u(r_nd[i].w);
  }
  return HJ_OK;
}

}  // extern "C"
