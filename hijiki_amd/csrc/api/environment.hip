// Environment lighting (no counterpart upstream): the checks and the sampling distribution behind hj_scene_upload_env, and the
// probes hj_debug_env_lookup / hj_debug_env_sample (the shade stage's own device functions, kernels/hj_env.h) and
// hj_debug_env_distribution (host code only).  DESIGN.md "Environment lighting" defines all of it.
#include "hj_internal.h"
#include "../kernels/hj_env.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

__global__ void k_debug_env_lookup(DeviceScene sc, const float* __restrict__ dirs, uint32_t n, float* __restrict__ rgb) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const v3 c = env_radiance(sc, V(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]));
  rgb[3 * (size_t)i + 0] = c.x;
  rgb[3 * (size_t)i + 1] = c.y;
  rgb[3 * (size_t)i + 2] = c.z;
}

// the draws of sample_emitter<true> after it has picked the environment, with coin = the first draw (env_p = 1)
__global__ void k_debug_env_sample(DeviceScene sc, const uint32_t* __restrict__ states, uint32_t n, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t rng = states[i];
  const float coin = rng_float(rng);
  const uint32_t a = rng_uint(rng), b = rng_uint(rng);
  float pdf;
  uint32_t cell;
  const v3 d = env_sample(sc, coin, a, b, pdf, cell);
  const v3 w = divs(env_radiance(sc, d), pdf);
  float* o = out + 8 * (size_t)i;
  o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = pdf; o[4] = (float)cell; o[5] = w.x; o[6] = w.y; o[7] = w.z;
}

}  // namespace hj

namespace {

constexpr size_t kMaxEnvTexels = (size_t)1 << 28;

// The sampling distribution: a cell per texel, weight = max(r, g, b) of scale * texel (negative: 0) - for a bilinear environment the
// max over the 3 x 3 texels (with the lookup's wrap) whose values a lookup inside the cell can blend - times the cell's solid angle
// (2 pi / W) (sin lat1 - sin lat0).  P = w / sum w; Vose's alias table over N P; every record = (threshold, alias, P / solid angle of
// the cell, of the alias cell).  Double precision throughout, floats at the end.
int build_env_table(const hj_texture_set* t, const hj_environment* env, std::vector<float4>& rec, std::vector<double>& prob,
                    std::vector<double>& omega, double& sum) {
  const hj_texture& x = t->textures[env->texture];
  const uint32_t W = x.width, H = x.height;
  const size_t N = (size_t)W * H;
  const float* tx = t->texels + 4 * (size_t)x.first_texel;
  std::vector<double> m(N), w(N);
  prob.assign(N, 0.0);
  omega.assign(N, 0.0);
  for (size_t i = 0; i < N; i++) {
    double v = 0.0;
    for (int c = 0; c < 3; c++) v = std::max(v, (double)env->scale[c] * (double)tx[4 * i + c]);
    m[i] = v;
  }
  const double kPiD = 3.14159265358979323846;
  sum = 0.0;
  for (uint32_t y = 0; y < H; y++) {
    const double s1 = std::sin(kPiD * (0.5 - (double)y / H)), s0 = std::sin(kPiD * (0.5 - (double)(y + 1) / H));
    const double om = (2.0 * kPiD / W) * (s1 - s0);
    for (uint32_t c = 0; c < W; c++) {
      double v = m[(size_t)y * W + c];
      if (x.filter == HJ_TEX_BILINEAR) {
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) {
            const uint32_t yy = (uint32_t)(((int64_t)y + dy + H) % H), xx = (uint32_t)(((int64_t)c + dx + W) % W);
            v = std::max(v, m[(size_t)yy * W + xx]);
          }
      }
      w[(size_t)y * W + c] = v * om;
      omega[(size_t)y * W + c] = om;
      sum += v * om;
    }
  }
  rec.assign(N, make_float4(0.f, 0.f, 0.f, 0.f));
  if (!(sum > 0.0) || !std::isfinite(sum)) return HJ_OK;
  std::vector<double> q(N);
  std::vector<uint32_t> small, large, alias(N);
  std::vector<double> thr(N, 1.0);
  for (size_t i = 0; i < N; i++) {
    prob[i] = w[i] / sum;
    q[i] = prob[i] * (double)N;
    alias[i] = (uint32_t)i;
    (q[i] < 1.0 ? small : large).push_back((uint32_t)i);
  }
  while (!small.empty() && !large.empty()) {
    const uint32_t s = small.back(), l = large.back();
    small.pop_back();
    large.pop_back();
    thr[s] = q[s];
    alias[s] = l;
    q[l] = (q[l] + q[s]) - 1.0;
    (q[l] < 1.0 ? small : large).push_back(l);
  }
  // (what is left over holds its own column: threshold 1, by rounding only a hair off 1)
  for (size_t i = 0; i < N; i++) {
    const uint32_t a = alias[i];
    rec[i] = make_float4((float)thr[i], __builtin_bit_cast(float, a), (float)(prob[i] / omega[i]), (float)(prob[a] / omega[a]));
  }
  return HJ_OK;
}

}  // namespace

namespace hjapi {

int validate_environment(hj_context* ctx, const hj_scene_desc* s, const hj_texture_set* t, const hj_environment* env, EnvTable& out) {
  out.rec.clear();
  out.weight_sum = 0.0;
  if (!env) return HJ_OK;
  const size_t nt = t ? t->num_textures : 0;
  if (env->texture >= nt) return set_error(ctx, HJ_ERR_INVALID, "environment: texture %u of %zu", env->texture, nt);
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(env->scale[c]) || env->scale[c] < 0.0f)
      return set_error(ctx, HJ_ERR_INVALID, "environment: scale[%d] = %g is not a finite non-negative number", c, (double)env->scale[c]);
  if (!(env->select_prob >= 0.0f && env->select_prob <= 1.0f))
    return set_error(ctx, HJ_ERR_INVALID, "environment: select_prob = %g is outside [0, 1]", (double)env->select_prob);
  if (s && s->num_emitters == 0 && env->select_prob != 1.0f)
    return set_error(ctx, HJ_ERR_INVALID, "environment: the scene has no emitters, so select_prob must be 1 (it is %g)", (double)env->select_prob);
  const hj_texture& x = t->textures[env->texture];
  if ((size_t)x.width * x.height > kMaxEnvTexels)
    return set_error(ctx, HJ_ERR_UNSUPPORTED, "environment: %u x %u texels, at most 2^28 are supported", x.width, x.height);
  const float* tx = t->texels + 4 * (size_t)x.first_texel;
  for (size_t i = 0; i < 4 * (size_t)x.width * x.height; i++)
    if ((i & 3) != 3 && !std::isfinite(tx[i])) return set_error(ctx, HJ_ERR_INVALID, "environment: texel %zu is not finite", i / 4);
  try {
    HJ_TRY(build_env_table(t, env, out.rec, out.prob, out.omega, out.weight_sum));
  } catch (const std::bad_alloc&) {
    return set_error(ctx, HJ_ERR_NOMEM, "environment: out of host memory");
  }
  if (env->select_prob > 0.0f && !(out.weight_sum > 0.0))
    return set_error(ctx, HJ_ERR_INVALID, "environment: select_prob = %g, but every cell of the sampling distribution weighs 0", (double)env->select_prob);
  if (!std::isfinite(out.weight_sum)) return set_error(ctx, HJ_ERR_INVALID, "environment: the cell weights overflow");
  return HJ_OK;
}

int upload_environment(DevBufs& bufs, const hj_texture_set* t, const hj_environment* env, const EnvTable& table, hj::DeviceScene& d) {
  d.env_alias = nullptr;
  if (!env) return HJ_OK;
  HJ_TRY(upload(bufs, table.rec.data(), table.rec.size(), &d.env_alias));
  d.env_tex = env->texture;
  d.env_w = t->textures[env->texture].width;
  d.env_h = t->textures[env->texture].height;
  for (int c = 0; c < 3; c++) d.env_scale[c] = env->scale[c];
  d.env_p = env->select_prob;
  return HJ_OK;
}

}  // namespace hjapi

extern "C" {

int hj_debug_env_lookup(hj_context* ctx, const float* dirs, size_t n, float* rgb) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene || !ctx->scene.env_alias) return set_error(ctx, HJ_ERR_STATE, "environment lookup without an uploaded environment");
  if (n == 0) return HJ_OK;
  if (!dirs || !rgb) return set_error(ctx, HJ_ERR_INVALID, "null argument");
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "too many lookups");
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  DevBufs bufs(ctx);
  float *d_dirs = nullptr, *d_rgb = nullptr;
  HJ_TRY(bufs.alloc(d_dirs, 3 * n));
  HJ_TRY(bufs.alloc(d_rgb, 3 * n));
  HJ_HIP(ctx, hipMemcpyAsync(d_dirs, dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t cnt = (uint32_t)n;
  hipLaunchKernelGGL(hj::k_debug_env_lookup, dim3((cnt + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->scene,
                     static_cast<const float*>(d_dirs), cnt, d_rgb);
  HJ_HIP(ctx, hipGetLastError());
  HJ_HIP(ctx, hipMemcpyAsync(rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HJ_OK;
}

int hj_debug_env_sample(hj_context* ctx, const uint32_t* rng_states, size_t n, float* out) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene || !ctx->scene.env_alias) return set_error(ctx, HJ_ERR_STATE, "environment sample without an uploaded environment");
  if (n == 0) return HJ_OK;
  if (!rng_states || !out) return set_error(ctx, HJ_ERR_INVALID, "null argument");
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "too many samples");
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  DevBufs bufs(ctx);
  uint32_t* d_states = nullptr;
  float* d_out = nullptr;
  HJ_TRY(bufs.alloc(d_states, n));
  HJ_TRY(bufs.alloc(d_out, 8 * n));
  HJ_HIP(ctx, hipMemcpyAsync(d_states, rng_states, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t cnt = (uint32_t)n;
  hipLaunchKernelGGL(hj::k_debug_env_sample, dim3((cnt + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->scene,
                     static_cast<const uint32_t*>(d_states), cnt, d_out);
  HJ_HIP(ctx, hipGetLastError());
  HJ_HIP(ctx, hipMemcpyAsync(out, d_out, 8 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HJ_OK;
}

int hj_debug_env_distribution(const hj_texture_set* textures, const hj_environment* env, float* prob, float* pdf, float* alias_prob,
                              uint32_t* alias, double* weight_sum) {
  if (!textures || !env) return set_error(nullptr, HJ_ERR_INVALID, "null argument");
  HJ_TRY(validate_textures(nullptr, textures));
  if (!(env->select_prob >= 0.0f && env->select_prob <= 1.0f))
    return set_error(nullptr, HJ_ERR_INVALID, "environment: select_prob = %g is outside [0, 1]", (double)env->select_prob);
  // (select_prob 0: no check against the weights, so that a black environment is described too; no scene: no emitter check)
  hj_environment e = *env;
  e.select_prob = 0.0f;
  EnvTable table;
  HJ_TRY(validate_environment(nullptr, nullptr, textures, &e, table));
  for (size_t i = 0; i < table.rec.size(); i++) {
    if (prob) prob[i] = (float)table.prob[i];
    if (pdf) pdf[i] = table.rec[i].z;
    if (alias_prob) alias_prob[i] = table.rec[i].x;
    if (alias) alias[i] = __builtin_bit_cast(uint32_t, table.rec[i].y);
  }
  if (weight_sum) *weight_sum = table.weight_sum;
  return HJ_OK;
}

}  // extern "C"
