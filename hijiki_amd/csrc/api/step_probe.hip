// Probes below the frame level (DESIGN.md "Primitive level").  hj_debug_num: the functions of kernels/hj_num.h themselves - the
// device text of numeric contract HJ-NUM-1 - on caller-given inputs, one thread per record.  Nothing here restates their
// arithmetic; this unit includes hj_num.h only (the other kernel headers define __global__ functions that render.hip owns), so the
// path kernels' machine code does not depend on it.
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

}  // extern "C"
