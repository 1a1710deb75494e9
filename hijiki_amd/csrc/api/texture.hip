// Image textures (no counterpart upstream): the checks and the device buffer behind hj_scene_upload_textured, and the probe
// hj_debug_texture_lookup, which runs the shade stage's own lookup (kernels/hj_texture.h) on the uploaded scene's textures.
#include "hj_internal.h"
#include "../kernels/hj_texture.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

__global__ void k_debug_texture(const float4* __restrict__ tex, uint32_t t, const float* __restrict__ uv, uint32_t n, float* __restrict__ rgb) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const v3 c = texture_rgb(tex, t, uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
  rgb[3 * (size_t)i + 0] = c.x;
  rgb[3 * (size_t)i + 1] = c.y;
  rgb[3 * (size_t)i + 2] = c.z;
}

}  // namespace hj

namespace hjapi {

int validate_textures(hj_context* ctx, const hj_texture_set* t) {
  if (!t) return HJ_OK;
  if ((t->num_textures && !t->textures) || (t->num_texels && !t->texels)) return set_error(ctx, HJ_ERR_INVALID, "textures: null array with non-zero count");
  // device indices are 32-bit and count the records too (kernels/hj_texture.h)
  if (t->num_texels > ((size_t)1 << 32) || t->num_textures + t->num_texels > ((size_t)1 << 32))
    return set_error(ctx, HJ_ERR_UNSUPPORTED, "textures: %zu texels, at most 2^32 are supported", t->num_texels);
  for (size_t i = 0; i < t->num_textures; i++) {
    const hj_texture& x = t->textures[i];
    if (x.width == 0 || x.height == 0) return set_error(ctx, HJ_ERR_INVALID, "texture %zu: %u x %u texels", i, x.width, x.height);
    if (x.filter > HJ_TEX_BILINEAR) return set_error(ctx, HJ_ERR_INVALID, "texture %zu: unknown filter %u", i, x.filter);
    if (x.width > (1u << 24) || x.height > (1u << 24))
      return set_error(ctx, HJ_ERR_UNSUPPORTED, "texture %zu: %u x %u texels, at most 2^24 per axis are supported", i, x.width, x.height);
    if ((uint64_t)x.first_texel + (uint64_t)x.width * x.height > (uint64_t)t->num_texels)
      return set_error(ctx, HJ_ERR_INVALID, "texture %zu: texels %u + %u x %u beyond the %zu of the set", i, x.first_texel, x.width, x.height, t->num_texels);
  }
  return HJ_OK;
}

// One buffer: a record per texture - (width, height, filter, first texel counted from the start of the buffer) - then the texels.
int upload_textures(DevBufs& bufs, const hj_texture_set* t, const float4** out) {
  *out = nullptr;
  if (!t || t->num_textures == 0) return HJ_OK;
  std::vector<float4> rec;
  try { rec.resize(t->num_textures); } catch (const std::bad_alloc&) { return set_error(bufs.ctx, HJ_ERR_NOMEM, "out of host memory"); }
  for (size_t i = 0; i < t->num_textures; i++) {
    const hj_texture& x = t->textures[i];
    rec[i] = make_float4(__builtin_bit_cast(float, x.width), __builtin_bit_cast(float, x.height), __builtin_bit_cast(float, x.filter),
                         __builtin_bit_cast(float, (uint32_t)(t->num_textures + x.first_texel)));
  }
  float4* p = nullptr;
  HJ_TRY(bufs.alloc(p, t->num_textures + t->num_texels));
  HJ_HIP(bufs.ctx, hipMemcpy(p, rec.data(), rec.size() * sizeof(float4), hipMemcpyHostToDevice));
  if (t->num_texels) HJ_HIP(bufs.ctx, hipMemcpy(p + t->num_textures, t->texels, t->num_texels * sizeof(float4), hipMemcpyHostToDevice));
  *out = p;
  return HJ_OK;
}

}  // namespace hjapi

extern "C" {

int hj_debug_texture_lookup(hj_context* ctx, uint32_t texture, const float* uv, size_t n, float* rgb) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "texture lookup before hj_scene_upload");
  if (texture >= ctx->num_textures) return set_error(ctx, HJ_ERR_INVALID, "texture %u of %u", texture, ctx->num_textures);
  if (n == 0) return HJ_OK;
  if (!uv || !rgb) return set_error(ctx, HJ_ERR_INVALID, "null argument");
  if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "too many lookups");
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  DevBufs bufs(ctx);
  float *d_uv = nullptr, *d_rgb = nullptr;
  HJ_TRY(bufs.alloc(d_uv, 2 * n));
  HJ_TRY(bufs.alloc(d_rgb, 3 * n));
  HJ_HIP(ctx, hipMemcpyAsync(d_uv, uv, 2 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  const uint32_t cnt = (uint32_t)n;
  hipLaunchKernelGGL(hj::k_debug_texture, dim3((cnt + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->scene.textures, texture,
                     static_cast<const float*>(d_uv), cnt, d_rgb);
  HJ_HIP(ctx, hipGetLastError());
  HJ_HIP(ctx, hipMemcpyAsync(rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HJ_OK;
}

}  // extern "C"
