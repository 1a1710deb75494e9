// Frame AOVs and material queries ("Frame AOVs and material queries"; include/hijiki_hip.h hj_eval_materials,
// hj_render_aovs): what colour a surface has at (u, v), and a frame's albedo / normal / depth from the frame's own primary rays.
// The functions a hit needs are the shade stage's - camera_ray (hj_stages.h), populate_*, checkerboard (hj_shade.h), texture_rgb
// (hj_texture.h), walk_segment (hj_walk_segment.h) - included here and edited nowhere: this header adds the tag dispatch of a material
// that LEAVES the kernel (eval_material: stage_shade's own dispatch multiplies the colour into the path throughput) and the
// kernels around it.  No global atomics, no inline assembly of its own.
//   k_mat_eval            one lane per (hit, surface) record pair of hj_trace_rays
//   k_aov_walk<PAIRS>     the persistent walk with a fetch that builds the camera ray from the sample index: no ray array exists
//   k_aov_resolve         one lane per sample slot of a run of blocks: the sample's 12-word record added to its pixel
#pragma once
#include "hj_walk_segment.h"

#pragma clang fp contract(off)

namespace hj {

constexpr uint32_t kMatMiss = 0xFFFFFFFFu;   // word 3 of a material record for an id outside [0, shapes)

// The material of shape `id` (< ns + nq + nt) at texture coordinates (u, v): albedo, emitted radiance, the uploaded word.
//   diffuse: its colour; checkerboard: checkerboard(index, u, v); textured: texture_rgb(textures, index, u, v)
//   mirror, dielectric: albedo 1 (what a discrete bounce multiplies the throughput by, before extinction)
//   emissive: albedo 0, emission = its power (what render.glsl:114-116 adds for a discrete hit at throughput 1)
HJ_DEV void eval_material(const DeviceScene& sc, uint32_t id, float u, float v, v3& albedo, v3& emission, uint32_t& word) {
  const uint32_t mat = sc.materials[id];
  const uint32_t midx = mat & HJ_MATERIAL_INDEX_MASK;
  word = mat;
  albedo = V(0.f, 0.f, 0.f);
  emission = V(0.f, 0.f, 0.f);
  switch (mat >> HJ_MATERIAL_TAG_SHIFT) {
    case HJ_MAT_DIFFUSE: albedo = xyz(sc.diffuse[midx]); break;
    case HJ_MAT_DIFFUSECBOARD: albedo = checkerboard(sc, midx, u, v); break;
    case HJ_MAT_DIFFUSE_TEXTURED: albedo = texture_rgb(sc.textures, midx, u, v); break;
    case HJ_MAT_MIRROR:
    case HJ_MAT_DIELECTRIC: albedo = V(1.f, 1.f, 1.f); break;
    case HJ_MAT_EMISSIVE: emission = xyz(sc.emissive[midx]); break;
    default: break;                          // (hj_scene_upload refuses every other tag)
  }
}

#ifndef HJ_AOV_NO_KERNELS   // (kernels/hj_follow.h takes the functions and brings kernels of its own)
// hits: hj_trace_rays' records (objectID bits, t, u, v); surface: its four float4 per ray (u, v = words 6, 7).  out: two float4
// per record = albedo.rgb, material word bits | emission.rgb, 0.  The word comes from the scene by id, never from the surface
// record: a miss's all-zero record would read as "diffuse, index 0".
__global__ __launch_bounds__(kBlockThreads) void k_mat_eval(DeviceScene sc, const float4* __restrict__ hits, const float4* __restrict__ surface,
                                                            uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = __float_as_uint(hits[i].x);
  float4 o0 = make_float4(0.f, 0.f, 0.f, __uint_as_float(kMatMiss)), o1 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (id < sc.ns + sc.nq + sc.nt) {                                // (a miss is 0xFFFFFFFF; any other id outside the scene is one too)
    const float4 s1 = surface[4 * (size_t)i + 1];
    v3 albedo, emission;
    uint32_t word;
    eval_material(sc, id, s1.z, s1.w, albedo, emission, word);
    o0 = make_float4(albedo.x, albedo.y, albedo.z, __uint_as_float(word));
    o1 = make_float4(emission.x, emission.y, emission.z, 0.f);
  }
  out[2 * (size_t)i] = o0;
  out[2 * (size_t)i + 1] = o1;
}

#endif  // HJ_AOV_NO_KERNELS

// The blocks of a launch as camera_ray reads them: it touches blocks and num_blocks of the batch (and the scene's camera), and
// group_sample the scene's group_tile, nothing else.
HJ_DEV BatchState aov_batch(const hj_image_block* blocks, uint32_t num_blocks) {
  BatchState st{};
  st.blocks = blocks;
  st.num_blocks = num_blocks;
  return st;
}

#ifndef HJ_AOV_NO_KERNELS
// Sample slots [0, n = num_blocks * kSlotsPerBlock) of the launch's blocks.  Workgroup g walks queue entries [g * wg_rays, ...)
// (walk_segment); entry i is lane i & 63 of 64-sample group i >> 6 (group_sample: a block row's 64 pixels, or an 8 x 8 tile over
// a large tree - the grouping the camera packets use, a bijection of the slots either way), and its hit record (objectID bits, t,
// u, v; a miss: (-1, 0, 0, 0)) goes to hits[slot]: which lane or workgroup carried a sample shows in no result.  A slot without a
// sample (outside its block's dimension or the image: camera_ray says so) is fetched as a ray with the empty range [+inf, -inf]:
// it fails every box and shape test and leaves the tree at the first node; k_aov_resolve never reads its record.
template <bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_aov_walk(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                            uint32_t wg_rays, float4* __restrict__ hits) {
  const BatchState st = aov_batch(blocks, num_blocks);
  auto fetch = [&](uint32_t q, uint32_t& slot, Ray& r, bool& any, RawHit& h) {
    const uint32_t smp = group_sample(q >> 6, q & 63u, sc.group_tile);
    slot = smp;
    any = false;
    uint32_t rng_unused = 0;
    r.o = V(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]);
    r.d = V(0.f, 0.f, 0.f);
    walk_empty_range(r, camera_ray(st, sc, smp, rng_unused, r.d));
    walk_reset(h);
  };
  auto finish = [&](bool done, uint32_t slot, const RawHit& h, bool) {
    if (done) hits[slot] = walk_hit_record(h);
  };
  walk_segment<0, PAIRS>(sc, num_blocks * kSlotsPerBlock, wg_rays, fetch, finish);
}

#endif  // HJ_AOV_NO_KERNELS

// The 12-word record of a sample whose ray (o, d) ended in hit record hr (objectID bits, t, u, v): the hit populated as the shade
// stage populates it (hit point fma(t, d, o), scene.glsl:164), the material evaluated by eval_material -> albedo.rgb, 1 | n.xyz, t |
// emission.rgb, 1; a miss (an id outside the scene): 0, 0, 0, 1 and eight zeros.  ONE text for k_aov_resolve and the followed
// resolve of kernels/hj_follow.h.  -> a hit
HJ_DEV bool aov_record(const DeviceScene& sc, v3 o, v3 d, float4 hr, float4& r0, float4& r1, float4& r2) {
  const uint32_t id = __float_as_uint(hr.x);
  r0 = make_float4(0.f, 0.f, 0.f, 1.f);
  r1 = make_float4(0.f, 0.f, 0.f, 0.f);
  r2 = r1;
  if (id >= sc.ns + sc.nq + sc.nt) return false;
  Its its;
  its.p = V(fmaf(hr.y, d.x, o.x), fmaf(hr.y, d.y, o.y), fmaf(hr.y, d.z, o.z));
  if (id < sc.ns) populate_sphere(sc.spheres[id], its);
  else if (id < sc.ns + sc.nq) populate_quad(sc, id - sc.ns, hr.z, hr.w, its);
  else populate_triangle(sc, id - sc.ns - sc.nq, hr.z, hr.w, its);
  v3 albedo, emission;
  uint32_t word;
  eval_material(sc, id, its.u, its.v, albedo, emission, word);
  r0 = make_float4(albedo.x, albedo.y, albedo.z, 1.f);
  r1 = make_float4(its.n.x, its.n.y, its.n.z, hr.y);
  r2 = make_float4(emission.x, emission.y, emission.z, 1.f);
  return true;
}

// The pixel (origin + l) of sample slot smp, a sample camera_ray has accepted -> false outside width x height (no wrap-around)
HJ_DEV bool aov_pixel(const hj_image_block* __restrict__ blocks, uint32_t smp, uint32_t width, uint32_t height, uint32_t& px, uint32_t& py) {
  const hj_image_block b = blocks[smp / kSlotsPerBlock];
  const uint32_t lx = smp & (HJ_BLOCK_SIZE - 1u), ly = (smp / HJ_BLOCK_SIZE) & (HJ_BLOCK_SIZE - 1u);
  if (b.origin[0] >= width || lx >= width - b.origin[0] || b.origin[1] >= height || ly >= height - b.origin[1]) return false;
  px = b.origin[0] + lx;
  py = b.origin[1] + ly;
  return true;
}

// The record added to pixel p's three float4: a read-add-write, which races with nothing inside a run
HJ_DEV void aov_add(float4* __restrict__ p, float4 r0, float4 r1, float4 r2) {
  float4 a0 = p[0], a1 = p[1], a2 = p[2];
  a0.x += r0.x; a0.y += r0.y; a0.z += r0.z; a0.w += r0.w;
  a1.x += r1.x; a1.y += r1.y; a1.z += r1.z; a1.w += r1.w;
  a2.x += r2.x; a2.y += r2.y; a2.z += r2.z; a2.w += r2.w;
  p[0] = a0; p[1] = a1; p[2] = a2;
}

#ifndef HJ_AOV_NO_KERNELS
// A RUN: blocks [b0, b0 + nb) of the launch's block list, whose pixel rectangles are pairwise disjoint (the host cuts the list so),
// so every pixel gets at most one sample of this launch and the read-add-write below races with nothing.  One lane per sample slot:
// the ray is rebuilt (camera_ray) and the record (aov_record: albedo.rgb, 1 | n.xyz, t | emission.rgb, hit ? 1 : 0; a miss: 0, 0, 0,
// 1 and eight zeros) added to pixel (origin + l) of aov, 12 floats a pixel.  A pixel outside width x height is not written.
__global__ __launch_bounds__(kBlockThreads) void k_aov_resolve(DeviceScene sc, const hj_image_block* __restrict__ blocks, uint32_t num_blocks,
                                                               uint32_t b0, uint32_t nb, const float4* __restrict__ hits, uint32_t width,
                                                               uint32_t height, float4* __restrict__ aov) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nb * kSlotsPerBlock) return;
  const uint32_t smp = b0 * kSlotsPerBlock + j;
  const BatchState st = aov_batch(blocks, num_blocks);
  uint32_t rng_unused = 0;
  v3 d = V(0.f, 0.f, 0.f);
  if (!camera_ray(st, sc, smp, rng_unused, d)) return;
  uint32_t px, py;
  if (!aov_pixel(blocks, smp, width, height, px, py)) return;
  float4 r0, r1, r2;
  (void)aov_record(sc, V(sc.camera.position[0], sc.camera.position[1], sc.camera.position[2]), d, hits[smp], r0, r1, r2);
  aov_add(aov + 3 * ((size_t)py * width + px), r0, r1, r2);
}

#endif  // HJ_AOV_NO_KERNELS

}  // namespace hj
