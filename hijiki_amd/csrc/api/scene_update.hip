// hj_scene_update_shapes: the uploaded scene's shapes moved IN PLACE.  The re-laid-out tree is a function of the links and of one
// box per node, so an update recomputes the boxes (the refit's bottom-up pass, api/refit_pass.hpp) and writes them where the upload
// put each node (hj_context::SceneUpdate::node_map); every link, the collapse, pair and hot sets and the record positions stay.
//
//   k_su_links        (first update) the uploaded topology's links, read back from the second copy of the tree on the device
//   k_su_check        every coordinate and radius finite, every emitter's shape emissive: the verdict, before any live buffer is written
//   k_rf_tiled / k_rf_climb   skip-link records with the new boxes into a scratch buffer kept with the scene
//   ---- one stream synchronisation: the verdict ----
//   k_su_scatter      one thread per uploaded node: its box into its re-laid-out record, into record root2 + i, and - a guarded leaf -
//                     the guard's box (scene_upload.hip's formula, operation for operation; the parent's box where the parent was
//                     collapsed and no longer contains the padded one); box words only
//   k_su_triangles, k_su_pairs, k_su_emitters     tri_isect / tri_shade, tri_pair, emit_rec gathered again
#include "hj_internal.h"
#include "guard_box.hpp"
#include "refit_pass.hpp"
#include "scene_relayout.hpp"

#pragma clang fp contract(off)

using namespace hjapi;

namespace {

constexpr uint32_t kNoRecord = hj_context::SceneUpdate::kNoRecord;
enum : uint32_t { kSuNonFinite = 1u, kSuEmitterNotEmissive = 2u, kSuEmitterRange = 4u };

// (shape_index, exit_index) of node i of the uploaded array from record root2 + i (scene_upload.hip "The second copy of the tree":
// A = the shape of a leaf, B = root2 + exit, or kEndOfWalk on the right spine - any index >= n0 serves there)
__global__ __launch_bounds__(256) void k_su_links(const float4* __restrict__ nodes, uint32_t root2, uint32_t n0, uint2* __restrict__ links) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  const uint32_t a = __float_as_uint(nodes[2 * ((size_t)root2 + i)].w), b = __float_as_uint(nodes[2 * ((size_t)root2 + i) + 1].w);
  links[i] = make_uint2((a & hj::kInnerFlag) ? HJ_BVH_INNER : a, b == hj::kEndOfWalk ? n0 : b - root2);
}

// one thread per sphere, quad part, vertex and emitter
__global__ __launch_bounds__(256) void k_su_check(RefitShapes s, uint32_t nv, const hj_emitter* __restrict__ emitters, uint32_t ne,
                                                  const uint32_t* __restrict__ materials, uint32_t* __restrict__ verdict) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = true;
  if (i < s.ns) {
    const float4 v = s.spheres[i];
    ok = su_finite(v.x) && su_finite(v.y) && su_finite(v.z) && su_finite(v.w);
  } else if ((i -= s.ns) < 3u * s.nq) {
    const float4 v = s.quads[i];
    ok = su_finite(v.x) && su_finite(v.y) && su_finite(v.z);
  } else if ((i -= 3u * s.nq) < nv) {
    const hj_vertex v = s.vertices[i];
    ok = su_finite(v.pos[0]) && su_finite(v.pos[1]) && su_finite(v.pos[2]);
  } else if ((i -= nv) < ne) {
    const uint32_t sh = emitters[i].shape;
    if (sh >= s.ns + s.nq + s.nt) atomicOr(verdict, (uint32_t)kSuEmitterRange);
    else if ((materials[sh] >> HJ_MATERIAL_TAG_SHIFT) != HJ_MAT_EMISSIVE) atomicOr(verdict, (uint32_t)kSuEmitterNotEmissive);
  }
  if (!ok) atomicOr(verdict, (uint32_t)kSuNonFinite);
}

// box words of record `at` replaced, link words kept: two 16-byte loads, two 16-byte stores
__device__ inline void su_put_box(float4* __restrict__ nodes, uint32_t at, const float lo[3], const float hi[3]) {
  float4* rec = nodes + 2 * (size_t)at;
  const float a = rec[0].w, b = rec[1].w;
  rec[0] = make_float4(lo[0], lo[1], lo[2], a);
  rec[1] = make_float4(hi[0], hi[1], hi[2], b);
}

// One thread per node of the uploaded array.  fresh: the refitted skip-link records; where: hj_context::SceneUpdate::node_map;
// parent: the link set's (the root's is never read: a leaf is not the root of a tree of two or more shapes).
__global__ __launch_bounds__(256) void k_su_scatter(const float4* __restrict__ fresh, const uint2* __restrict__ where,
                                                    const uint32_t* __restrict__ parent, uint32_t n0, uint32_t root2, RefitShapes s, float cam_x, float cam_y, float cam_z, float4* __restrict__ nodes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n0) return;
  const float4 l4 = fresh[2 * (size_t)i], h4 = fresh[2 * (size_t)i + 1];
  const float lo[3] = {l4.x, l4.y, l4.z}, hi[3] = {h4.x, h4.y, h4.z};
  const uint2 w = where[i];
  su_put_box(nodes, root2 + i, lo, hi);
  if (w.x != kNoRecord) su_put_box(nodes, w.x, lo, hi);
  if (w.y != kNoRecord) {
    // the absolute part of the padding: 2e-4, or 4e-6 of the extent of the new root box joined with the camera
    const float4 r0 = fresh[0], r1 = fresh[1];
    const float rlo[3] = {r0.x, r0.y, r0.z}, rhi[3] = {r1.x, r1.y, r1.z}, cam[3] = {cam_x, cam_y, cam_z};
    float pad_abs = 2e-4f, ext = 0.f;
    for (int k = 0; k < 3; k++) {
      const float a = su_min(rlo[k], cam[k]), b = su_max(rhi[k], cam[k]);
      if (b - a == b - a) ext = su_max(ext, b - a);
    }
    if (su_finite(ext)) pad_abs = su_max(pad_abs, 4e-6f * ext);
    float gmin[3], gmax[3];
    su_guard_box(s, __float_as_uint(l4.w), pad_abs, gmin, gmax);
    // The upload collapsed this leaf's parent P only because the guard's box lay inside P's (scene_upload.hip "Collapse": "child
    // passes => P passes" needs containment).  P's refitted box is tight around the moved leaves and the padded box may stick out
    // of it now: a ray could pass the guard where the reference fails P and never tests the shape.  Then the guard takes P's box -
    // its test is the reference's own test of P, bit for bit, and the sibling's box lies inside P's by the refit.
    const uint32_t p = parent[i];
    if (p < n0 && where[p].x == kNoRecord) {
      const float4 p0 = fresh[2 * (size_t)p], p1 = fresh[2 * (size_t)p + 1];
      const float plo[3] = {p0.x, p0.y, p0.z}, phi[3] = {p1.x, p1.y, p1.z};
      bool in = true;
      for (int k = 0; k < 3; k++) in = in && gmin[k] >= plo[k] && gmax[k] <= phi[k];
      if (!in) for (int k = 0; k < 3; k++) { gmin[k] = plo[k]; gmax[k] = phi[k]; }
    }
    su_put_box(nodes, w.y, gmin, gmax);
  }
}

__global__ __launch_bounds__(256) void k_su_triangles(const hj_triangle* __restrict__ tris, const hj_vertex* __restrict__ verts, uint32_t nt,
                                                      float4* __restrict__ isect, float4* __restrict__ shade) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nt) tri_records(tris, verts, i, isect, shade);
}

// the two triangles of pair p again, from the new tri_isect; the shape indices stay in [0].w and [3].w
__global__ __launch_bounds__(256) void k_su_pairs(const float4* __restrict__ isect, uint32_t first_tri, uint32_t np, float4* __restrict__ pairs) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  float4* out = pairs + 6 * (size_t)p;
  for (int k = 0; k < 2; k++) {
    const float shape_bits = out[3 * k].w;
    const size_t t = __float_as_uint(shape_bits) - first_tri;
    float4 a = isect[3 * t];
    a.w = shape_bits;
    out[3 * k] = a; out[3 * k + 1] = isect[3 * t + 1]; out[3 * k + 2] = isect[3 * t + 2];
  }
}

// emit_rec (kernels/hj_device.h) as scene_upload.hip emitter_records fills it, from the arrays on the device
__global__ __launch_bounds__(64) void k_su_emitters(RefitShapes s, const hj_emitter* __restrict__ emitters, uint32_t ne,
                                                    const uint32_t* __restrict__ materials, const float4* __restrict__ emissive,
                                                    float4* __restrict__ rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ne) return;
  float4 r[hj::kEmitRecF4];
  for (uint32_t k = 0; k < hj::kEmitRecF4; k++) r[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t shape = emitters[i].shape;
  const float4 power = emissive[materials[shape] & HJ_MATERIAL_INDEX_MASK];
  uint32_t kind;
  if (shape < s.ns) {
    kind = 0;
    const float4 sp = s.spheres[shape];
    r[1] = make_float4(sp.x, sp.y, sp.z, 0.f);
    r[0].z = sp.w;
  } else if (shape < s.ns + s.nq) {
    kind = 1;
    const uint32_t q = shape - s.ns;
    for (int k = 0; k < 3; k++) { const float4 v = s.quads[3 * q + k]; r[1 + k] = make_float4(v.x, v.y, v.z, 0.f); }
  } else {
    kind = 2;
    const hj_triangle t = s.triangles[shape - s.ns - s.nq];
    for (int k = 0; k < 3; k++) {
      const hj_vertex v = s.vertices[t.v[k]];
      r[1 + k] = make_float4(v.pos[0], v.pos[1], v.pos[2], 0.f);
      r[4 + k] = make_float4(v.normal[0], v.normal[1], v.normal[2], 0.f);
    }
  }
  r[0].x = emitters[i].pdf;
  r[0].y = __uint_as_float(kind);
  r[1].w = power.x; r[2].w = power.y; r[3].w = power.z;
  for (uint32_t k = 0; k < hj::kEmitRecF4; k++) rec[(size_t)hj::kEmitRecF4 * i + k] = r[k];
}

// The first update of a scene: the link set and every buffer the later ones reuse, allocated into a set of its own that joins the
// scene's only when the links have been verified.  A tree the refit cannot take (a shape in two leaves or in none: an upload accepts
// such arrays) is refused with HJ_ERR_UNSUPPORTED and the scene stays as it is.
int prepare(hj_context* ctx) {
  hj_context::SceneUpdate& u = ctx->update;
  const hj::DeviceScene& d = ctx->scene;
  const size_t n = (size_t)d.ns + d.nq + d.nt, N = u.nodes0;
  if (!u.node_map || n < 2 || N != 2 * n - 1 || d.num_nodes - d.root2 != N)
    return set_error(ctx, HJ_ERR_UNSUPPORTED, "hj_scene_update_shapes: the uploaded tree has %zu records for %zu shapes: only a tree with one leaf per shape can be refitted", N, n);
  DevBufs bufs(ctx);
  uint2* links = nullptr;
  uint32_t* zeroed = nullptr;
  hj_context::SceneUpdate nu = u;
  HJ_TRY(bufs.alloc(links, N));
  HJ_TRY(bufs.alloc(nu.parent, N));
  HJ_TRY(bufs.alloc(nu.arrived, N));
  HJ_TRY(bufs.alloc(nu.scratch, 2 * N));
  HJ_TRY(bufs.alloc(nu.partial, refit_cost_partials((uint32_t)N)));
  HJ_TRY(bufs.alloc(nu.verdict, 4));
  HJ_TRY(bufs.alloc(nu.in_spheres, d.ns));
  HJ_TRY(bufs.alloc(nu.in_quads, 3 * (size_t)d.nq));
  HJ_TRY(bufs.alloc(nu.in_vertices, u.num_vertices));
  HJ_TRY(bufs.alloc(nu.in_emitters, d.num_emitters));
  HJ_TRY(bufs.alloc(zeroed, N + n + 4));
  nu.links = links;
  hipLaunchKernelGGL(k_su_links, dim3(((uint32_t)N + 255u) / 256u), dim3(256), 0, ctx->stream, d.nodes, d.root2, (uint32_t)N, links);
  const RefitLinks rl{links, nu.parent, nu.arrived, (uint32_t)N, (uint32_t)n};
  const int rc = refit_check_links(ctx, rl, zeroed, "hj_scene_update_shapes: the uploaded tree cannot be refitted");
  if (rc == HJ_ERR_INVALID) return HJ_ERR_UNSUPPORTED;       // (the message names what the links lack)
  HJ_TRY(rc);
  bufs.take(zeroed).release();
  bufs.move_into(ctx->scene_bufs);
  nu.ready = true;
  u = nu;
  return HJ_OK;
}

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

}  // namespace

extern "C" {

int hj_scene_update_shapes(hj_context* ctx, const hj_scene_desc* s, uint32_t flags, double* out_cost) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!s) return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: null scene");
  if (flags & ~(uint32_t)(HJ_UPDATE_DEVICE_ARRAYS | HJ_UPDATE_NO_LIGHT_GRID))
    return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: unknown flag bits 0x%x", flags);
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "hj_scene_update_shapes: no scene has been uploaded");
  hj_context::SceneUpdate& u = ctx->update;
  hj::DeviceScene& d = ctx->scene;
  if (s->num_spheres != d.ns || s->num_quads != d.nq || s->num_triangles != d.nt || s->num_vertices != u.num_vertices || s->num_emitters != d.num_emitters)
    return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: %zu / %zu / %zu shapes, %zu vertices, %zu emitters; the uploaded scene has %u / %u / %u, %zu, %u",
                     s->num_spheres, s->num_quads, s->num_triangles, s->num_vertices, s->num_emitters, d.ns, d.nq, d.nt, u.num_vertices, d.num_emitters);
  if ((s->num_spheres && !s->spheres) || (s->num_quads && !s->quads) || (s->num_vertices && !s->vertices) || (s->num_emitters && !s->emitters))
    return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: null array with non-zero count");
  if (!finite3(s->camera.position) || !finite3(s->camera.rotation) || !std::isfinite(s->camera.rotation[3]) || !std::isfinite(s->camera.fov))
    return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: the camera is not finite");
  const bool on_device = (flags & HJ_UPDATE_DEVICE_ARRAYS) != 0;
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  HJ_TRY(sync_all(ctx));
  const Tuning tn = ctx->tuning = Tuning::from_env();
  hipStream_t st = ctx->stream;
  StageClock clock{tn.lbvh_timing != 0, "hj_scene_update_shapes: %-28s %7.2f ms\n", st};
  if (!u.ready) {
    HJ_TRY(prepare(ctx));
    clock.mark("first update: link set");
  }
  const uint32_t N = (uint32_t)u.nodes0, nv = (uint32_t)u.num_vertices, ne = d.num_emitters;
  const dim3 blk(256);
  auto blocks = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };

  // ---- everything up to the verdict reads live buffers and writes only scratch and staging
  RefitShapes sh{};
  sh.ns = d.ns; sh.nq = d.nq; sh.nt = d.nt;
  sh.triangles = d.triangles;
  if (on_device) {
    sh.spheres = reinterpret_cast<const float4*>(s->spheres); sh.quads = reinterpret_cast<const float4*>(s->quads); sh.vertices = s->vertices;
  } else {
    if (d.ns) HJ_HIP(ctx, hipMemcpyAsync(u.in_spheres, s->spheres, sizeof(float4) * d.ns, hipMemcpyHostToDevice, st));
    if (d.nq) HJ_HIP(ctx, hipMemcpyAsync(u.in_quads, s->quads, sizeof(float4) * 3 * d.nq, hipMemcpyHostToDevice, st));
    if (nv) HJ_HIP(ctx, hipMemcpyAsync(u.in_vertices, s->vertices, sizeof(hj_vertex) * nv, hipMemcpyHostToDevice, st));
    sh.spheres = u.in_spheres; sh.quads = u.in_quads; sh.vertices = u.in_vertices;
  }
  if (ne) HJ_HIP(ctx, hipMemcpyAsync(u.in_emitters, s->emitters, sizeof(hj_emitter) * ne, hipMemcpyHostToDevice, st));
  HJ_HIP(ctx, hipMemsetAsync(u.verdict, 0, sizeof(uint32_t) * 4, st));
  clock.mark("shape arrays to the device");
  const size_t checked = (size_t)d.ns + 3 * (size_t)d.nq + nv + ne;
  hipLaunchKernelGGL(k_su_check, blocks(checked), blk, 0, st, sh, nv, u.in_emitters, ne, d.materials, u.verdict);
  const RefitLinks rl{u.links, u.parent, u.arrived, N, d.ns + d.nq + d.nt};
  refit_enqueue(ctx, rl, sh, u.scratch, tn.refit_tiled != 0);
  if (out_cost) refit_enqueue_cost(ctx, u.scratch, N, u.partial);
  uint32_t verdict[4] = {0, 0, 0, 0};
  HJ_HIP(ctx, hipMemcpyAsync(verdict, u.verdict, sizeof verdict, hipMemcpyDeviceToHost, st));
  HJ_HIP(ctx, hipStreamSynchronize(st));                     // the one synchronisation before a live buffer is written
  HJ_HIP(ctx, hipGetLastError());
  clock.mark("checks + bottom-up pass");
  if (verdict[0] & kSuNonFinite) return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: a coordinate or a radius is not finite");
  if (verdict[0] & kSuEmitterRange) return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: an emitter names a shape out of range");
  if (verdict[0] & kSuEmitterNotEmissive) return set_error(ctx, HJ_ERR_INVALID, "hj_scene_update_shapes: an emitter names a shape that is not emissive");
  std::vector<double> partial;
  hj_bvh_node root{};
  std::vector<hj_bvh_node> host_tree;
  std::vector<hj_sphere> h_spheres;
  std::vector<hj_quad> h_quads;
  std::vector<hj_vertex> h_vertices;
  std::vector<hj_triangle> h_triangles;
  const bool regrid = d.light_grid != nullptr && !(flags & HJ_UPDATE_NO_LIGHT_GRID);
  try {
    if (out_cost) partial.resize(refit_cost_partials(N));
    if (regrid) {
      host_tree.resize(N); h_triangles.resize(d.nt);
      if (on_device) { h_spheres.resize(d.ns); h_quads.resize(d.nq); h_vertices.resize(nv); }
    }
  } catch (const std::bad_alloc&) {
    return set_error(ctx, HJ_ERR_NOMEM, "out of host memory");
  }

  // ---- from here on only a device error can fail: the scene is released then, as after a failed upload
  auto run = [&]() -> int {
    float4* nodes = const_cast<float4*>(d.nodes);
    if (d.ns) HJ_HIP(ctx, hipMemcpyAsync(const_cast<float4*>(d.spheres), sh.spheres, sizeof(float4) * d.ns, hipMemcpyDeviceToDevice, st));
    if (d.nq) HJ_HIP(ctx, hipMemcpyAsync(const_cast<float4*>(d.quads), sh.quads, sizeof(float4) * 3 * d.nq, hipMemcpyDeviceToDevice, st));
    if (nv) HJ_HIP(ctx, hipMemcpyAsync(const_cast<hj_vertex*>(d.vertices), sh.vertices, sizeof(hj_vertex) * nv, hipMemcpyDeviceToDevice, st));
    if (ne) HJ_HIP(ctx, hipMemcpyAsync(const_cast<hj_emitter*>(d.emitters), u.in_emitters, sizeof(hj_emitter) * ne, hipMemcpyDeviceToDevice, st));
    clock.mark("shape arrays into the scene");
    hipLaunchKernelGGL(k_su_scatter, blocks(N), blk, 0, st, u.scratch, u.node_map, u.parent, N, d.root2, sh, s->camera.position[0], s->camera.position[1],
                       s->camera.position[2], nodes);
    clock.mark("scatter");
    if (d.nt) hipLaunchKernelGGL(k_su_triangles, blocks(d.nt), blk, 0, st, d.triangles, sh.vertices, d.nt, const_cast<float4*>(d.tri_isect),
                                 const_cast<float4*>(d.tri_shade));
    if (u.num_pairs) hipLaunchKernelGGL(k_su_pairs, blocks(u.num_pairs), blk, 0, st, d.tri_isect, d.ns + d.nq, (uint32_t)u.num_pairs,
                                        const_cast<float4*>(d.tri_pair));
    if (ne) hipLaunchKernelGGL(k_su_emitters, dim3((ne + 63u) / 64u), dim3(64), 0, st, sh, u.in_emitters, ne, d.materials, d.emissive,
                               const_cast<float4*>(d.emit_rec));
    clock.mark("triangle, pair, emitter records");
    if (out_cost) {
      HJ_HIP(ctx, hipMemcpyAsync(partial.data(), u.partial, sizeof(double) * partial.size(), hipMemcpyDeviceToHost, st));
      HJ_HIP(ctx, hipMemcpyAsync(&root, u.scratch, sizeof root, hipMemcpyDeviceToHost, st));
    }
    if (regrid) {
      HJ_HIP(ctx, hipMemcpyAsync(host_tree.data(), u.scratch, sizeof(hj_bvh_node) * N, hipMemcpyDeviceToHost, st));
      if (d.nt) HJ_HIP(ctx, hipMemcpyAsync(h_triangles.data(), d.triangles, sizeof(hj_triangle) * d.nt, hipMemcpyDeviceToHost, st));
      if (on_device) {
        if (d.ns) HJ_HIP(ctx, hipMemcpyAsync(h_spheres.data(), sh.spheres, sizeof(hj_sphere) * d.ns, hipMemcpyDeviceToHost, st));
        if (d.nq) HJ_HIP(ctx, hipMemcpyAsync(h_quads.data(), sh.quads, sizeof(hj_quad) * d.nq, hipMemcpyDeviceToHost, st));
        if (nv) HJ_HIP(ctx, hipMemcpyAsync(h_vertices.data(), sh.vertices, sizeof(hj_vertex) * nv, hipMemcpyDeviceToHost, st));
      }
    }
    HJ_HIP(ctx, hipStreamSynchronize(st));                   // (the caller's arrays have been read; the host copies are complete)
    HJ_HIP(ctx, hipGetLastError());
    clock.mark("copies to the host");
    d.camera = s->camera;
    d.tan_half_fov = (float)std::tan((double)(0.5f * s->camera.fov) * (3.14159265358979323846 / 180.0));
    // The light-shaft grid's proofs are about the old geometry: never kept.  A scene that had one gets a new one from the same
    // builder over the refitted tree, or none.
    if (d.light_grid) {
      ctx->scene_bufs.take(d.light_grid).release();
      d.light_grid = nullptr;
      d.lg_res = 0;
      if (regrid) {
        hj_scene_desc g = *s;
        g.bvh = host_tree.data(); g.num_bvh_nodes = N;
        g.triangles = h_triangles.data();
        if (on_device) { g.spheres = h_spheres.data(); g.quads = h_quads.data(); g.vertices = h_vertices.data(); }
        DevBufs grid_bufs(ctx);
        HJ_TRY(upload_light_grid(grid_bufs, &g, tn, nullptr, d));
        grid_bufs.move_into(ctx->scene_bufs);
        clock.mark("light-shaft grid");
      }
    }
    return HJ_OK;
  };
  const int rc = run();
  if (rc != HJ_OK) {
    (void)hipStreamSynchronize(st);
    release_scene(ctx);
    return rc;
  }
  if (out_cost) *out_cost = refit_cost(partial, root);
  return HJ_OK;
}

// The device node array and the kept map, for tests that look at records and not only at frames.  records: 8 floats per record,
// capacity_records of them (NULL: only info); info: num_nodes, root, root2, num_hot; map (may be NULL): 2 words per node of the
// uploaded array (num_nodes - root2 of them) - its record, its guard's record, 0xFFFFFFFF for none.
int hj_debug_scene_tree(hj_context* ctx, float* records, size_t capacity_records, uint32_t info[4], uint32_t* map) {
  if (!ctx) return HJ_ERR_INVALID;
  HJ_NOT_BUSY(ctx);
  HJ_NOT_PIPELINED(ctx);
  if (!ctx->have_scene) return set_error(ctx, HJ_ERR_STATE, "hj_debug_scene_tree: no scene has been uploaded");
  const hj::DeviceScene& d = ctx->scene;
  if (info) { info[0] = d.num_nodes; info[1] = d.root; info[2] = d.root2; info[3] = d.num_hot; }
  if (records && capacity_records < d.num_nodes)
    return set_error(ctx, HJ_ERR_INVALID, "hj_debug_scene_tree: room for %zu records, the scene has %u", capacity_records, d.num_nodes);
  HJ_HIP(ctx, hipSetDevice(ctx->device));
  HJ_TRY(sync_all(ctx));
  if (records) HJ_HIP(ctx, hipMemcpy(records, d.nodes, sizeof(float4) * 2 * d.num_nodes, hipMemcpyDeviceToHost));
  if (map) {
    if (!ctx->update.node_map) return set_error(ctx, HJ_ERR_STATE, "hj_debug_scene_tree: the scene keeps no map");
    HJ_HIP(ctx, hipMemcpy(map, ctx->update.node_map, sizeof(uint2) * ctx->update.nodes0, hipMemcpyDeviceToHost));
  }
  return HJ_OK;
}

}  // extern "C"
