// hj_trace_rays: caller-given rays through the uploaded tree - the public ray query ("Ray queries").
//
// The walk is the path kernel's own (kernels/hj_walk.h trace_persistent: in-wave ray replacement, merged first step, the LDS copy
// of the hot nodes, pair nodes, the second tree for rays outside general position), instantiated here with a fetch that reads the
// caller's ray array and a finish that writes one hit record per ray, behind the shell the flat segment walks share
// (kernels/hj_walk_segment.h).  Nothing of the kernel headers is restated or edited: this unit includes them (as api/render.hip
// does for the path kernels) and defines kernels of its own beside theirs.
//   k_rq_walk<ANY, PAIRS>   persistent form: a workgroup owns a contiguous segment of the rays and walks it with ray replacement
//   k_rq_plain<ANY>         plain form: one thread per ray through traverse() - the A/B partner (HJ_TRACE_PERSISTENT=0)
//   k_rq_surface            second pass, one thread per ray: the populated intersection and the material word of every hit
#include "hj_internal.h"
#include "../kernels/hj_walk_segment.h"

#pragma clang fp contract(off)

using namespace hjapi;

namespace hj {

// rays: two float4 per ray (origin.xyz, direction.x | direction.yz, tMin, tMax)
HJ_DEV Ray rq_ray(float4 a, float4 b) {
  Ray r; r.o = V(a.x, a.y, a.z); r.d = V(a.w, b.x, b.y); r.tmin = b.z; r.tmax = b.w;
  return r;
}

// Workgroup g walks rays [g * wg_rays, min(n, (g + 1) * wg_rays)): its waves pull them from the segment's head in LDS, a free lane
// takes the next index (consecutive free lanes read consecutive rays), a finished ray's record goes to its own index - so which
// lane or workgroup carried a ray shows in no result.
template <bool ANY, bool PAIRS>
__global__ __launch_bounds__(kBlockThreads) void k_rq_walk(DeviceScene sc, const float4* __restrict__ rays, uint32_t n, uint32_t wg_rays,
                                                           float4* __restrict__ hits) {
  const uint32_t first = blockIdx.x * wg_rays;                    // (walk_segment's: the arrays are addressed from the segment's start)
  const float4* __restrict__ seg_rays = rays + 2 * (size_t)first;
  float4* __restrict__ seg_hits = hits + first;
  auto fetch = [&](uint32_t q, uint32_t& slot, Ray& r, bool& any, RawHit& h) {
    const uint32_t i = q - first;
    slot = i;
    any = ANY;
    r = rq_ray(seg_rays[2 * i], seg_rays[2 * i + 1]);
    walk_reset(h);
  };
  auto finish = [&](bool done, uint32_t slot, const RawHit& h, bool) {
    if (done) seg_hits[slot] = walk_hit_record(h);
  };
  walk_segment<ANY ? 1 : 0, PAIRS>(sc, n, wg_rays, fetch, finish);
}

template <bool ANY>
__global__ __launch_bounds__(kBlockThreads) void k_rq_plain(DeviceScene sc, const float4* __restrict__ rays, uint32_t n,
                                                            float4* __restrict__ hits) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  RawHit h; h.t = 0.f; h.u = 0.f; h.v = 0.f;
  traverse<true, ANY>(sc, rq_ray(rays[2 * (size_t)i], rays[2 * (size_t)i + 1]), h);
  hits[i] = walk_hit_record(h);
}

// surface: four float4 per ray = p.xyz, n.xyz, u, v, ft.xyz, fb.xyz, material word, 0.  The hit point and populate* are the shade
// stage's (kernels/hj_stages.h stage_shade: fma(t, d, o), scene.glsl:164).  A pass of its own: inside the walk's finish it would
// take the walk's registers.
__global__ __launch_bounds__(kBlockThreads) void k_rq_surface(DeviceScene sc, const float4* __restrict__ rays, const float4* __restrict__ hits,
                                                              uint32_t n, float4* __restrict__ surface) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 hr = hits[i];
  const uint32_t id = (uint32_t)__float_as_int(hr.x);
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
  if (id < sc.ns + sc.nq + sc.nt) {                                // (a miss is 0xFFFFFFFF)
    const Ray r = rq_ray(rays[2 * (size_t)i], rays[2 * (size_t)i + 1]);
    Its its;
    its.p = V(fmaf(hr.y, r.d.x, r.o.x), fmaf(hr.y, r.d.y, r.o.y), fmaf(hr.y, r.d.z, r.o.z));
    if (id < sc.ns) populate_sphere(sc.spheres[id], its);
    else if (id < sc.ns + sc.nq) populate_quad(sc, id - sc.ns, hr.z, hr.w, its);
    else populate_triangle(sc, id - sc.ns - sc.nq, hr.z, hr.w, its);
    s0 = make_float4(its.p.x, its.p.y, its.p.z, its.n.x);
    s1 = make_float4(its.n.y, its.n.z, its.u, its.v);
    s2 = make_float4(its.ft.x, its.ft.y, its.ft.z, its.fb.x);
    s3 = make_float4(its.fb.y, its.fb.z, __uint_as_float(sc.materials[id]), 0.f);
  }
  float4* __restrict__ out = surface + 4 * (size_t)i;
  out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3;
}

}  // namespace hj

namespace hjapi {

// rays per workgroup: HJ_TRACE_WG_RAYS, fewer when the launch would otherwise leave CUs without a workgroup (never below one
// ray per thread)
uint32_t walk_wg_rays(const hj_context* ctx, uint32_t n) {
  const uint32_t per_cu = ((n + (uint32_t)ctx->num_cus - 1u) / (uint32_t)ctx->num_cus + 63u) / 64u * 64u;
  return std::min<uint32_t>((uint32_t)ctx->tuning.trace_wg_rays, std::max<uint32_t>(per_cu, (uint32_t)hj::kBlockThreads));
}

}  // namespace hjapi

namespace {

// one launch: rays [0, n) at `rays` -> `hits` (and `surface` unless null), all on the device
void launch_query(hj_context* ctx, const float4* rays, uint32_t n, bool any, float4* hits, float4* surface) {
  const hj::DeviceScene& sc = ctx->scene;
  hipStream_t s = ctx->stream;
  const dim3 blk(hj::kBlockThreads);
  if (ctx->tuning.trace_persistent != 0) {
    const uint32_t wg_rays = walk_wg_rays(ctx, n);
    const dim3 grid((n + wg_rays - 1u) / wg_rays);
    const bool pairs = sc.has_pairs != 0;
    if (any && pairs) hipLaunchKernelGGL((hj::k_rq_walk<true, true>), grid, blk, 0, s, sc, rays, n, wg_rays, hits);
    else if (any) hipLaunchKernelGGL((hj::k_rq_walk<true, false>), grid, blk, 0, s, sc, rays, n, wg_rays, hits);
    else if (pairs) hipLaunchKernelGGL((hj::k_rq_walk<false, true>), grid, blk, 0, s, sc, rays, n, wg_rays, hits);
    else hipLaunchKernelGGL((hj::k_rq_walk<false, false>), grid, blk, 0, s, sc, rays, n, wg_rays, hits);
  } else {
    if (any) hipLaunchKernelGGL(hj::k_rq_plain<true>, per_lane(n), blk, 0, s, sc, rays, n, hits);
    else hipLaunchKernelGGL(hj::k_rq_plain<false>, per_lane(n), blk, 0, s, sc, rays, n, hits);
  }
  if (surface) hipLaunchKernelGGL(hj::k_rq_surface, per_lane(n), blk, 0, s, sc, rays, static_cast<const float4*>(hits), n, surface);
}

}  // namespace

extern "C" {

// The argument checks come first and need neither a device nor a context's state (a refusal without a context leaves its text in
// hj_last_error(NULL), as hj_context_create's do).  Then the queries' gate (query_gate, api/path_query.hip): a null context, a frame
// in flight, frames in the pipeline, no scene.
int hj_trace_rays(hj_context* ctx, const float* rays, size_t n, uint32_t flags, float* hits, float* surface) {
  if (flags & ~(uint32_t)(HJ_TRACE_ANY_HIT | HJ_TRACE_DEVICE_ARRAYS)) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays: unknown flag bits 0x%x", flags);
  const bool any = (flags & HJ_TRACE_ANY_HIT) != 0, on_device = (flags & HJ_TRACE_DEVICE_ARRAYS) != 0;
  if (n != 0) {
    if (!rays || !hits) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays: null %s", !rays ? "rays" : "hits");
    if (n > 0x7FFFFFFFu) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays: %zu rays, at most 2^31 - 1 a call", n);
    if (surface && any) return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays: an any-hit record is no closest hit: no surface with HJ_TRACE_ANY_HIT");
    if (on_device && misaligned(rays, hits, surface))
      return set_error(ctx, HJ_ERR_INVALID, "hj_trace_rays: device arrays must be 16-byte aligned");
  }
  HJ_TRY(query_gate(ctx, __func__));
  if (n == 0) return HJ_OK;
  hj_context::RayQuery& q = ctx->query;
  const size_t f4 = sizeof(float4);
  const QueryArray arrays[] = {{rays, &q.rays, 2 * f4, false}, {hits, &q.hits, f4, true}, {surface, &q.surface, 4 * f4, true}};
  return chunked_query(ctx, __func__, n, on_device, arrays, [&](void* const d[], uint32_t cnt, size_t) {
    launch_query(ctx, static_cast<const float4*>(d[0]), cnt, any, static_cast<float4*>(d[1]), static_cast<float4*>(d[2]));
    return hipGetLastError();
  });
}

}  // extern "C"
