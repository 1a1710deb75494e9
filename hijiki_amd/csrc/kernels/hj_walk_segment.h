// The shell of a kernel that walks a flat segment of entries through trace_persistent (hj_walk.h): THE text of its prologue and of
// the three records every such kernel writes, for k_rq_walk (api/ray_query.hip), k_aov_walk (hj_aov.h), k_mv_walk (hj_motion.h) and
// the follow rounds (chain_round, hj_chain.h).  The path kernels' own prologues differ (their USE_BVH and n != 0 guards) and stay
// where they are: this header includes hj_stages.h and edits nothing.  No global atomics, no inline assembly of its own.
#pragma once
#include "hj_stages.h"

#pragma clang fp contract(off)

namespace hj {

// a lane's hit record before its ray enters the walk
HJ_DEV void walk_reset(RawHit& h) { h.t = 0.f; h.u = 0.f; h.v = 0.f; h.id = -1; }

// The range of a fetched ray: (eps, +inf), the next segment of a path (render.glsl:33), or for an entry without a ray the empty range
// [+inf, -inf]: it fails every box and shape test and leaves the tree at the first node.
HJ_DEV void walk_empty_range(Ray& r, bool valid) {
  r.tmin = valid ? kEps : kInf;
  r.tmax = valid ? kInf : -kInf;
}

// the record of a finished ray: (objectID bits, t, u, v); a miss: (-1, 0, 0, 0)
HJ_DEV float4 walk_hit_record(const RawHit& h) {
  const bool hit = h.id >= 0;
  return make_float4(__int_as_float(hit ? h.id : -1), hit ? h.t : 0.f, hit ? h.u : 0.f, hit ? h.v : 0.f);
}

// Workgroup g walks entries [g * wg_rays, min(n, (g + 1) * wg_rays)) of the launch's n (the grid is ceil(n / wg_rays), so its
// first entry is below n): its waves pull them from the segment's head in LDS beside the copy of the hot nodes.
//   fetch(q, slot, ray, any, h)   trace_persistent's fetch with the GLOBAL entry index q in place of the segment's own
//   finish(done, slot, h, any)    trace_persistent's finish as it stands
template <int MODE, bool PAIRS, class Fetch, class Finish>
HJ_DEV void walk_segment(const DeviceScene& sc, uint32_t n, uint32_t wg_rays, Fetch fetch, Finish finish) {
  __shared__ WgShared sh;
  const uint32_t first = blockIdx.x * wg_rays;
  const uint32_t cnt = n - first < wg_rays ? n - first : wg_rays;
  if (threadIdx.x == 0) sh.head = 0;
  load_hot_nodes(sc, sh);
  __syncthreads();
  trace_persistent<MODE, PAIRS>(sc, cnt, &sh.head, sh.nodes,
                                [&](uint32_t i, uint32_t& slot, Ray& r, bool& any, RawHit& h) { fetch(first + i, slot, r, any, h); }, finish);
}

}  // namespace hj
