// The stages of a refit (kernels/hj_lbvh.h "REFIT", launched from api/lbvh_build.hip) for a caller that brings its own link set:
// hj_refit_bvh_device over hj_context::refit_links, hj_scene_update_shapes over the uploaded scene's topology.  Everything runs on the
// context's stream; all pointers are device pointers.
#pragma once
#include "hj_internal.h"

namespace hjapi {

struct RefitLinks {
  const uint2* links;          // [N] (shape_index, exit_index) of a pre-order skip-link tree with one shape per leaf
  uint32_t* parent;            // [N] derived by refit_check_links
  uint32_t* arrived;           // [N] the climb's counters: zeroed by refit_check_links, left zero by every pass
  uint32_t N, n;               // records, shapes (N = 2n - 1)
};
struct RefitShapes {
  const float4* spheres;       // hj_sphere
  const float4* quads;         // hj_quad as 3 x float4
  const hj_triangle* triangles;
  const hj_vertex* vertices;
  uint32_t ns, nq, nt;
};

// links -> parents and counters, with every check of a pre-order skip-link tree whose leaves hold each shape once.  zeroed: N + n + 4
// words of scratch.  One stream synchronisation brings the verdict: HJ_ERR_INVALID with a message that starts with `who`.
int refit_check_links(hj_context* ctx, const RefitLinks& l, uint32_t* zeroed, const char* who);
// The bottom-up pass: N 32-byte skip-link records into `out` (tiled: which kernel form - HJ_REFIT_TILED).  Enqueued only.
void refit_enqueue(hj_context* ctx, const RefitLinks& l, const RefitShapes& sh, float4* out, bool tiled);
// The cost's partial sums over such records, one double per 256 of them.  Enqueued only.
void refit_enqueue_cost(hj_context* ctx, const float4* records, uint32_t N, double* partial);
inline size_t refit_cost_partials(uint32_t N) { return (N + 255u) / 256u; }
// sum over inner nodes of area(node) / area(root) from the partial sums (added in index order) and the root record
double refit_cost(const std::vector<double>& partial, const hj_bvh_node& root);

}  // namespace hjapi
