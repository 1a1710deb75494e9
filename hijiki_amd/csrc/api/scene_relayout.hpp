// hj_scene_upload's re-layout of the reference's tree into the kernels' records (kernels/hj_device.h): on the host
// (scene_upload.hip, small trees and arrays that are not trees) or on the device (scene_relayout.hip, large trees and the tree
// hj_build_bvh_device left there).  Both allocate what the scene keeps into the caller's set and fill the same RelayoutOut.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hj_internal.h"

namespace hjapi {

struct RelayoutOut {
  const float4* nodes = nullptr;       // 2 x float4 per record, placed inside one 4 GiB window
  const float4* tri_isect = nullptr;
  const float4* tri_shade = nullptr;
  const float4* tri_pair = nullptr;
  uint32_t num_nodes = 0, root = 0, root2 = 0, num_hot = 0, num_pairs = 0;   // root2: the second copy of the tree (the reference's own)
  size_t kept = 0;                     // records without padding
  const uint2* node_map = nullptr;     // per node of the uploaded array: (its record, its guard record), hj_context::SceneUpdate::kNoRecord for none
};

// The host path: every array comes from `s` (leaf guards, collapse, pair nodes, hot-first order, the second copy of the tree).
int relayout_on_host(hj_context* ctx, const hj_scene_desc* s, const Tuning& tn, StageClock& clock, DevBufs& keep, RelayoutOut& out);

// d_tris / d_verts: the scene's triangle and vertex arrays, already on the device.  node_order: HJ_NODE_ORDER (-1: by tree).
// HJ_ERR_UNSUPPORTED: the array is not a tree (or a node has more kept children than the kernels enumerate) - the caller takes the
// host path; `keep` may hold some of this call's buffers then.
int relayout_on_device(hj_context* ctx, const hj_scene_desc* s, const hj_triangle* d_tris, const hj_vertex* d_verts, bool pairs_on,
                       int node_order, float collapse_thr, bool timing, DevBufs& keep, RelayoutOut& out, const hj_bvh_node* d_tree = nullptr);

// The node array (rec_bytes of records) in a new buffer of `bufs` that does not cross a 4 GiB boundary.  kept: records without
// padding (for the error message).
int place_node_array(DevBufs& bufs, size_t rec_bytes, size_t kept, float4** out);

// One triangle's pre-gathered records (kernels/hj_device.h: tri_isect, tri_shade): ONE text for the upload (k_rl_triangles) and for
// hj_scene_update_shapes (k_su_triangles); b - a and c - a are the single IEEE subtractions the host's gather performs.
__device__ inline void tri_records(const hj_triangle* __restrict__ tris, const hj_vertex* __restrict__ verts, uint32_t i,
                                   float4* __restrict__ isect, float4* __restrict__ shade) {
  const hj_vertex A = verts[tris[i].v[0]], B = verts[tris[i].v[1]], C = verts[tris[i].v[2]];
  isect[3 * (size_t)i + 0] = make_float4(A.pos[0], A.pos[1], A.pos[2], 0.f);
  isect[3 * (size_t)i + 1] = make_float4(B.pos[0] - A.pos[0], B.pos[1] - A.pos[1], B.pos[2] - A.pos[2], 0.f);
  isect[3 * (size_t)i + 2] = make_float4(C.pos[0] - A.pos[0], C.pos[1] - A.pos[1], C.pos[2] - A.pos[2], 0.f);
  shade[4 * (size_t)i + 0] = make_float4(A.normal[0], A.normal[1], A.normal[2], A.u);
  shade[4 * (size_t)i + 1] = make_float4(B.normal[0], B.normal[1], B.normal[2], B.u);
  shade[4 * (size_t)i + 2] = make_float4(C.normal[0], C.normal[1], C.normal[2], C.u);
  shade[4 * (size_t)i + 3] = make_float4(A.v, B.v, C.v, 0.f);
}

}  // namespace hjapi
