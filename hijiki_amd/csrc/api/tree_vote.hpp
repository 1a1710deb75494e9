// The ray-voted child order on the device (kernels/hj_vote.h): host half, shared by hj_tune_bvh_device and hj_build_bvh_device.
#pragma once
#include "hj_internal.h"

namespace hjapi {

struct VoteShapes {               // the shape arrays of an hj_scene_desc, on the device
  const float4* spheres;          // hj_sphere
  const float4* quads;            // hj_quad as 3 x float4
  const hj_triangle* triangles;
  const hj_vertex* vertices;
};

struct VoteResult { uint32_t exchanged = 0, levels = 0; };
struct VoteGains { unsigned long long *l = nullptr, *r = nullptr; };   // [N] each, on the device: kernels/hj_vote.h gain_l / gain_r

// The two stages of vote_on_device, which calls one and then the other; hj_debug_vote_gains and hj_debug_vote_exchange enter them
// on their own.
//   vote_sample    uploads the tags, emitters and dielectrics of `s` and two zeroed gain arrays into buffers of `sc` and enqueues
//                  k_vote_paths over `paths` camera paths (0: no launch, the gains stay zero); w_shadow from the context's tuning.
//                  clock (may be NULL): the "uploads" and "sampled paths" marks of HJ_LBVH_TIMING
//   vote_exchange  d_nodes[N] re-ordered by gain_l / gain_r (device arrays of N words) into d_out[N]; the stream is drained.
//                  info: [0] levels that held an inner node  [1] nodes whose children were exchanged  [2] the kernels' error bits.
//                  Fewer than 3 records: a copy.  HJ_ERR_INVALID: links that are not a tree's (the kernels check what they need to
//                  walk, not all a tree must hold: the callers bring validated or device-built links); HJ_ERR_UNSUPPORTED: more than
//                  hj::vote::kMaxLevels levels
int vote_sample(hj_context* ctx, const hj_scene_desc* s, const VoteShapes& shapes, const hj_bvh_node* d_nodes, size_t N, size_t paths, DevBufs& sc,
                VoteGains& gains, StageClock* clock);
int vote_exchange(hj_context* ctx, const hj_bvh_node* d_nodes, size_t N, const unsigned long long* gain_l, const unsigned long long* gain_r,
                  hj_bvh_node* d_out, uint32_t info[4]);

// d_nodes[N]: a flattened tree (pre-order skip-link records) over the shapes of `s`, on the device.  Samples `paths` camera paths
// of `s` (camera, materials, emitters: uploaded here), exchanges the children of the inner nodes where the sample finds the other
// order cheaper and writes the re-ordered array to d_out[N] (device, not d_nodes).  HJ_ERR_INVALID when the links are not a tree's.
int vote_on_device(hj_context* ctx, const hj_scene_desc* s, const VoteShapes& shapes, const hj_bvh_node* d_nodes, size_t N, size_t paths,
                   hj_bvh_node* d_out, bool timing, VoteResult* result);

// (position, record) pairs into a device array of records
int put_records(hj_context* ctx, const std::vector<std::pair<uint32_t, hj_bvh_node>>& records, hj_bvh_node* d_array);

}  // namespace hjapi
