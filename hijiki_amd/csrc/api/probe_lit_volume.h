// What api/probe_lit.hip holds for api/direct_lit.hip as well: the volume a probe-lit stage carries, its refusals and staging, and the
// two AovStage hooks that do not depend on the resolve.  The including unit has included hj_internal.h.
#pragma once
#define HJ_PROBE_VIS_NO_KERNELS        // PvGrid and PvvMap, by value in Lit: the look-up kernels stay in the units that hold them
#include "../kernels/hj_probe_vis.h"

namespace hjapi {

enum class LitLookup { kPlain, kVisible, kPlaced };

// What a call's stage carries: the volume on the device and which look-up reads it
struct Lit {
  LitLookup lookup;
  hj::PvGrid g;
  hj::PvvMap v;
  const float4* d_probes;
  const float2* d_atlas;
  const float4* d_place;
};

// AovStage::reserve and ::points of a probe-lit stage (st.self: its Lit; nullptr: no volume, k_pl_points alone and no look-up)
int lit_reserve(hj_context* ctx, const AovStage& st, size_t slots);
hipError_t lit_points(hj_context* ctx, const AovStage& st, const hj_image_block* d_blocks, uint32_t nb, const float4* d_hits, bool followed);
// the volume's refusals, without a device (any: the call has blocks) -> lit's look-up, grid and map; np; reads_atlas
int lit_check(hj_context* ctx, const char* fn, const hj_probe_lighting* l, bool any, Lit& lit, uint32_t& np, bool& reads_atlas);
// behind the gate: the volume's device arrays - the caller's own, or staged copies enqueued on the context's stream, once a call
int lit_stage(hj_context* ctx, const char* fn, const hj_probe_lighting* l, uint32_t np, bool reads_atlas, Lit& lit);

}  // namespace hjapi
