// Every environment switch of libhijiki_hip.so, in ONE table, read in ONE place (hjapi::Tuning::from_env): an entry point that
// uses a switch reads the table once at its start and passes the struct down - no getenv anywhere else in the library.
// None of the switches changes a result bit (tests/test_gpu_parity.py::test_tuning_switches_never_change_a_bit on a frame,
// tests/test_switch_matrix_gpu.py through every query and render call; tests/test_tuning_table_host.py demands a test for every
// row added here); the defaults are the measured optima (DESIGN.md section 4 "Tuning switches", profiles/NOTES.md).  Plain C++: api/light_grid.cpp (g++) includes it too.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace hjapi {

struct Tuning {
  static constexpr int kUnset = -0x7fffffff;               // "chosen where it is used": by tree size, by call size
  // X(field, "NAME", default, lowest, highest)            what it is
#define HJ_TUNING_TABLE(X)                                                                                                              \
  /* context (read by hj_context_create) */                                                                                            \
  X(slots, "HJ_SLOTS", 3, 1, 4)                            /* batches in flight (kMaxSlots = 4) */                                      \
  X(pool, "HJ_POOL", 32768, 64, 1 << 20)                   /* record positions per workgroup */                                         \
  X(wg_per_cu, "HJ_WG_PER_CU", 8, 1, 32)                   /* persistent workgroups per CU, large render call */                        \
  X(wg_small, "HJ_WG_SMALL", 6, 1, 32)                     /* ... of a small one (a rank's share on 4 - 8 GPUs) */                      \
  X(recon_priority, "HJ_RECON_PRIORITY", 1, 0, 1)          /* reconstructions on a high-priority stream */                              \
  /* render calls */                                                                                                                   \
  X(batch_cap, "HJ_BATCH_CAP", 8192, 64, 32768)            /* blocks per batch, upper bound */                                          \
  X(wg_small_blocks, "HJ_WG_SMALL_BLOCKS", 12288, 0, 1 << 30) /* calls below this many blocks are "small" */                            \
  X(xcd_deal, "HJ_XCD_DEAL", 0, 0, 1)                      /* XCD-aware deal of sample groups (measured: -7 % on c4) */                 \
  X(lds_pad_kb, "HJ_LDS_PAD_KB", 0, 0, 64)                 /* dynamic LDS padding of the path kernel (occupancy experiments) */         \
  X(mem_limit_mb, "HJ_MEM_LIMIT_MB", 0, 0, 1 << 30)        /* test rig: pretend this little device memory is free */                    \
  X(alloc_limit_mb, "HJ_ALLOC_LIMIT_MB", 0, 0, 1 << 30)    /* test rig: allocations beyond this total fail (read once per process) */  \
  /* scene upload: what is derived from the uploaded tree, and where */                                                                \
  X(upload_device, "HJ_UPLOAD_DEVICE", -1, -1, 1)          /* re-layout on the device: -1 from upload_device_min nodes on */            \
  X(upload_device_min, "HJ_UPLOAD_DEVICE_MIN", 100000, 0, 1 << 30)                                                                      \
  X(upload_timing, "HJ_UPLOAD_TIMING", 0, 0, 1)            /* stage times on stderr */                                                  \
  X(pair_leaves, "HJ_PAIR_LEAVES", -1, -1, 1)              /* pair nodes: -1 from pair_min_nodes nodes on */                            \
  X(pair_min_nodes, "HJ_PAIR_MIN_NODES", 0, 0, 1 << 30)                                                                                 \
  X(collapse_pct, "HJ_COLLAPSE_PCT", 50, 0, 1000)          /* collapse threshold, per cent of the kept ancestor's area */               \
  X(leaf_guards, "HJ_LEAF_GUARDS", 2, 0, 3)                /* 2: triangle and quad leaves; 1 / 3 add the INEXACT sphere guards */       \
  X(node_order, "HJ_NODE_ORDER", -1, -1, 1)                /* cold nodes: 0 pre-order, 1 sibling groups, -1 by tree */                  \
  X(stream_state, "HJ_STREAM_STATE", -1, -1, 1)            /* non-temporal path-state accesses: -1 from stream_min_nodes nodes on */    \
  X(stream_min_nodes, "HJ_STREAM_MIN_NODES", 300000, 0, 1 << 30) /* "large tree" (also: 8 x 8 packets, no light grid, full shadow votes) */ \
  X(group_tile, "HJ_GROUP_TILE", -1, -1, 1)                /* camera packets of 8 x 8 pixels instead of 64 x 1: -1 on large trees */    \
  X(inner_burst, "HJ_INNER_BURST", kUnset, 1, 1 << 20)     /* box steps per round of the walk loop: 6 (8 on large trees) */            \
  X(refill_min, "HJ_REFILL_MIN", kUnset, 1, 64)            /* idle lanes that trigger a refill: 24 (32) */                              \
  X(light_grid, "HJ_LIGHT_GRID", kUnset, 0, 256)           /* cells per axis of the light-shaft grid: 64, none on large trees */        \
  X(light_grid_mesh, "HJ_LIGHT_GRID_MESH", 1, 0, 1)        /* also cells on meshes and in corners (flat shapes, not coplanar): bundle proofs */ \
  /* multi-GPU test rigs */                                                                                                            \
  X(comm_shared_gpu, "HJ_COMM_SHARED_GPU", 0, 0, 1)        /* several contexts of a communicator on one GPU (kernel sum) */             \
  X(comm_force_rccl, "HJ_COMM_FORCE_RCCL", 0, 0, 1)        /* RCCL also for a one-rank communicator */                                  \
  /* device BVH build + ray vote */                                                                                                    \
  X(lbvh_timing, "HJ_LBVH_TIMING", 0, 0, 1)                                                                                             \
  X(lbvh_big_pct, "HJ_LBVH_BIG_PCT", 2, 0, 100)            /* shapes above this share of the scene's box area stay out of the Morton tree */ \
  X(lbvh_cluster, "HJ_LBVH_CLUSTER", 512, 0, 1 << 20)      /* leaves per SAH-re-split cluster */                                        \
  X(lbvh_sah, "HJ_LBVH_SAH", 1, 0, 1)                                                                                                   \
  X(lbvh_top_rotate, "HJ_LBVH_TOP_ROTATE", -1, -1, 64)     /* rotation passes over the host-built top: -1 by size */                    \
  X(lbvh_vote_paths, "HJ_LBVH_VOTE_PATHS", 60000, 0, 1 << 24) /* camera paths of the ray vote at the end of the build */                \
  X(refit_tiled, "HJ_REFIT_TILED", 1, 0, 1)                /* hj_refit_bvh_device: 1 subtrees inside a run of records in LDS, 0 the plain climb */ \
  X(bvh_child_order, "HJ_BVH_CHILD_ORDER", 3, 0, 9)        /* static child order of the device build (3: fewer shapes first) */         \
  /* hj_trace_rays (read when the context is created and by every upload, render call and build: not per query) */                     \
  X(trace_persistent, "HJ_TRACE_PERSISTENT", 1, 0, 1)      /* 1 the persistent walk with ray replacement (k_rq_walk), 0 one thread per ray (k_rq_plain) */ \
  X(trace_wg_rays, "HJ_TRACE_WG_RAYS", 2048, 64, 1 << 24)  /* rays per workgroup segment of the persistent form */                      \
  X(trace_chunk, "HJ_TRACE_CHUNK", 1 << 22, 64, 0x7FFFFFFF) /* rays per launch (and per staging buffer of host arrays) */               \
  X(closest_ordered, "HJ_CLOSEST_ORDERED", 1, 0, 1)      /* hj_closest_points: 1 nearer child first with an LDS stack, 0 the stackless walk alone */ \
  /* hj_trace_paths (read like hj_trace_rays' rows).  Path state costs about 250 B per position (181 B, 213 B with tinted glass, 4 B more   \
     with an environment, rounded up), a sample 32 B: the defaults bound a query's path state at 2048 x 2048 x 250 B = 1 GB - as many    \
     workgroups as a 256-CU device keeps resident at 8 per CU, each with 32 rounds' worth of a full workgroup in flight - and its       \
     samples at 128 MB; a small query takes what its sample count needs */                                                              \
  X(paths_pool, "HJ_PATHS_POOL", 2048, 64, 1 << 19)        /* positions per workgroup (rounded down to a multiple of 64) */             \
  X(paths_wgs, "HJ_PATHS_WGS", 2048, 1, 4096)              /* most workgroups per launch (fewer when the chunk has fewer 64-sample groups) */ \
  X(paths_chunk, "HJ_PATHS_CHUNK", 1 << 22, 64, 0x7FFFFFFF) /* samples per launch (the sample index shares its word with kCameraFlag) */  \
  X(bvh_vote_shadow, "HJ_BVH_VOTE_SHADOW", kUnset, 0, 16)  /* a shadow ray's vote in quarters of a closest-hit ray's: 1 (4 on large trees) */ \
  /* hj_lightmap_texels / hj_bake_lightmap (read like hj_trace_rays' rows: as the context's creation or its last upload, render     \
     call or build found them - the light-map calls themselves do not refresh the table) */                                          \
  X(lightmap_lane_texels, "HJ_LIGHTMAP_LANE_TEXELS", 64, 0, 1 << 28) /* k_lm_owner: a texel box up to this size is one lane's, a larger one k_lm_owner_wide's */ \
  X(lightmap_slices, "HJ_LIGHTMAP_SLICES", kUnset, 1, 256) /* grid rows of k_lm_owner_wide that share a box: as many as fill the device, at most 256 */ \
  /* hj_filter_lightmap / hj_bake_lightmap_filtered (read like the rows above) */                                                        \
  X(lightmap_filter_lds_step, "HJ_LIGHTMAP_FILTER_LDS_STEP", 128, 0, 128) /* steps up to this take k_lm_filter_lds, larger ones k_lm_filter_direct: 0 never, 128 always (measured faster at every step) */ \
  /* hj_denoise_frame (read like the rows above) */                                                                                      \
  X(denoise_lds_step, "HJ_DENOISE_LDS_STEP", 8, 0, 128)    /* steps up to this take k_dn_filter_lds, larger ones k_dn_filter_direct: 0 never, 128 always (measured: faster up to step 8, slower at 16) */
  // presence flags (debugging aids): set to anything = on
#define HJ_TUNING_FLAGS(X)                                                                                                              \
  X(trace_bounces, "HJ_TRACE_BOUNCES")                     /* per-bounce table of the split-kernel path on stderr */                    \
  X(relayout_debug, "HJ_RL_DEBUG")                         /* device re-layout: intermediate arrays checked on the host */              \
  X(light_grid_timing, "HJ_LIGHT_GRID_TIMING")             /* light-shaft grid: stage times on stderr */

#define HJ_X_FIELD(field, name, dflt, lo, hi) int field = dflt;
  HJ_TUNING_TABLE(HJ_X_FIELD)
#undef HJ_X_FIELD
#define HJ_X_FLAG(field, name) bool field = false;
  HJ_TUNING_FLAGS(HJ_X_FLAG)
#undef HJ_X_FLAG

  static int pick(int value, int where_unset) { return value == kUnset ? where_unset : value; }

  static Tuning from_env() {                                // THE place where the library reads its environment
    Tuning t;
    auto read = [](const char* name, int dflt, int lo, int hi) {
      const char* v = std::getenv(name);
      if (!v || !*v) return dflt;
      return std::min(hi, std::max(lo, std::atoi(v)));
    };
#define HJ_X_READ(field, name, dflt, lo, hi) t.field = read(name, dflt, lo, hi);
    HJ_TUNING_TABLE(HJ_X_READ)
#undef HJ_X_READ
#define HJ_X_READ_FLAG(field, name) t.field = std::getenv(name) != nullptr;
    HJ_TUNING_FLAGS(HJ_X_READ_FLAG)
#undef HJ_X_READ_FLAG
    return t;
  }
};

}  // namespace hjapi
