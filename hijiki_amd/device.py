"""ctypes mirror of the device C ABI (include/hijiki_hip.h -> libhijiki_hip.so).

`Renderer` plays the role of the reference's `Renderer` (src/main.rs:1143-1424)
for the hot path only: scene upload, the per-block render loop, read-back.
There is no CPU fallback: without the HIP library or a GPU every call raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("HIJIKI_HIP_LIB", os.path.join(_HERE, "lib", "libhijiki_hip.so"))
_LIB = None

# every symbol include/hijiki_hip.h declares
EXPORTS = ("hj_context_create", "hj_context_destroy", "hj_last_error", "hj_version", "hj_default_render_opts",
           "hj_scene_upload", "hj_framebuffer_create", "hj_framebuffer_clear", "hj_framebuffer_device_ptr",
           "hj_framebuffer_read", "hj_framebuffer_resolve", "hj_render_blocks", "hj_render_frame", "hj_block_seed",
           "hj_pass_offset", "hj_block_owner", "hj_debug_trace", "hj_debug_samples", "hj_reduce_framebuffers",
           "hj_build_bvh_device", "hj_render_frame_async", "hj_sync", "hj_set_progress_callback", "hj_device_count",
           "hj_comm_create", "hj_comm_destroy", "hj_comm_reduce_framebuffers", "hj_reserve", "hj_framebuffer_bind",
           "hj_pipeline_wait", "hj_debug_light_grid", "hj_debug_light_grid_planes", "hj_tune_bvh_device", "hj_bvh_device_read",
           "hj_scene_upload_textured", "hj_debug_texture_lookup", "hj_scene_upload_env", "hj_debug_env_lookup", "hj_debug_env_sample",
           "hj_debug_env_distribution", "hj_refit_bvh_device", "hj_scene_update_shapes", "hj_debug_scene_tree", "hj_debug_num",
           "hj_debug_shade_step", "hj_trace_rays", "hj_debug_reconstruct", "hj_trace_paths", "hj_trace_paths_adaptive",
           "hj_trace_irradiance", "hj_optimize_bvh_device", "hj_lightmap_texels", "hj_bake_lightmap", "hj_filter_lightmap",
           "hj_bake_lightmap_filtered", "hj_trace_irradiance_adaptive", "hj_bake_lightmap_adaptive", "hj_probe_points", "hj_bake_probes",
           "hj_sample_probes", "hj_debug_vote_cast", "hj_debug_vote_exchange", "hj_debug_vote_gains", "hj_probe_visibility_rays",
           "hj_bake_probe_visibility", "hj_sample_probes_visible", "hj_update_probes", "hj_update_probe_visibility", "hj_place_probes",
           "hj_update_probes_placed", "hj_update_probe_visibility_placed", "hj_sample_probes_visible_placed", "hj_closest_points",
           "hj_distance_field", "hj_trace_rays_all", "hj_points_inside", "hj_eval_materials", "hj_render_aovs", "hj_render_aovs_frame",
           "hj_denoise_frame", "hj_denoise_frame_temporal", "hj_render_motion", "hj_denoise_frame_temporal_motion",
           "hj_follow_specular", "hj_render_aovs_followed", "hj_render_aovs_frame_followed", "hj_render_motion_followed",
           "hj_render_probe_lit", "hj_render_probe_lit_frame", "hj_render_direct_lit", "hj_render_direct_lit_frame")

PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64)


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise ImportError(f"{HIP_LIB_PATH} missing: run `make hip` (or __graft_entry__.build()); "
                              "the HIP path has no fallback")
        L = C.CDLL(HIP_LIB_PATH)
        vp = C.c_void_p
        L.hj_context_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.hj_context_destroy.argtypes = [vp]
        L.hj_context_destroy.restype = None
        L.hj_last_error.argtypes = [vp]
        L.hj_last_error.restype = C.c_char_p
        L.hj_version.restype = C.c_uint32
        L.hj_default_render_opts.argtypes = [C.POINTER(abi.RenderOpts)]
        L.hj_default_render_opts.restype = None
        L.hj_scene_upload.argtypes = [vp, C.POINTER(abi.SceneDesc)]
        L.hj_scene_upload_textured.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(abi.TextureSet)]
        L.hj_debug_texture_lookup.argtypes = [vp, C.c_uint32, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float)]
        L.hj_scene_upload_env.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(abi.TextureSet), C.POINTER(abi.Environment)]
        L.hj_debug_env_lookup.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float)]
        L.hj_debug_env_sample.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_float)]
        L.hj_debug_env_distribution.argtypes = [C.POINTER(abi.TextureSet), C.POINTER(abi.Environment), C.POINTER(C.c_float),
                                                C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32),
                                                C.POINTER(C.c_double)]
        L.hj_framebuffer_create.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.hj_framebuffer_clear.argtypes = [vp]
        L.hj_framebuffer_device_ptr.argtypes = [vp]
        L.hj_framebuffer_device_ptr.restype = vp
        L.hj_framebuffer_read.argtypes = [vp, C.POINTER(C.c_float)]
        L.hj_framebuffer_resolve.argtypes = [vp, C.POINTER(C.c_float)]
        L.hj_render_blocks.argtypes = [vp, C.POINTER(abi.ImageBlock), C.c_size_t, C.POINTER(abi.RenderOpts),
                                       C.POINTER(abi.RenderStats)]
        L.hj_render_frame.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(abi.RenderOpts), C.POINTER(abi.RenderStats)]
        L.hj_reserve.argtypes = [vp, C.c_size_t, C.POINTER(abi.RenderOpts)]
        L.hj_framebuffer_bind.argtypes = [vp, vp]
        L.hj_pipeline_wait.argtypes = [vp, C.c_uint32, C.POINTER(abi.RenderStats)]
        L.hj_reduce_framebuffers.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
        L.hj_render_frame_async.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.POINTER(abi.RenderOpts)]
        L.hj_sync.argtypes = [vp, C.POINTER(abi.RenderStats)]
        L.hj_set_progress_callback.argtypes = [vp, PROGRESS_FN, vp, C.c_uint32]
        L.hj_set_progress_callback.restype = None
        L.hj_device_count.restype = C.c_int
        L.hj_comm_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
        L.hj_comm_destroy.argtypes = [vp]
        L.hj_comm_destroy.restype = None
        L.hj_comm_reduce_framebuffers.argtypes = [vp, C.c_int]
        L.hj_debug_trace.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.hj_trace_rays.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp]      # (host or device pointers)
        L.hj_trace_paths.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.POINTER(abi.RenderOpts), C.c_uint32, vp,
                                     C.POINTER(abi.RenderStats)]               # (host or device pointers)
        L.hj_trace_paths_adaptive.argtypes = [vp, vp, C.c_size_t, C.POINTER(abi.AdaptiveOpts), C.POINTER(abi.RenderOpts), C.c_uint32, vp, vp,
                                              C.POINTER(abi.RenderStats)]      # (host or device pointers)
        L.hj_trace_irradiance.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.POINTER(abi.RenderOpts), C.c_uint32, vp,
                                          C.POINTER(abi.RenderStats)]          # (host or device pointers)
        L.hj_lightmap_texels.argtypes = [vp, C.POINTER(abi.LightmapDesc), vp, C.c_size_t, vp, C.POINTER(C.c_size_t)]   # (host or device pointers)
        L.hj_bake_lightmap.argtypes = [vp, C.POINTER(abi.LightmapDesc), C.c_uint32, C.c_uint32, C.POINTER(abi.RenderOpts), vp,
                                       C.POINTER(C.c_size_t), C.POINTER(abi.RenderStats)]
        L.hj_filter_lightmap.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.POINTER(abi.LightmapFilter), vp]   # (host or device pointers)
        L.hj_bake_lightmap_filtered.argtypes = [vp, C.POINTER(abi.LightmapDesc), C.c_uint32, C.c_uint32, C.POINTER(abi.LightmapFilter),
                                                C.POINTER(abi.RenderOpts), vp, C.POINTER(C.c_size_t), C.POINTER(abi.RenderStats)]
        L.hj_trace_irradiance_adaptive.argtypes = [vp, vp, C.c_size_t, C.POINTER(abi.AdaptiveOpts), C.POINTER(abi.RenderOpts), C.c_uint32, vp, vp,
                                                   C.POINTER(abi.RenderStats)]  # (host or device pointers)
        L.hj_bake_lightmap_adaptive.argtypes = [vp, C.POINTER(abi.LightmapDesc), C.POINTER(abi.AdaptiveOpts), C.c_uint32, C.POINTER(abi.LightmapFilter),
                                                C.POINTER(abi.RenderOpts), vp, vp, C.POINTER(C.c_size_t), C.POINTER(abi.RenderStats)]
        L.hj_probe_points.argtypes = [vp, C.POINTER(abi.ProbeDesc), vp]      # (host or device pointers)
        L.hj_bake_probes.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.c_uint32, C.POINTER(abi.RenderOpts), vp, C.POINTER(abi.RenderStats)]
        L.hj_sample_probes.argtypes = [vp, C.POINTER(abi.ProbeDesc), vp, vp, C.c_size_t, vp]
        L.hj_probe_visibility_rays.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), C.c_uint32, C.c_uint32, vp]
        L.hj_bake_probe_visibility.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), vp]   # (host or device pointers)
        L.hj_sample_probes_visible.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), vp, vp, vp, C.c_size_t, vp]
        L.hj_update_probes.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeUpdate), C.c_uint32, C.POINTER(abi.RenderOpts), vp,
                                       C.POINTER(abi.RenderStats)]
        L.hj_update_probe_visibility.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), C.POINTER(abi.ProbeUpdate), vp]
        L.hj_place_probes.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), C.POINTER(abi.ProbePlace), vp]
        L.hj_update_probes_placed.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeUpdate), C.c_uint32, C.POINTER(abi.RenderOpts), vp, vp,
                                              C.POINTER(abi.RenderStats)]
        L.hj_update_probe_visibility_placed.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), C.POINTER(abi.ProbeUpdate), vp, vp]
        L.hj_sample_probes_visible_placed.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.POINTER(abi.ProbeVisDesc), vp, vp, vp, C.c_size_t, vp, vp]
        L.hj_closest_points.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, C.POINTER(C.c_uint64)]   # (host or device pointers)
        L.hj_distance_field.argtypes = [vp, C.POINTER(abi.ProbeDesc), C.c_float, C.c_uint32, vp]
        L.hj_trace_rays_all.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp]         # (host or device pointers)
        L.hj_points_inside.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp]
        L.hj_eval_materials.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]                     # (host or device pointers)
        L.hj_render_aovs.argtypes = [vp, C.POINTER(abi.ImageBlock), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.hj_render_aovs_frame.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.hj_follow_specular.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp]                    # (host or device pointers)
        L.hj_render_aovs_followed.argtypes = [vp, C.POINTER(abi.ImageBlock), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.hj_render_aovs_frame_followed.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.hj_render_probe_lit.argtypes = [vp, C.POINTER(abi.ImageBlock), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(abi.ProbeLighting), vp]
        L.hj_render_probe_lit_frame.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(abi.ProbeLighting), vp]
        L.hj_render_direct_lit.argtypes = L.hj_render_probe_lit.argtypes          # (lighting may be NULL)
        L.hj_render_direct_lit_frame.argtypes = L.hj_render_probe_lit_frame.argtypes
        L.hj_denoise_frame.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(abi.DenoiseOpts), vp]   # (host or device pointers)
        L.hj_denoise_frame_temporal.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(abi.DenoiseOpts), C.POINTER(abi.TemporalOpts), vp, vp, vp]
        L.hj_denoise_frame_temporal_motion.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(abi.DenoiseOpts), C.POINTER(abi.TemporalOpts), vp, vp, vp, vp]
        L.hj_render_motion.argtypes = [vp, C.POINTER(abi.SceneDesc), C.c_uint32, C.c_uint32, C.c_uint32, vp]   # (host or device pointers)
        L.hj_render_motion_followed.argtypes = [vp, C.POINTER(abi.SceneDesc), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.hj_debug_samples.argtypes = [vp, C.POINTER(abi.ImageBlock), C.POINTER(abi.RenderOpts), C.POINTER(C.c_float)]
        L.hj_build_bvh_device.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(abi.BvhNode), C.c_size_t, C.POINTER(C.c_size_t)]
        L.hj_tune_bvh_device.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(abi.BvhNode), C.c_size_t, C.c_size_t]
        L.hj_bvh_device_read.argtypes = [vp, C.POINTER(abi.BvhNode), C.c_size_t, C.POINTER(C.c_size_t)]
        L.hj_refit_bvh_device.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(abi.BvhNode), C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_double)]
        L.hj_optimize_bvh_device.argtypes = [vp, C.POINTER(abi.SceneDesc), C.c_uint32, C.POINTER(abi.BvhNode), C.c_size_t,
                                             C.POINTER(C.c_size_t), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        L.hj_scene_update_shapes.argtypes = [vp, C.POINTER(abi.SceneDesc), C.c_uint32, C.POINTER(C.c_double)]
        L.hj_debug_scene_tree.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.hj_debug_num.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]
        L.hj_debug_shade_step.argtypes = [vp, C.POINTER(abi.RenderOpts), C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.hj_debug_reconstruct.argtypes = [vp, C.POINTER(abi.ImageBlock), C.c_size_t, C.POINTER(abi.RenderOpts), C.POINTER(C.c_float)]
        u64p = C.POINTER(C.c_uint64)
        L.hj_debug_vote_cast.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(C.c_float), C.c_size_t, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_uint32), u64p, u64p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.hj_debug_vote_exchange.argtypes = [vp, C.POINTER(abi.BvhNode), C.c_size_t, u64p, u64p, C.POINTER(abi.BvhNode), C.c_size_t,
                                             C.POINTER(C.c_uint32)]
        L.hj_debug_vote_gains.argtypes = [vp, C.POINTER(abi.SceneDesc), C.c_size_t, u64p, u64p, C.c_size_t]
        L.hj_block_seed.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.hj_block_seed.restype = C.c_uint32
        L.hj_pass_offset.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_float)]
        L.hj_pass_offset.restype = None
        L.hj_block_owner.argtypes = [C.c_uint32] * 5
        L.hj_block_owner.restype = C.c_uint32
        _LIB = L
    return _LIB


def reduce_framebuffers(renderers, root=0):
    """hj_reduce_framebuffers: RCCL sum of the framebuffers of several in-process renderers (one per GPU) into `root`."""
    arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
    rc = lib().hj_reduce_framebuffers(arr, len(renderers), root)
    if rc != abi.HJ_OK:
        raise abi.HijikiError(rc, lib().hj_last_error(renderers[root]._h).decode())


def env_distribution(textures, env):
    """hj_debug_env_distribution (host code, no GPU): the environment's sampling distribution as hj_scene_upload_env builds it ->
    dict of (H, W) arrays prob, pdf, alias_prob, alias and the float weight_sum (0: a black environment).  Raises on a refusal."""
    t = textures.textures[env.texture]
    shape = (t.height, t.width)
    out = {k: np.zeros(shape, np.float32) for k in ("prob", "pdf", "alias_prob")}
    out["alias"] = np.zeros(shape, np.uint32)
    total = C.c_double()
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = lib().hj_debug_env_distribution(C.byref(textures), C.byref(env), f(out["prob"]), f(out["pdf"]), f(out["alias_prob"]),
                                         out["alias"].ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(total))
    if rc != abi.HJ_OK:
        raise abi.HijikiError(rc, "hj_debug_env_distribution refused the environment")
    out["weight_sum"] = total.value
    return out


def device_count():
    return lib().hj_device_count()


def resolve_aovs(aov):
    """The (height, width, 12) sums of `Renderer.render_aovs` as means -> dict(albedo (H, W, 3): words 0..2 over the sample count
    (word 3); normal (H, W, 3), depth (H, W): words 4..6 and 7 over the hit count (word 11); emission (H, W, 3): words 8..10 over the
    sample count; coverage (H, W): hits over samples), each 0 where its count is 0.  The normal mean is not renormalised.  A numpy
    array gives numpy arrays, a torch tensor tensors on its device."""
    if type(aov).__module__.split(".")[0] == "torch":
        import torch
        where, zero = torch.where, torch.zeros((), dtype=aov.dtype, device=aov.device)
    else:
        aov = np.asarray(aov, np.float32)
        where, zero = np.where, np.float32(0)
    if aov.ndim != 3 or aov.shape[2] != abi.AOV_WORDS:
        raise ValueError(f"resolve_aovs: (height, width, {abi.AOV_WORDS}) is needed (got {tuple(aov.shape)})")
    samples, hits = aov[..., 3], aov[..., 11]

    def mean(x, count):
        c = count if x.ndim == count.ndim else count[..., None]
        return where(c > 0, x / where(c > 0, c, zero + 1), zero)

    return dict(albedo=mean(aov[..., 0:3], samples), normal=mean(aov[..., 4:7], hits), depth=mean(aov[..., 7], hits),
                emission=mean(aov[..., 8:11], samples), coverage=mean(hits, samples))


def resolve_probe_lit(image):
    """The (height, width, 4) sums of `Renderer.render_probe_lit` or `Renderer.render_direct_lit` as the mean radiance -> (height, width, 3): words 0..2 over the
    sample count (word 3), 0 where no sample fell.  A numpy array gives a numpy array, a torch tensor a tensor on its device."""
    if type(image).__module__.split(".")[0] == "torch":
        import torch
        where, zero = torch.where, torch.zeros((), dtype=image.dtype, device=image.device)
    else:
        image = np.asarray(image, np.float32)
        where, zero = np.where, np.float32(0)
    if image.ndim != 3 or image.shape[2] != abi.PROBE_LIT_WORDS:
        raise ValueError(f"resolve_probe_lit: (height, width, {abi.PROBE_LIT_WORDS}) is needed (got {tuple(image.shape)})")
    c = image[..., 3:4]
    return where(c > 0, image[..., 0:3] / where(c > 0, c, zero + 1), zero)


def motion_ids(m):
    """word 3 of `render_motion`'s records as uint32 (height, width): the shape the pixel's centre ray hits, abi.MOTION_NONE for a
    pixel without a previous position.  m: the (height, width, 4) float32 array or tensor; a view where the type allows one."""
    if isinstance(m, np.ndarray):
        return np.ascontiguousarray(m, np.float32).view(np.uint32)[..., 3]
    import torch
    return m.contiguous().view(torch.int32)[..., 3].cpu().numpy().view(np.uint32)


class Comm:
    """hj_comm: the in-process contexts (one per GPU) + their RCCL communicators, made once and reused by every reduce."""

    def __init__(self, renderers):
        self.renderers = list(renderers)
        self._h = C.c_void_p()
        self._destroy = lib().hj_comm_destroy
        arr = (C.c_void_p * len(self.renderers))(*[r._h for r in self.renderers])
        rc = lib().hj_comm_create(arr, len(self.renderers), C.byref(self._h))
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, lib().hj_last_error(self.renderers[0]._h).decode())

    def reduce(self, root=0):
        rc = lib().hj_comm_reduce_framebuffers(self._h, root)
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, lib().hj_last_error(self.renderers[root]._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def default_opts():
    o = abi.RenderOpts()
    lib().hj_default_render_opts(C.byref(o))
    return o


def default_filter_sigmas(compiled):
    """(sigma_position, sigma_normal, sigma_color) the command line's `--filter N` uses for a compiled scene with a host tree: 1 % of
    the root box's diagonal, 0.5, 0 (float32 arithmetic, as the CLI computes it).  A starting point, not a tuned optimum."""
    root = compiled.bvh_f32[0]
    d = root[4:7] - root[0:3]
    return float(np.float32(0.01) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])), 0.5, 0.0


def stats_dict(st):
    return {n: getattr(st, n) for n, _ in abi.RenderStats._fields_}


class Renderer:
    """One GPU context: scene + framebuffer + render calls."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = int(device)
        self._destroy = lib().hj_context_destroy     # bound now: module globals may be gone at interpreter exit
        rc = lib().hj_context_create(device, C.byref(self._h))
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, lib().hj_last_error(None).decode())
        self.width = self.height = 0

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, lib().hj_last_error(self._h).decode())

    def upload_scene(self, compiled, device_tree=False, textures=None, environment=None):
        """hj_scene_upload.  device_tree: scene->bvh = NULL - the tree `build_bvh(compiled, keep_on_device=True)` left on the device.
        A compiled scene with image textures goes up with them (hj_scene_upload_textured); `textures` (an abi.TextureSet) overrides.
        A compiled scene with an environment (host.Scene.set_environment) goes up with it (hj_scene_upload_env); `environment` (an
        abi.Environment) overrides."""
        if environment is None:
            environment = getattr(compiled, "environment", None)
        desc = compiled.desc if hasattr(compiled, "desc") else compiled
        if textures is None and hasattr(compiled, "texture_set"):
            t = compiled.texture_set
            textures = t if t.num_textures else None
        if device_tree:
            d2 = abi.SceneDesc()
            C.memmove(C.byref(d2), C.byref(desc), C.sizeof(abi.SceneDesc))
            d2.bvh = None
            d2.num_bvh_nodes = 0
            desc = d2
        if environment is not None:
            self._check(lib().hj_scene_upload_env(self._h, C.byref(desc), C.byref(textures) if textures is not None else None,
                                                  C.byref(environment)))
        elif textures is not None:
            self._check(lib().hj_scene_upload_textured(self._h, C.byref(desc), C.byref(textures)))
        else:
            self._check(lib().hj_scene_upload(self._h, C.byref(desc)))

    def env_lookup(self, dirs):
        """hj_debug_env_lookup: (n, 3) directions -> (n, 3) float32 radiance of the uploaded environment."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        rgb = np.zeros((len(d), 3), np.float32)
        self._check(lib().hj_debug_env_lookup(self._h, d.ctypes.data_as(C.POINTER(C.c_float)), len(d),
                                              rgb.ctypes.data_as(C.POINTER(C.c_float))))
        return rgb

    def env_sample(self, rng_states):
        """hj_debug_env_sample: n uint32 RNG states -> (n, 8) float32: direction xyz, pdf, texel index, Le / pdf rgb."""
        s = np.ascontiguousarray(rng_states, np.uint32).reshape(-1)
        out = np.zeros((len(s), 8), np.float32)
        self._check(lib().hj_debug_env_sample(self._h, s.ctypes.data_as(C.POINTER(C.c_uint32)), len(s),
                                              out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def create_framebuffer(self, width, height, external_device_ptr=None):
        self._check(lib().hj_framebuffer_create(self._h, width, height, external_device_ptr))
        self.width, self.height = width, height

    def clear(self):
        self._check(lib().hj_framebuffer_clear(self._h))

    @property
    def framebuffer_ptr(self):
        return lib().hj_framebuffer_device_ptr(self._h)

    def render_blocks(self, blocks, opts=None):
        st = abi.RenderStats()
        n = len(blocks)
        self._check(lib().hj_render_blocks(self._h, blocks, n, C.byref(opts) if opts is not None else None,
                                           C.byref(st)))
        return stats_dict(st)

    def render_frame(self, spp, master_seed, pass_begin=0, pass_end=None, rank=0, world=1, opts=None):
        st = abi.RenderStats()
        pass_end = spp if pass_end is None else pass_end
        self._check(lib().hj_render_frame(self._h, spp, master_seed, pass_begin, pass_end, rank, world,
                                          C.byref(opts) if opts is not None else None, C.byref(st)))
        return stats_dict(st)

    def submit_frame(self, spp, master_seed, pass_begin=0, pass_end=None, rank=0, world=1, opts=None):
        """hj_render_frame with HJ_RENDER_NO_DRAIN: returns when the frame's batches are enqueued; `pipeline_wait` joins.
        The frame accumulates into the framebuffer bound at the time of the call (`bind_framebuffer`)."""
        o = abi.RenderOpts()
        C.memmove(C.byref(o), C.byref(opts if opts is not None else default_opts()), C.sizeof(abi.RenderOpts))
        o.flags |= abi.RENDER_NO_DRAIN
        pass_end = spp if pass_end is None else pass_end
        self._check(lib().hj_render_frame(self._h, spp, master_seed, pass_begin, pass_end, rank, world, C.byref(o), None))

    def bind_framebuffer(self, device_ptr):
        """hj_framebuffer_bind: frames submitted from now on accumulate into this caller-owned buffer (no synchronisation)."""
        self._check(lib().hj_framebuffer_bind(self._h, device_ptr))

    def pipeline_wait(self, keep=0):
        """hj_pipeline_wait: until at most `keep` submitted frames are in flight; keep = 0 drains and returns the statistics of
        all frames since the last drain."""
        st = abi.RenderStats()
        self._check(lib().hj_pipeline_wait(self._h, keep, C.byref(st) if keep == 0 else None))
        return stats_dict(st) if keep == 0 else None

    def reserve(self, total_blocks, opts=None):
        """hj_reserve: allocate now what a render call of `total_blocks` ImageBlocks will use (set-up, not rendering)."""
        self._check(lib().hj_reserve(self._h, int(total_blocks), C.byref(opts) if opts is not None else None))

    def render_frame_async(self, spp, master_seed, pass_begin=0, pass_end=None, rank=0, world=1, opts=None):
        """hj_render_frame on the context's worker thread; `sync()` waits for it and returns the statistics."""
        pass_end = spp if pass_end is None else pass_end
        self._check(lib().hj_render_frame_async(self._h, spp, master_seed, pass_begin, pass_end, rank, world,
                                                C.byref(opts) if opts is not None else None))

    def sync(self):
        st = abi.RenderStats()
        self._check(lib().hj_sync(self._h, C.byref(st)))
        return stats_dict(st)

    def set_progress(self, fn, interval_blocks=128):
        """fn(blocks_done, blocks_total) whenever `interval_blocks` more ImageBlocks have completed; None = off."""
        self._progress = PROGRESS_FN(lambda _u, d, t: fn(d, t)) if fn else PROGRESS_FN()
        lib().hj_set_progress_callback(self._h, self._progress, None, interval_blocks)

    def build_bvh(self, compiled, keep_on_device=False):
        """LBVH over the shapes of `compiled`, built on the device (hj_build_bvh_device): (2 * shapes - 1, 8) uint32
        records in the reference's layout.  `compiled.set_bvh(nodes)` installs it.  keep_on_device: nothing comes back to the host
        (returns the record count): `upload_scene(compiled, device_tree=True)` takes the tree over, `read_device_bvh()` copies it out."""
        if keep_on_device:
            got = C.c_size_t(0)
            self._check(lib().hj_build_bvh_device(self._h, C.byref(compiled.desc), None, 0, C.byref(got)))
            return got.value
        n = 2 * compiled.num_shapes - 1
        nodes = np.zeros((max(n, 1), 8), np.uint32)
        got = C.c_size_t(0)
        self._check(lib().hj_build_bvh_device(self._h, C.byref(compiled.desc), nodes.ctypes.data_as(C.POINTER(abi.BvhNode)),
                                              len(nodes), C.byref(got)))
        return nodes[:got.value]

    def refit_bvh(self, compiled, topology=None, keep_on_device=False, cost=False):
        """hj_refit_bvh_device: the boxes of a tree recomputed for the shapes of `compiled` as they are now (`compiled.vertices`,
        `.spheres`, `.quads` are writable views: an animation writes into them); the links stay.  `topology`: an (N, 8) uint32 array
        whose shape and exit words are the tree (its boxes are ignored; the context keeps the links), None = the links the last
        refit with a topology left.  Returns the (2 * shapes - 1, 8) uint32 records, or with keep_on_device=True their count
        (`upload_scene(compiled, device_tree=True)` takes the tree over, `read_device_bvh()` copies it out); with cost=True a pair
        (that, the tree's surface-area cost: sum over inner nodes of area(node) / area(root))."""
        d = abi.SceneDesc()
        C.memmove(C.byref(d), C.byref(compiled.desc), C.sizeof(abi.SceneDesc))
        if topology is None:
            d.bvh = None
            d.num_bvh_nodes = 0
        else:
            topology = np.ascontiguousarray(topology, np.uint32).reshape(-1, 8)
            d.bvh = topology.ctypes.data_as(C.POINTER(abi.BvhNode))
            d.num_bvh_nodes = len(topology)
        got = C.c_size_t(0)
        sa = C.c_double(0.0)
        nodes = None if keep_on_device else np.zeros((max(2 * compiled.num_shapes - 1, 1), 8), np.uint32)
        self._check(lib().hj_refit_bvh_device(self._h, C.byref(d), None if nodes is None else nodes.ctypes.data_as(C.POINTER(abi.BvhNode)),
                                              0 if nodes is None else len(nodes), C.byref(got), C.byref(sa) if cost else None))
        out = got.value if keep_on_device else nodes[:got.value]
        return (out, sa.value) if cost else out

    def optimize_bvh_device(self, compiled=None, passes=8, keep_on_device=True):
        """hj_optimize_bvh_device: the tree `build_bvh` / `refit_bvh` left on the device (keep_on_device=True there), optimised by at
        most `passes` passes of parallel reinsertion; it replaces that tree.  compiled: the scene whose rays vote the child order of
        the new tree (None: no vote).  Returns a dict: `nodes` (the record count, or with keep_on_device=False the (N, 8) uint32
        records), `cost_before`, `cost_after` (surface-area cost, as `refit_bvh`'s), `moves` (subtrees moved)."""
        passes = int(passes)
        if not 0 <= passes <= abi.REINSERT_MAX_PASSES:
            raise ValueError(f"passes must be 0 ... {abi.REINSERT_MAX_PASSES}")
        got, moves = C.c_size_t(0), C.c_uint32(0)
        before, after = C.c_double(0.0), C.c_double(0.0)
        nodes = None
        if not keep_on_device:
            self._check(lib().hj_bvh_device_read(self._h, None, 0, C.byref(got)))
            nodes = np.zeros((max(got.value, 1), 8), np.uint32)
        self._check(lib().hj_optimize_bvh_device(self._h, None if compiled is None else C.byref(compiled.desc), passes,
                                                 None if nodes is None else nodes.ctypes.data_as(C.POINTER(abi.BvhNode)),
                                                 0 if nodes is None else len(nodes), C.byref(got), C.byref(before), C.byref(after),
                                                 C.byref(moves)))
        return {"nodes": got.value if keep_on_device else nodes[:got.value], "cost_before": before.value, "cost_after": after.value,
                "moves": moves.value}

    def update_shapes(self, compiled, device_arrays=None, light_grid=True, cost=False):
        """hj_scene_update_shapes: the uploaded scene's shapes moved in place - spheres, quads, vertices, emitters and camera of
        `compiled` as they are now; links, triangles, materials, textures and environment stay as uploaded.  device_arrays: a dict of
        torch tensors on the renderer's device (`vertices` (V, 8), `spheres` (S, 4), `quads` (Q, 12); float32, contiguous) read in
        place of the host arrays - ALL shape arrays then come from the device, so every kind the scene has must be there; torch's
        current stream is synchronised first.  light_grid=False: a scene with a light-shaft grid loses it instead of getting a new
        one.  cost=True: returns the refitted tree's surface-area cost (as `refit_bvh`)."""
        d = abi.SceneDesc()
        C.memmove(C.byref(d), C.byref(compiled.desc), C.sizeof(abi.SceneDesc))
        flags = 0 if light_grid else abi.UPDATE_NO_LIGHT_GRID
        if device_arrays is not None:
            import torch
            flags |= abi.UPDATE_DEVICE_ARRAYS
            for name, field, count, words, rec in (("spheres", "spheres", d.num_spheres, 4, abi.Sphere), ("quads", "quads", d.num_quads, 12, abi.Quad),
                                                   ("vertices", "vertices", d.num_vertices, 8, abi.Vertex)):
                t = device_arrays.get(name)
                if t is None:
                    if count:
                        raise ValueError(f"device_arrays lacks '{name}' ({count} records in the scene)")
                    continue
                if not (t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == count * words):
                    raise ValueError(f"device_arrays['{name}']: a contiguous float32 tensor of {count} x {words} on GPU {self.device} is needed"
                                     f" (got {tuple(t.shape)} {t.dtype} on {t.device})")
                setattr(d, field, C.cast(C.c_void_p(t.data_ptr() if count else None), C.POINTER(rec)))
            torch.cuda.current_stream().synchronize()
        sa = C.c_double(0.0)
        self._check(lib().hj_scene_update_shapes(self._h, C.byref(d), flags, C.byref(sa) if cost else None))
        return sa.value if cost else None

    def scene_tree(self):
        """hj_debug_scene_tree: dict of `records` (num_nodes, 8) uint32 - the device node array, both copies of the tree -, `map`
        (uploaded nodes, 2) uint32 - per uploaded node its record and its guard's record, 0xFFFFFFFF for none -, num_nodes, root,
        root2, num_hot."""
        info = (C.c_uint32 * 4)()
        self._check(lib().hj_debug_scene_tree(self._h, None, 0, info, None))
        records = np.zeros((max(info[0], 1), 8), np.uint32)
        where = np.zeros((max(info[0] - info[2], 1), 2), np.uint32)
        self._check(lib().hj_debug_scene_tree(self._h, records.ctypes.data_as(C.POINTER(C.c_float)), len(records), info,
                                              where.ctypes.data_as(C.POINTER(C.c_uint32))))
        return {"records": records[:info[0]], "map": where[:info[0] - info[2]], "num_nodes": info[0], "root": info[1], "root2": info[2],
                "num_hot": info[3]}

    def read_device_bvh(self):
        """hj_bvh_device_read: the tree the last build left on the device, (nodes, 8) uint32."""
        got = C.c_size_t(0)
        self._check(lib().hj_bvh_device_read(self._h, None, 0, C.byref(got)))
        nodes = np.zeros((max(got.value, 1), 8), np.uint32)
        self._check(lib().hj_bvh_device_read(self._h, nodes.ctypes.data_as(C.POINTER(abi.BvhNode)), len(nodes), C.byref(got)))
        return nodes[:got.value]

    def tune_bvh_device(self, compiled, vote_paths=60000):
        """The tree of `compiled` with its child order voted by `vote_paths` sampled camera paths on the device
        (hj_tune_bvh_device): (nodes, 8) uint32 records, same boxes and leaves.  `compiled.set_bvh(nodes)` installs it."""
        nodes = np.zeros((max(len(compiled.bvh), 1), 8), np.uint32)
        self._check(lib().hj_tune_bvh_device(self._h, C.byref(compiled.desc), nodes.ctypes.data_as(C.POINTER(abi.BvhNode)),
                                             len(nodes), int(vote_paths)))
        return nodes[:len(compiled.bvh)]

    def debug_vote_cast(self, compiled, rays, any_hit=False, w_shadow=1, hits=None):
        """hj_debug_vote_cast: what the (n, 8) float32 `rays` add to the vote's gains in the tree of `compiled`.  hits: None (the
        vote's own closest hit), or (leaf positions (n,) - abi.VOTE_MISS for a miss -, t (n,) float32).  Returns gain_l, gain_r
        (N,) uint64 and found (n, 4) uint32: leaf position, shape, t bits, 0."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n, N = len(rays), len(compiled.bvh)
        given = None
        if hits is not None:
            given = np.zeros((n, 2), np.uint32)
            given[:, 0] = np.asarray(hits[0], np.uint32)
            given[:, 1] = np.ascontiguousarray(hits[1], np.float32).view(np.uint32)
        gl, gr, found = np.zeros(max(N, 1), np.uint64), np.zeros(max(N, 1), np.uint64), np.zeros((max(n, 1), 4), np.uint32)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        self._check(lib().hj_debug_vote_cast(self._h, C.byref(compiled.desc), rays.ctypes.data_as(C.POINTER(C.c_float)), n, int(bool(any_hit)),
                                             int(w_shadow), None if given is None else given.ctypes.data_as(u32p), gl.ctypes.data_as(u64p),
                                             gr.ctypes.data_as(u64p), len(gl), found.ctypes.data_as(u32p)))
        return gl[:N], gr[:N], found[:n]

    def debug_vote_exchange(self, nodes, gain_l, gain_r):
        """hj_debug_vote_exchange: the (N, 8) uint32 records re-ordered by the (N,) uint64 gains -> (records, exchanged, levels)."""
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
        gl, gr = np.ascontiguousarray(gain_l, np.uint64), np.ascontiguousarray(gain_r, np.uint64)
        if gl.shape != (len(nodes),) or gr.shape != (len(nodes),):
            raise ValueError("debug_vote_exchange: one gain of each side per record")
        out = np.zeros((max(len(nodes), 1), 8), np.uint32)
        info = (C.c_uint32 * 4)()
        u64p, bp = C.POINTER(C.c_uint64), C.POINTER(abi.BvhNode)
        self._check(lib().hj_debug_vote_exchange(self._h, nodes.ctypes.data_as(bp), len(nodes), gl.ctypes.data_as(u64p), gr.ctypes.data_as(u64p),
                                                 out.ctypes.data_as(bp), len(out), info))
        return out[:len(nodes)], int(info[1]), int(info[0])

    def debug_vote_gains(self, compiled, paths):
        """hj_debug_vote_gains: gain_l, gain_r (N,) uint64 as `paths` sampled camera paths of `compiled` leave them."""
        N = len(compiled.bvh)
        gl, gr = np.zeros(max(N, 1), np.uint64), np.zeros(max(N, 1), np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(lib().hj_debug_vote_gains(self._h, C.byref(compiled.desc), int(paths), gl.ctypes.data_as(u64p), gr.ctypes.data_as(u64p), len(gl)))
        return gl[:N], gr[:N]

    def trace(self, rays, use_bvh=True, any_hit=False):
        """intersectScene for (n,8) rays -> ids (n,) int32, t, u, v (n,) float32 (raw hit, before populate)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.zeros((len(rays), 4), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(lib().hj_debug_trace(self._h, rays.ctypes.data_as(fp), len(rays), int(use_bvh), int(any_hit),
                                         hits.ctypes.data_as(fp)))
        return hits[:, 0].copy().view(np.int32), hits[:, 1], hits[:, 2], hits[:, 3]

    def trace_rays(self, rays, any_hit=False, surface=False):
        """hj_trace_rays: (n, 8) rays (origin, direction of any length, tMin, tMax) through the uploaded tree -> ids (n,) int32 (-1: a
        miss), t, u, v (n,) float32 of the raw hit [, surface (n, 16) float32: p, n, u, v, ft, fb of the populated intersection, the
        hit shape's material word as float bits, 0; zeros for a miss].  any_hit: the walk stops at the first accepted hit - `ids >= 0`
        is the answer; no surface with it.  A float32 numpy array gives numpy arrays.  A contiguous float32 torch tensor on the
        renderer's GPU is read in place and gives tensors on that GPU (ids: an int32 view of the hit records' first column); torch's
        current stream is synchronised first."""
        if any_hit and surface:
            raise ValueError("trace_rays: no surface with any_hit (the record is not the closest hit)")
        flags = abi.TRACE_ANY_HIT if any_hit else 0
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not (rays.is_cuda and rays.device.index == self.device and rays.dtype == torch.float32 and rays.is_contiguous()
                    and rays.dim() == 2 and rays.shape[1] == 8):
                raise ValueError(f"trace_rays: a contiguous float32 tensor of (n, 8) on GPU {self.device} is needed"
                                 f" (got {tuple(rays.shape)} {rays.dtype} on {rays.device})")
            n = rays.shape[0]
            hits = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            surf = torch.empty((n, 16), dtype=torch.float32, device=rays.device) if surface else None
            torch.cuda.current_stream(rays.device).synchronize()      # (the allocations and whatever wrote `rays`)
            self._check(lib().hj_trace_rays(self._h, rays.data_ptr() if n else None, n, flags | abi.TRACE_DEVICE_ARRAYS,
                                            hits.data_ptr() if n else None, surf.data_ptr() if surface and n else None))
            out = (hits[:, 0].view(torch.int32), hits[:, 1], hits[:, 2], hits[:, 3])
            return out + ((surf,) if surface else ())
        rays = np.asarray(rays)
        if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"trace_rays: a float32 array of (n, 8) is needed (got {rays.shape} {rays.dtype})")
        rays = np.ascontiguousarray(rays)
        hits = np.zeros((len(rays), 4), np.float32)
        surf = np.zeros((len(rays), 16), np.float32) if surface else None
        self._check(lib().hj_trace_rays(self._h, rays.ctypes.data, len(rays), flags, hits.ctypes.data,
                                        surf.ctypes.data if surface else None))
        out = (hits[:, 0].copy().view(np.int32), hits[:, 1], hits[:, 2], hits[:, 3])
        return out + ((surf,) if surface else ())

    def closest_points(self, points, radius=float("inf"), stats=False, device=None):
        """hj_closest_points: the nearest surface point of the uploaded scene to each of n points -> (n, 8) float32 records: the shape
        index as int32 bits (-1: a miss), the distance, q (3), u, v, side; a miss is -1 and seven zeros.  points: (n, 4) = position
        and search radius, or (n, 3) with `radius` a scalar or (n,) values (+inf: unbounded).  A shape counts when its squared
        distance is <= radius^2; ties resolve to the lower shape index; a NaN or negative radius or a non-finite position is a miss.
        `side` is the facing of the nearest shape (+1: the side its normal cross(edge1, edge2) points to, or outside a sphere), not a
        robust inside / outside test.  A float32 numpy array gives a numpy array.  A float32 torch tensor on the renderer's GPU is
        read in place (an (n, 3) one is packed with its radii on that GPU first) and gives a tensor there; torch's current stream is
        synchronised first.  device: True / False demands a tensor / an array; None takes what comes.  stats=True: returns (records,
        {"nodes_visited", "shapes_tested"}) - functions of the points and the uploaded tree alone."""
        is_torch = type(points).__module__.split(".")[0] == "torch"
        if device is not None and bool(device) != is_torch:
            raise ValueError(f"closest_points: device={device} but points is a {'torch tensor' if is_torch else 'host array'}")
        st = (C.c_uint64 * 2)(0, 0)
        sp = st if stats else None
        if is_torch:
            import torch
            if not (points.is_cuda and points.device.index == self.device and points.dtype == torch.float32 and points.dim() == 2
                    and points.shape[1] in (3, 4)):
                raise ValueError(f"closest_points: a float32 tensor of (n, 3) or (n, 4) on GPU {self.device} is needed"
                                 f" (got {tuple(points.shape)} {points.dtype} on {points.device})")
            n = points.shape[0]
            if points.shape[1] == 3:
                r = torch.as_tensor(radius, dtype=torch.float32, device=points.device).expand(n) if not hasattr(radius, "shape") or radius.ndim == 0 \
                    else torch.as_tensor(radius, dtype=torch.float32, device=points.device).reshape(n)
                points = torch.cat([points, r.reshape(n, 1)], 1)
            points = points.contiguous()
            out = torch.empty((n, abi.CLOSEST_WORDS), dtype=torch.float32, device=points.device)
            torch.cuda.current_stream(points.device).synchronize()    # (the allocations and whatever wrote `points`)
            self._check(lib().hj_closest_points(self._h, points.data_ptr() if n else None, n, abi.CLOSEST_DEVICE_ARRAYS,
                                                out.data_ptr() if n else None, sp))
        else:
            points = np.asarray(points)
            if points.dtype != np.float32 or points.ndim != 2 or points.shape[1] not in (3, 4):
                raise ValueError(f"closest_points: a float32 array of (n, 3) or (n, 4) is needed (got {points.shape} {points.dtype})")
            n = len(points)
            if points.shape[1] == 3:
                points = np.concatenate([points, np.broadcast_to(np.asarray(radius, np.float32).reshape(-1, 1), (n, 1))], 1)
            points = np.ascontiguousarray(points, np.float32)
            out = np.zeros((n, abi.CLOSEST_WORDS), np.float32)
            self._check(lib().hj_closest_points(self._h, points.ctypes.data, n, 0, out.ctypes.data, sp))
        return (out, dict(nodes_visited=int(st[0]), shapes_tested=int(st[1]))) if stats else out

    def distance_field(self, origin, spacing, count, max_distance=float("inf"), signed=True, device=False):
        """hj_distance_field: the distance to the nearest surface of the uploaded scene on the grid of `probe_points` - point (x, y, z)
        at origin + (x, y, z) * spacing -, computed without the points leaving the device -> (nz, ny, nx) float32: side * distance
        (signed) or the distance alone.  Only shapes within `max_distance` count; a grid point without one gets max_distance
        (signed: +max_distance).  `side` is the facing of the nearest shape - which side of its plane, or of a sphere's surface, the
        point is on -, not a robust inside / outside test: near edges shared by faces that face differently the sign follows the
        shape with the lower index.  device=True: a torch tensor on the renderer's GPU."""
        d = self._probe_desc("distance_field", origin, spacing, count, 0, 1, 0.0, device)
        md = float(np.float32(max_distance))
        if not md >= 0:
            raise ValueError(f"distance_field: max_distance {max_distance}: >= 0 is needed (inf: no limit)")
        flags = 0 if signed else abi.DISTANCE_UNSIGNED
        shape = (d.count[2], d.count[1], d.count[0])
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            field = torch.empty(shape, dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            self._check(lib().hj_distance_field(self._h, C.byref(d), md, flags, field.data_ptr()))
            return field
        field = np.zeros(shape, np.float32)
        self._check(lib().hj_distance_field(self._h, C.byref(d), md, flags, field.ctypes.data))
        return field

    def _query_input(self, what, a, words):
        """(array or tensor, is_torch) of a query's (n, words) float32 input, by trace_rays' conventions"""
        if type(a).__module__.split(".")[0] == "torch":
            import torch
            if not (a.is_cuda and a.device.index == self.device and a.dtype == torch.float32 and a.is_contiguous() and a.dim() == 2
                    and a.shape[1] == words):
                raise ValueError(f"{what}: a contiguous float32 tensor of (n, {words}) on GPU {self.device} is needed"
                                 f" (got {tuple(a.shape)} {a.dtype} on {a.device})")
            return a, True
        a = np.asarray(a)
        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != words:
            raise ValueError(f"{what}: a float32 array of (n, {words}) is needed (got {a.shape} {a.dtype})")
        return np.ascontiguousarray(a), False

    def trace_rays_all(self, rays, max_hits=abi.ALLHITS_MAX_HITS):
        """hj_trace_rays_all: every hit of (n, 8) rays (origin, direction of any length, tMin, tMax) with the uploaded scene, the range
        never shrunk -> (counts (n,) uint32: the number of candidates; crossings (n,) int32: +1 for each that leaves through a surface,
        -1 for each that enters; hits (n, max_hits, 4) float32: per ray the min(count, max_hits) candidates nearest first as
        (shape index as int32 bits, t, u, v), the rest (-1, 0, 0, 0)).  max_hits: 0 ... abi.ALLHITS_MAX_HITS; 0 counts only.  Equal t
        goes to the lower shape index; a sphere gives its two roots (u = 0: the near one, 1: the far one).  The candidates are those
        of the query's own box test, not the closest-hit walk's.  A float32 numpy array gives numpy arrays.  A contiguous float32
        torch tensor on the renderer's GPU is read in place and gives tensors on that GPU; torch's current stream is synchronised
        first."""
        K = int(max_hits)
        if not 0 <= K <= abi.ALLHITS_MAX_HITS:
            raise ValueError(f"trace_rays_all: max_hits {max_hits}: 0 ... {abi.ALLHITS_MAX_HITS}")
        rays, is_torch = self._query_input("trace_rays_all", rays, 8)
        n = rays.shape[0]
        if is_torch:
            import torch
            counts = torch.empty((n, 2), dtype=torch.int32, device=rays.device)
            hits = torch.empty((n, K, 4), dtype=torch.float32, device=rays.device)
            torch.cuda.current_stream(rays.device).synchronize()      # (the allocations and whatever wrote `rays`)
            self._check(lib().hj_trace_rays_all(self._h, rays.data_ptr() if n else None, n, K, abi.ALLHITS_DEVICE_ARRAYS,
                                                counts.data_ptr() if n else None, hits.data_ptr() if n and K else None))
            return counts[:, 0], counts[:, 1], hits
        counts, hits = np.zeros((n, 2), np.uint32), np.zeros((n, K, 4), np.float32)
        self._check(lib().hj_trace_rays_all(self._h, rays.ctypes.data, n, K, 0, counts.ctypes.data, hits.ctypes.data if K else None))
        return counts[:, 0].copy(), counts[:, 1].copy().view(np.int32), hits

    def points_inside(self, points, parity=False):
        """hj_points_inside: whether each of (n, 4) points (position, one reserved word) lies inside closed geometry of the uploaded
        scene, by the signed crossings of three fixed rays (abi.INSIDE_DIRECTIONS) computed without leaving the device -> (inside (n,)
        uint32: 1 when at least two rays vote inside; votes (n,) uint32: how many did).  A ray votes inside when its crossing sum is
        > 0 - surfaces oriented outward -; parity=True: when it crosses an odd number of surfaces, for geometry without a consistent
        orientation.  Arrays and tensors as for trace_rays_all (tensors: counts as int32, torch has no uint32 arithmetic)."""
        flags = abi.INSIDE_PARITY if parity else 0
        points, is_torch = self._query_input("points_inside", points, 4)
        n = points.shape[0]
        if is_torch:
            import torch
            out = torch.empty((n, 2), dtype=torch.int32, device=points.device)
            torch.cuda.current_stream(points.device).synchronize()    # (the allocation and whatever wrote `points`)
            self._check(lib().hj_points_inside(self._h, points.data_ptr() if n else None, n, flags | abi.INSIDE_DEVICE_ARRAYS,
                                               out.data_ptr() if n else None))
            return out[:, 0], out[:, 1]
        out = np.zeros((n, 2), np.uint32)
        self._check(lib().hj_points_inside(self._h, points.ctypes.data, n, flags, out.ctypes.data))
        return out[:, 0].copy(), out[:, 1].copy()

    def eval_materials(self, hits, surface):
        """hj_eval_materials: the material at each of n hits -> (n, 8) float32 records: albedo (3), the uploaded material word as bits
        (abi.MATERIAL_MISS for a miss), emitted radiance (3), 0.  hits (n, 4) and surface (n, 16) are hj_trace_rays' two arrays - the
        hit records (shape id bits, t, u, v; `trace_rays` returns their columns: stack ids.view(float32), t, u, v) and the surface
        records.  Diffuse: its colour; checkerboard and image texture: evaluated at the surface record's (u, v); mirror and glass:
        albedo 1; an emitter: albedo 0 and its power as emission; a miss: zeros.  float32 numpy arrays give a numpy array.
        Contiguous float32 torch tensors on the renderer's GPU are read in place and give a tensor on that GPU; torch's current
        stream is synchronised first."""
        hits, is_torch = self._query_input("eval_materials", hits, 4)
        surface, surf_torch = self._query_input("eval_materials", surface, 16)
        if is_torch != surf_torch or hits.shape[0] != surface.shape[0]:
            raise ValueError(f"eval_materials: hits {tuple(hits.shape)} and surface {tuple(surface.shape)} must be n records of one kind (arrays or tensors)")
        n = hits.shape[0]
        if is_torch:
            import torch
            out = torch.empty((n, abi.MATERIALS_WORDS), dtype=torch.float32, device=hits.device)
            torch.cuda.current_stream(hits.device).synchronize()      # (the allocation and whatever wrote the inputs)
            self._check(lib().hj_eval_materials(self._h, hits.data_ptr() if n else None, surface.data_ptr() if n else None, n,
                                                abi.MATERIALS_DEVICE_ARRAYS, out.data_ptr() if n else None))
            return out
        out = np.zeros((n, abi.MATERIALS_WORDS), np.float32)
        self._check(lib().hj_eval_materials(self._h, hits.ctypes.data, surface.ctypes.data, n, 0, out.ctypes.data))
        return out

    def follow_specular(self, rays, hits):
        """hj_follow_specular: the specular continuation of n rays at their hits -> (n, 8) float32 rays in `trace_rays`' layout: where
        the hit is a mirror or a dielectric the next segment of the chain (hit point, reflected or refracted direction, tMin = eps,
        tMax = inf - a dielectric reflects when k <= 0 or fr >= 0.5, else refracts: no random draw), elsewhere - another material, a
        miss - the empty ray (zeros, tMin = inf, tMax = -inf), which `trace_rays` answers with a miss.  rays (n, 8) and hits (n, 4) are
        hj_trace_rays' arrays (stack ids.view(float32), t, u, v).  Alternated with `trace_rays` it gives the chains of
        `render_aovs(..., follow=N)`.  Arrays and tensors as for `eval_materials`."""
        rays, is_torch = self._query_input("follow_specular", rays, 8)
        hits, hits_torch = self._query_input("follow_specular", hits, 4)
        if is_torch != hits_torch or rays.shape[0] != hits.shape[0]:
            raise ValueError(f"follow_specular: rays {tuple(rays.shape)} and hits {tuple(hits.shape)} must be n records of one kind (arrays or tensors)")
        n = rays.shape[0]
        if is_torch:
            import torch
            out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
            torch.cuda.current_stream(rays.device).synchronize()      # (the allocation and whatever wrote the inputs)
            self._check(lib().hj_follow_specular(self._h, rays.data_ptr() if n else None, hits.data_ptr() if n else None, n,
                                                 abi.FOLLOW_DEVICE_ARRAYS, out.data_ptr() if n else None))
            return out
        out = np.zeros((n, 8), np.float32)
        self._check(lib().hj_follow_specular(self._h, rays.ctypes.data, hits.ctypes.data, n, 0, out.ctypes.data))
        return out

    def render_aovs(self, width, height, blocks=None, spp=None, master_seed=0, passes=None, device=False, follow=0):
        """hj_render_aovs / hj_render_aovs_frame: the first-hit AOVs of a frame's primary rays -> (height, width, 12) float32: per pixel
        the float32 sums, in block order, of its samples' records (albedo.rgb, 1 | shading normal.xyz, t | emission.rgb, 1 on a
        hit; a miss: 0, 0, 0, 1 and zeros) - `resolve_aovs` turns them into means.  blocks: a ctypes array (or list) of
        abi.ImageBlock, each with original_dimension == (width, height) and dimension <= 128; or spp [, master_seed, passes =
        (begin, end)]: the blocks `render_frame(spp, master_seed, begin, end)` renders on a width x height framebuffer.  Needs no
        framebuffer and leaves it alone.  device=True: a torch tensor on the renderer's GPU, written in place.
        follow (0 ... abi.AOV_MAX_FOLLOW): hj_render_aovs_followed / hj_render_aovs_frame_followed - a sample whose hit is a mirror or
        glass is followed through up to that many specular surfaces (`follow_specular`'s rule) and gets the record of its chain's last
        hit, its depth the sum of the chain's distances; a chain that ends in nothing keeps the record of the surface it left, so
        the hit count is unchanged.  0: the first hit, as ever."""
        if (blocks is None) == (spp is None):
            raise ValueError("render_aovs: either blocks or spp is needed")
        follow = int(follow)
        if not 0 <= follow <= abi.AOV_MAX_FOLLOW:
            raise ValueError(f"render_aovs: follow {follow}: 0 ... {abi.AOV_MAX_FOLLOW}")
        width, height = int(width), int(height)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            aov = torch.empty((height, width, abi.AOV_WORDS), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            ptr, flags = aov.data_ptr(), abi.AOV_DEVICE_ARRAY
        else:
            aov = np.zeros((height, width, abi.AOV_WORDS), np.float32)
            ptr, flags = aov.ctypes.data, 0
        if blocks is not None:
            if not isinstance(blocks, C.Array):
                blocks = (abi.ImageBlock * len(blocks))(*blocks)
            if follow:
                self._check(lib().hj_render_aovs_followed(self._h, blocks, len(blocks), width, height, follow, flags, ptr))
            else:
                self._check(lib().hj_render_aovs(self._h, blocks, len(blocks), width, height, flags, ptr))
        else:
            begin, end = (0, int(spp)) if passes is None else (int(passes[0]), int(passes[1]))
            if follow:
                self._check(lib().hj_render_aovs_frame_followed(self._h, width, height, int(spp), int(master_seed), begin, end, follow, flags, ptr))
            else:
                self._check(lib().hj_render_aovs_frame(self._h, width, height, int(spp), int(master_seed), begin, end, flags, ptr))
        return aov

    def render_probe_lit(self, volume, origin, spacing, width, height, atlas=None, placement=None, normal_bias=0.0, backface=True, chebyshev=True,
                         blocks=None, spp=None, master_seed=0, passes=None, follow=0, device=None):
        """hj_render_probe_lit / hj_render_probe_lit_frame: the frame a probe volume is for -> (height, width, 4) float32: per pixel
        the float32 sums, in block order, of its samples' radiance L and the sample count - `resolve_probe_lit` gives the mean.  The
        samples and their chains through up to `follow` (0 ... abi.AOV_MAX_FOLLOW) mirrors and glass surfaces are `render_aovs(...,
        follow=)`'s; a chain's last hit gets L = emission + albedo * E / pi with E the look-up of the (nz, ny, nx, 28) `volume` at the
        hit point under the hit's shading normal: `sample_probes` without an atlas, `sample_probes_visible` with one (normal_bias,
        backface, chebyshev as there), its placed form with a `placement`.  A chain the cap cuts on a mirror or on glass gives 0, a
        miss the uploaded environment's radiance or 0.  blocks, or spp [, master_seed, passes], as in `render_aovs`.  numpy arrays give a
        numpy array; contiguous float32 torch tensors on the renderer's GPU (volume, atlas and placement alike; device=None decides by
        the volume's type) are read in place and give a tensor on that GPU; torch's current stream is synchronised first.  Needs no
        framebuffer and leaves it alone."""
        return Renderer._render_lit(self, "render_probe_lit", volume, origin, spacing, width, height, atlas, placement, normal_bias, backface, chebyshev, blocks, spp,
                                    master_seed, passes, follow, device)             # (the class's: the argument checks need no renderer)

    def render_direct_lit(self, width, height, volume=None, origin=None, spacing=None, atlas=None, placement=None, normal_bias=0.0, backface=True,
                          chebyshev=True, blocks=None, spp=None, master_seed=0, passes=None, follow=0, device=None):
        """hj_render_direct_lit / hj_render_direct_lit_frame: `render_probe_lit`'s frame with one traced next-event sample at each
        chain's last diffuse hit -> (height, width, 4) float32 sums as there (`resolve_probe_lit` gives the mean).  A sample's radiance
        is `render_probe_lit`'s plus the shade stage's direct term ((albedo * cos) / pi) * (emitted / pdf) of one emitter sample drawn
        from the sample's own seed, counted when its any-hit shadow ray finds nothing: sharp shadows at the cost of one extra round.
        volume=None: direct light alone (origin, spacing, atlas and placement are then not read; device=True gives a tensor).  A
        volume baked with indirect_only=True holds the indirect light alone and the frame has direct light once; with a plain volume
        it has it twice.  Everything else as in `render_probe_lit`."""
        return Renderer._render_lit(self, "render_direct_lit", volume, origin, spacing, width, height, atlas, placement, normal_bias, backface, chebyshev, blocks, spp,
                                    master_seed, passes, follow, device)             # (the class's: the argument checks need no renderer)

    def _render_lit(self, what, volume, origin, spacing, width, height, atlas, placement, normal_bias, backface, chebyshev, blocks, spp, master_seed, passes,
                    follow, device):
        """the two lit frames behind their names: hj_<what> for a block list, hj_<what>_frame for spp [, master_seed, passes]"""
        if (blocks is None) == (spp is None):
            raise ValueError(f"{what}: either blocks or spp is needed")
        follow = int(follow)
        if not 0 <= follow <= abi.AOV_MAX_FOLLOW:
            raise ValueError(f"{what}: follow {follow}: 0 ... {abi.AOV_MAX_FOLLOW}")
        on_gpu = type(volume).__module__.split(".")[0] == "torch" if device is None else bool(device)
        by_blocks, by_frame = getattr(lib(), "hj_" + what), getattr(lib(), "hj_" + what + "_frame")
        width, height = int(width), int(height)
        if volume is None:
            if what != "render_direct_lit":
                raise ValueError(f"{what}: a volume is needed")
            if on_gpu:
                import torch
                image = torch.empty((height, width, abi.PROBE_LIT_WORDS), dtype=torch.float32, device=f"cuda:{self.device}")
                torch.cuda.current_stream(image.device).synchronize()     # (the allocation)
                ptr, flags = image.data_ptr(), abi.AOV_DEVICE_ARRAY
            else:
                image = np.zeros((height, width, abi.PROBE_LIT_WORDS), np.float32)
                ptr, flags = image.ctypes.data, 0
            if blocks is not None:
                if not isinstance(blocks, C.Array):
                    blocks = (abi.ImageBlock * len(blocks))(*blocks)
                self._check(by_blocks(self._h, blocks, len(blocks), width, height, follow, flags, None, ptr))
            else:
                begin, end = (0, int(spp)) if passes is None else (int(passes[0]), int(passes[1]))
                self._check(by_frame(self._h, width, height, int(spp), int(master_seed), begin, end, follow, flags, None, ptr))
            return image
        if volume.ndim != 4 or volume.shape[3] != abi.PROBE_WORDS:
            raise ValueError(f"{what}: a volume of (nz, ny, nx, {abi.PROBE_WORDS}) is needed (got {tuple(volume.shape)})")
        if placement is not None and atlas is None:
            raise ValueError(f"{what}: a placement needs an atlas")
        if atlas is not None and (atlas.ndim != 6 or tuple(atlas.shape[0:3]) != tuple(volume.shape[0:3]) or atlas.shape[3] != atlas.shape[4] or atlas.shape[5] != 2):
            raise ValueError(f"{what}: an atlas of (nz, ny, nx, res + 2, res + 2, 2) on the volume's grid is needed (got {tuple(atlas.shape)})")
        count = (int(volume.shape[2]), int(volume.shape[1]), int(volume.shape[0]))
        d = self._probe_desc(what, origin, spacing, count, device=on_gpu)
        v = None
        if atlas is not None:
            v = self._probe_vis_desc(what, int(atlas.shape[3]) - 2, normal_bias=normal_bias, backface=backface, chebyshev=chebyshev, device=on_gpu)
        place_ptr = None
        if placement is not None:
            _, placement, place_ptr = self._placement(what, placement, d, on_gpu)
        if on_gpu:
            import torch
            for name, t in (("volume", volume),) + ((("atlas", atlas),) if atlas is not None else ()):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"{what}: {name} must be a contiguous float32 tensor on cuda:{self.device}")
            image = torch.empty((height, width, abi.PROBE_LIT_WORDS), dtype=torch.float32, device=volume.device)
            torch.cuda.current_stream(volume.device).synchronize()    # (the allocation and whatever wrote the tensors)
            ptr, flags = image.data_ptr(), abi.AOV_DEVICE_ARRAY
            vol_ptr, atlas_ptr = volume.data_ptr(), atlas.data_ptr() if atlas is not None else None
        else:
            vol = np.ascontiguousarray(volume, np.float32)
            atl = np.ascontiguousarray(atlas, np.float32) if atlas is not None else None
            image = np.zeros((height, width, abi.PROBE_LIT_WORDS), np.float32)
            ptr, flags = image.ctypes.data, 0
            vol_ptr, atlas_ptr = vol.ctypes.data, atl.ctypes.data if atl is not None else None
        lighting = abi.ProbeLighting(C.pointer(d), C.pointer(v) if v is not None else None, vol_ptr, atlas_ptr, place_ptr)
        if blocks is not None:
            if not isinstance(blocks, C.Array):
                blocks = (abi.ImageBlock * len(blocks))(*blocks)
            self._check(by_blocks(self._h, blocks, len(blocks), width, height, follow, flags, C.byref(lighting), ptr))
        else:
            begin, end = (0, int(spp)) if passes is None else (int(passes[0]), int(passes[1]))
            self._check(by_frame(self._h, width, height, int(spp), int(master_seed), begin, end, follow, flags, C.byref(lighting), ptr))
        return image

    def render_motion(self, prev, width, height, device_arrays=None, device=False, follow=0):
        """hj_render_motion: per-pixel motion for `denoise_frame_temporal` -> (height, width, 4) float32: per pixel (sx, sy, zp, id
        bits) - where the surface point the pixel's centre ray sees in the uploaded scene was in the previous image, its distance
        from the previous camera, and the shape - or (0, 0, 0, abi.MOTION_NONE) for a miss or a point behind the previous camera
        (`motion_ids` views word 3).  prev: how the scene stood in the previous frame - a compiled scene, or anything with `.desc`
        (camera, spheres, quads, vertices with the uploaded counts; a NULL array: that kind did not move), as `update_shapes` takes
        it.  The current frame is the scene as uploaded or as the last `update_shapes` left it.  device_arrays: the dict of torch
        tensors `update_shapes` takes, read in place of prev's host arrays (a kind it lacks did not move).  device=True: the result
        is a torch tensor on the renderer's GPU, written in place.  Not followed: a sphere's rotation about its centre, moving
        lights' shadows, and with follow = 0 what a mirror or glass shows.
        follow (0 ... abi.AOV_MAX_FOLLOW): hj_render_motion_followed - a pixel whose centre ray hits a mirror or glass is followed
        through up to that many specular surfaces, as `render_aovs(..., follow=N)` follows it, and its record is the previous
        position of the virtual point a followed guide describes (zp beside the guide's summed depth), word 3 the last hit's shape,
        or abi.MOTION_LEFT where the chain ended in nothing.  Exact for a static planar mirror; a curved one by its tangent plane, a
        refraction passes the displacement on unchanged.  0: hj_render_motion, as ever."""
        follow = int(follow)
        if not 0 <= follow <= abi.AOV_MAX_FOLLOW:
            raise ValueError(f"render_motion: follow {follow}: 0 ... {abi.AOV_MAX_FOLLOW}")
        d = abi.SceneDesc()
        C.memmove(C.byref(d), C.byref(prev.desc), C.sizeof(abi.SceneDesc))
        width, height = int(width), int(height)
        flags = 0
        if device_arrays is not None:
            import torch
            flags |= abi.MOTION_DEVICE_SHAPES
            for name, count, words, rec in (("spheres", d.num_spheres, 4, abi.Sphere), ("quads", d.num_quads, 12, abi.Quad), ("vertices", d.num_vertices, 8, abi.Vertex)):
                t = device_arrays.get(name)
                if t is not None and not (t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == count * words):
                    raise ValueError(f"device_arrays['{name}']: a contiguous float32 tensor of {count} x {words} on GPU {self.device} is needed"
                                     f" (got {tuple(t.shape)} {t.dtype} on {t.device})")
                setattr(d, name, C.cast(C.c_void_p(t.data_ptr() if t is not None and count else None), C.POINTER(rec)))
            torch.cuda.current_stream().synchronize()
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            motion = torch.empty((height, width, abi.MOTION_WORDS), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            ptr, flags = motion.data_ptr(), flags | abi.MOTION_DEVICE_OUT
        else:
            motion = np.zeros((height, width, abi.MOTION_WORDS), np.float32)
            ptr = motion.ctypes.data
        if follow:
            self._check(lib().hj_render_motion_followed(self._h, C.byref(d), width, height, follow, flags, ptr))
        else:
            self._check(lib().hj_render_motion(self._h, C.byref(d), width, height, flags, ptr))
        return motion

    def denoise_frame(self, aov, beauty=None, iterations=5, sigma_normal=0.5, sigma_depth=1.0, sigma_luminance=4.0, sigma_albedo=0.1, device=False):
        """hj_denoise_frame: the variance-guided a-trous filter of SVGF over one frame -> a new (height, width, 4) float32 image: the
        denoised rgb and, in word 3, the filtered variance of the demodulated luminance.  aov: the (height, width, 12) sums of
        `render_aovs` for the same frame.  beauty: (height, width, 4) in the framebuffer's format, (sum w * rgb, sum w) - what
        `read` returns; None: the renderer's own framebuffer, read on the device and left as it is (it must
        be width x height).  The light is divided by the first hit's mean albedo (floored at 1 / 64), filtered by `iterations`
        (0 ... 8) 5 x 5 B3-spline passes at the steps 1, 2, 4, ... with edge stops on normal (`sigma_normal`), depth in units of
        the local depth slope (`sigma_depth`), albedo (`sigma_albedo`) and luminance in standard deviations of a filtered
        per-pixel variance (`sigma_luminance`), and multiplied by the albedo again; a sigma of 0 switches its stop off.  Pixels
        without a hit or without a sample keep their colour, and so do a directly seen emitter's pixels and the pixels within two
        of them (the reach of the framebuffer's reconstruction filter).  The defaults are SVGF's starting points where it has them (depth,
        luminance) and guesses elsewhere: not tuned.  device=True: `aov` (and `beauty`) are contiguous float32 torch tensors on the
        renderer's GPU, read in place; the result is a new tensor there; torch's current stream is synchronised first."""
        iterations = int(iterations)
        sig = [float(sigma_normal), float(sigma_depth), float(sigma_luminance), float(sigma_albedo)]
        if not 0 <= iterations <= abi.DENOISE_MAX_ITERATIONS:
            raise ValueError(f"denoise_frame: {iterations} iterations: 0 ... {abi.DENOISE_MAX_ITERATIONS}")
        for name, v in zip(("sigma_normal", "sigma_depth", "sigma_luminance", "sigma_albedo"), sig):
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"denoise_frame: {name} {v}: finite and >= 0 is needed")
        o = abi.DenoiseOpts(iterations, *sig, abi.DENOISE_DEVICE_ARRAYS if device else 0)
        if device:
            import torch
            for name, t in (("aov", aov), ("beauty", beauty)):
                if t is None and name == "beauty":
                    continue
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"denoise_frame: {name} must be a contiguous float32 tensor on cuda:{self.device}")
            if aov.dim() != 3 or aov.shape[2] != abi.AOV_WORDS or (beauty is not None and tuple(beauty.shape) != (aov.shape[0], aov.shape[1], 4)):
                raise ValueError("denoise_frame: aov (height, width, 12) and beauty (height, width, 4) are needed")
            h, w = int(aov.shape[0]), int(aov.shape[1])
            out = torch.empty((h, w, 4), dtype=torch.float32, device=aov.device)
            torch.cuda.current_stream(aov.device).synchronize()       # (the allocation and whatever wrote the inputs)
            self._check(lib().hj_denoise_frame(self._h, w, h, None if beauty is None else beauty.data_ptr(), aov.data_ptr(), C.byref(o), out.data_ptr()))
            return out
        aov = np.ascontiguousarray(aov, np.float32)
        if beauty is not None:
            beauty = np.ascontiguousarray(beauty, np.float32)
        if aov.ndim != 3 or aov.shape[2] != abi.AOV_WORDS or (beauty is not None and beauty.shape != (aov.shape[0], aov.shape[1], 4)):
            raise ValueError("denoise_frame: aov (height, width, 12) and beauty (height, width, 4) are needed")
        out = np.zeros((aov.shape[0], aov.shape[1], 4), np.float32)
        self._check(lib().hj_denoise_frame(self._h, aov.shape[1], aov.shape[0], None if beauty is None else beauty.ctypes.data, aov.ctypes.data, C.byref(o),
                                           out.ctypes.data))
        return out

    def denoise_frame_temporal(self, aov, camera, prev_camera, history=None, beauty=None, iterations=5, sigma_normal=0.5, sigma_depth=1.0, sigma_luminance=4.0,
                               sigma_albedo=0.1, alpha=0.2, alpha_moments=0.2, depth_tolerance=0.1, normal_cos=0.9, max_history=64, feedback=True, device=False,
                               motion=None):
        """hj_denoise_frame_temporal: `denoise_frame` behind SVGF's temporal accumulation -> (out, history): the (height, width, 4)
        denoised image and the new (height, width, 12) history to pass as `history` with the next frame.  camera: the abi.Camera
        (beauty, aov) were rendered with; prev_camera: the camera of the frame that wrote `history`.  history None: the first frame
        (the output is `denoise_frame`'s).  Each guided pixel's world point - its depth along its camera ray - is projected into the
        previous camera; the history's four bilinear taps there count when their depth is within `depth_tolerance` (relative) of the
        point's distance and their normal within `normal_cos` of the pixel's; the pixel's light and luminance moments are blended
        with what they give, the new frame's weight being max(alpha, 1 / N) for a history of N frames (N capped at `max_history`,
        1 ... 65535).  A history of 4 frames or more gives the filter its temporal variance.  feedback: the first iteration's light
        goes into the history (SVGF's feedback).  A moved shape is met by the two tests alone.  alpha and alpha_moments 0.2 are
        SVGF's; depth_tolerance 0.1, normal_cos 0.9 and max_history 64 are guesses: not tuned.  Everything else as `denoise_frame`;
        device=True: `aov`, `history` and `beauty` are contiguous float32 torch tensors on the renderer's GPU, read in place, and
        both results are new tensors there.  motion: the (height, width, 4) image of `render_motion` for this frame
        (hj_denoise_frame_temporal_motion; a tensor with device=True): the history is read where each pixel's surface point was -
        moved shapes keep theirs -, a record of abi.MOTION_NONE has none, and the two cameras are checked but not used."""
        iterations = int(iterations)
        sig = [float(sigma_normal), float(sigma_depth), float(sigma_luminance), float(sigma_albedo)]
        if not 0 <= iterations <= abi.DENOISE_MAX_ITERATIONS:
            raise ValueError(f"denoise_frame_temporal: {iterations} iterations: 0 ... {abi.DENOISE_MAX_ITERATIONS}")
        for name, v in zip(("sigma_normal", "sigma_depth", "sigma_luminance", "sigma_albedo"), sig):
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"denoise_frame_temporal: {name} {v}: finite and >= 0 is needed")
        o = abi.DenoiseOpts(iterations, *sig, abi.DENOISE_DEVICE_ARRAYS if device else 0)
        t = abi.TemporalOpts(camera, prev_camera, float(alpha), float(alpha_moments), float(depth_tolerance), float(normal_cos), int(max_history),
                             abi.TEMPORAL_FEEDBACK if feedback else 0)
        if device:
            import torch
            for name, x in (("aov", aov), ("beauty", beauty), ("history", history), ("motion", motion)):
                if x is None and name != "aov":
                    continue
                if not (isinstance(x, torch.Tensor) and x.is_cuda and x.device.index == self.device and x.dtype == torch.float32 and x.is_contiguous()):
                    raise ValueError(f"denoise_frame_temporal: {name} must be a contiguous float32 tensor on cuda:{self.device}")
            if (aov.dim() != 3 or aov.shape[2] != abi.AOV_WORDS or (beauty is not None and tuple(beauty.shape) != (aov.shape[0], aov.shape[1], 4))
                    or (history is not None and tuple(history.shape) != (aov.shape[0], aov.shape[1], abi.TEMPORAL_WORDS))
                    or (motion is not None and tuple(motion.shape) != (aov.shape[0], aov.shape[1], abi.MOTION_WORDS))):
                raise ValueError("denoise_frame_temporal: aov (height, width, 12), beauty (height, width, 4), history (height, width, 12) and motion "
                                 "(height, width, 4) are needed")
            h, w = int(aov.shape[0]), int(aov.shape[1])
            out = torch.empty((h, w, 4), dtype=torch.float32, device=aov.device)
            hist = torch.empty((h, w, abi.TEMPORAL_WORDS), dtype=torch.float32, device=aov.device)
            torch.cuda.current_stream(aov.device).synchronize()       # (the allocations and whatever wrote the inputs)
            args = (None if history is None else history.data_ptr(), hist.data_ptr(), out.data_ptr())
            if motion is not None:
                self._check(lib().hj_denoise_frame_temporal_motion(self._h, w, h, None if beauty is None else beauty.data_ptr(), aov.data_ptr(), C.byref(o),
                                                                   C.byref(t), motion.data_ptr(), *args))
            else:
                self._check(lib().hj_denoise_frame_temporal(self._h, w, h, None if beauty is None else beauty.data_ptr(), aov.data_ptr(), C.byref(o), C.byref(t),
                                                            *args))
            return out, hist
        aov = np.ascontiguousarray(aov, np.float32)
        if beauty is not None:
            beauty = np.ascontiguousarray(beauty, np.float32)
        if history is not None:
            history = np.ascontiguousarray(history, np.float32)
        if (aov.ndim != 3 or aov.shape[2] != abi.AOV_WORDS or (beauty is not None and beauty.shape != (aov.shape[0], aov.shape[1], 4))
                or (history is not None and history.shape != (aov.shape[0], aov.shape[1], abi.TEMPORAL_WORDS))
                or (motion is not None and np.shape(motion) != (aov.shape[0], aov.shape[1], abi.MOTION_WORDS))):
            raise ValueError("denoise_frame_temporal: aov (height, width, 12), beauty (height, width, 4), history (height, width, 12) and motion "
                             "(height, width, 4) are needed")
        out = np.zeros((aov.shape[0], aov.shape[1], 4), np.float32)
        hist = np.zeros((aov.shape[0], aov.shape[1], abi.TEMPORAL_WORDS), np.float32)
        args = (None if history is None else history.ctypes.data, hist.ctypes.data, out.ctypes.data)
        if motion is not None:
            motion = np.ascontiguousarray(motion, np.float32)
            self._check(lib().hj_denoise_frame_temporal_motion(self._h, aov.shape[1], aov.shape[0], None if beauty is None else beauty.ctypes.data,
                                                               aov.ctypes.data, C.byref(o), C.byref(t), motion.ctypes.data, *args))
        else:
            self._check(lib().hj_denoise_frame_temporal(self._h, aov.shape[1], aov.shape[0], None if beauty is None else beauty.ctypes.data, aov.ctypes.data,
                                                        C.byref(o), C.byref(t), *args))
        return out, hist

    def trace_paths(self, rays, seeds=None, spp=1, opts=None, stats=False):
        """hj_trace_paths: the path-traced radiance along (n, 8) rays (origin, direction of any length, a uint32 seed as the bits of
        word 6, a reserved word) -> (n, 8) float32 in the layout of `samples`: the float32 sum of the ray's `spp` samples' radiance,
        (float)spp, the first hit's shading normal and t (zeros for a miss).  Sample k of ray i draws from seedRng(seed_i + k).
        seeds: an (n,) uint32 array (int32 tensor) written into column 6 of a COPY of `rays`; the caller's array is never modified.
        opts: max_bounces, rr_start and RENDER_NO_LIGHT_GRID as in a render call.  A float32 numpy array gives a numpy array.  A
        contiguous float32 torch tensor on the renderer's GPU is read in place and gives a tensor on that GPU; torch's current stream
        is synchronised first.  stats=True: returns (samples, statistics dict)."""
        spp = int(spp)
        if not 1 <= spp <= 65536:
            raise ValueError(f"trace_paths: spp {spp} outside [1, 65536]")
        st = abi.RenderStats()
        o = C.byref(opts) if opts is not None else None
        rays, on_gpu = self._path_rays("trace_paths", rays, seeds)
        n = len(rays)
        if on_gpu:
            import torch
            out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
            torch.cuda.current_stream(rays.device).synchronize()      # (the allocations and whatever wrote `rays`)
            self._check(lib().hj_trace_paths(self._h, rays.data_ptr() if n else None, n, spp, o, abi.PATHS_DEVICE_ARRAYS,
                                             out.data_ptr() if n else None, C.byref(st)))
            return (out, stats_dict(st)) if stats else out
        out = np.zeros((n, 8), np.float32)
        self._check(lib().hj_trace_paths(self._h, rays.ctypes.data, n, spp, o, 0, out.ctypes.data, C.byref(st)))
        return (out, stats_dict(st)) if stats else out

    def _path_rays(self, what, rays, seeds):
        """The ray argument of the path queries, checked before any call -> (rays, on_gpu): a contiguous float32 (n, 8) torch tensor
        on the renderer's GPU as it is, or a contiguous float32 numpy array; with `seeds` a copy whose column 6 holds them."""
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not (rays.is_cuda and rays.device.index == self.device and rays.dtype == torch.float32 and rays.is_contiguous()
                    and rays.dim() == 2 and rays.shape[1] == 8):
                raise ValueError(f"{what}: a contiguous float32 tensor of (n, 8) on GPU {self.device} is needed"
                                 f" (got {tuple(rays.shape)} {rays.dtype} on {rays.device})")
            n = rays.shape[0]
            if seeds is not None:
                if not (type(seeds).__module__.split(".")[0] == "torch" and seeds.device == rays.device and seeds.dtype == torch.int32
                        and tuple(seeds.shape) == (n,)):
                    raise ValueError(f"{what}: seeds must be an int32 tensor of ({n},) on GPU {self.device}")
                rays = rays.clone()
                rays.view(torch.int32)[:, 6] = seeds
            return rays, True
        rays = np.asarray(rays)
        if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"{what}: a float32 array of (n, 8) is needed (got {rays.shape} {rays.dtype})")
        if seeds is not None:
            seeds = np.asarray(seeds)
            if seeds.dtype != np.uint32 or seeds.shape != (len(rays),):
                raise ValueError(f"{what}: seeds must be a uint32 array of ({len(rays)},) (got {seeds.shape} {seeds.dtype})")
            rays = np.array(rays, np.float32, order="C")              # (a copy)
            rays.view(np.uint32)[:, 6] = seeds
        return np.ascontiguousarray(rays), False

    @staticmethod
    def _adaptive_opts(what, spp_min, spp_step, spp_max, rel_error, floor):
        """The adaptive opts of the adaptive calls, checked before any call."""
        spp_min, spp_step, spp_max, rel_error, floor = int(spp_min), int(spp_step), int(spp_max), float(rel_error), float(floor)
        if not (2 <= spp_min <= spp_max <= 65536 and spp_step >= 1):
            raise ValueError(f"{what}: 2 <= spp_min <= spp_max <= 65536 and spp_step >= 1 are needed (got {spp_min}, {spp_max}, {spp_step})")
        if 1 + -(-(spp_max - spp_min) // spp_step) > 64:
            raise ValueError(f"{what}: more than 64 rounds from {spp_min} to {spp_max} in steps of {spp_step}")
        if not (0.0 <= rel_error < float("inf") and 0.0 <= floor < float("inf")):
            raise ValueError(f"{what}: rel_error and floor must be finite and >= 0 (got {rel_error}, {floor})")
        return abi.AdaptiveOpts(spp_min, spp_step, spp_max, rel_error, floor)

    def trace_paths_adaptive(self, rays, seeds=None, spp_min=4, spp_step=4, spp_max=64, rel_error=0.05, floor=0.01, opts=None, stats=False,
                             moments=False):
        """hj_trace_paths_adaptive: `trace_paths` with the number of samples decided per ray on the device.  Every ray gets spp_min
        samples, then spp_step more a round (never more than spp_max in all) until the standard error of its mean luminance is at
        most rel_error * max(mean luminance, floor) - include/hijiki_hip.h spells the rule out.  -> (n, 8) float32 records as
        `trace_paths` gives them, word 3 = the samples the ray received: record i is what `trace_paths` returns for ray i with that
        spp.  rays, seeds, opts and the array / tensor handling are `trace_paths`'.  moments=True: also an (n, 4) float32 array
        (tensor) of S1, S2 (the sums of the samples' luminance and of its square), the last sem2 and the sample count as uint32 bits.
        stats=True: also the statistics dict (bounce_rounds = rounds run).  Returns samples [, moments] [, statistics]."""
        a = self._adaptive_opts("trace_paths_adaptive", spp_min, spp_step, spp_max, rel_error, floor)
        st = abi.RenderStats()
        o = C.byref(opts) if opts is not None else None
        rays, on_gpu = self._path_rays("trace_paths_adaptive", rays, seeds)
        n = len(rays)
        if on_gpu:
            import torch
            out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
            mom = torch.empty((n, 4), dtype=torch.float32, device=rays.device) if moments else None
            torch.cuda.current_stream(rays.device).synchronize()      # (the allocations and whatever wrote `rays`)
            self._check(lib().hj_trace_paths_adaptive(self._h, rays.data_ptr() if n else None, n, C.byref(a), o, abi.PATHS_DEVICE_ARRAYS,
                                                      out.data_ptr() if n else None, mom.data_ptr() if moments and n else None, C.byref(st)))
        else:
            out = np.zeros((n, 8), np.float32)
            mom = np.zeros((n, 4), np.float32) if moments else None
            self._check(lib().hj_trace_paths_adaptive(self._h, rays.ctypes.data, n, C.byref(a), o, 0, out.ctypes.data,
                                                      mom.ctypes.data if moments else None, C.byref(st)))
        res = (out,) + ((mom,) if moments else ()) + ((stats_dict(st),) if stats else ())
        return res if len(res) > 1 else out

    def trace_irradiance(self, points, seeds=None, spp=1, sphere=False, sh9=False, opts=None, stats=None, indirect=False):
        """hj_trace_irradiance: the radiance gathered at (n, 8) points (position, normal of any length - used as given -, a uint32
        seed as the bits of word 6, a reserved word).  Sample k of point i draws its direction on the device from seedRng(seed_i + k):
        cosine-weighted about the normal, or with sphere=True uniform over the sphere (the normal is ignored), and the path goes on
        from there as a sample of `trace_paths` does.  -> (n, 8) float32: the float32 sum of the `spp` samples' radiance, (float)spp,
        the number of samples whose first segment hit something, the nearest such hit's t (+inf if none), two zeros - irradiance is
        pi / spp x words 0..2, ambient occlusion word 4 / spp.  sh9=True (only with sphere=True): (n, 36), behind those eight words the
        sums of Y_j(direction) * radiance for the nine real spherical harmonics of bands 0..2 (word 8 + 3 j + c), word 35 zero.
        seeds, opts and the array / tensor handling are `trace_paths'`: a numpy array gives a numpy array; a contiguous float32 torch
        tensor on the renderer's GPU is read in place and gives a tensor on that GPU, torch's current stream synchronised first.
        With host arrays in hemisphere mode a normal that is not finite or all zero is refused; with tensors that is the caller's
        contract.  stats: true returns (records, statistics dict).  indirect=True (abi.GATHER_INDIRECT): a path starts with
        wasDiscrete clear, so a first segment that ends on an emitter or leaves into the environment adds nothing - the light that
        reaches the point directly is left out; everything else of a path and of a record is unchanged."""
        spp = int(spp)
        if not 1 <= spp <= 65536:
            raise ValueError(f"trace_irradiance: spp {spp} outside [1, 65536]")
        if sh9 and not sphere:
            raise ValueError("trace_irradiance: sh9 needs sphere=True (the basis is integrated over the whole sphere)")
        flags = (abi.GATHER_SPHERE if sphere else 0) | (abi.GATHER_SH9 if sh9 else 0) | (abi.GATHER_INDIRECT if indirect else 0)
        words = 36 if sh9 else 8
        st = abi.RenderStats()
        o = C.byref(opts) if opts is not None else None
        points, on_gpu = self._path_rays("trace_irradiance", points, seeds)
        n = len(points)
        if on_gpu:
            import torch
            out = torch.empty((n, words), dtype=torch.float32, device=points.device)
            torch.cuda.current_stream(points.device).synchronize()    # (the allocations and whatever wrote `points`)
            self._check(lib().hj_trace_irradiance(self._h, points.data_ptr() if n else None, n, spp, o, flags | abi.GATHER_DEVICE_ARRAYS,
                                                  out.data_ptr() if n else None, C.byref(st)))
            return (out, stats_dict(st)) if stats else out
        if not sphere:
            nm = points[:, 3:6]
            bad = ~np.isfinite(nm).all(axis=1) | (nm == 0).all(axis=1)
            if bad.any():
                i = int(np.argmax(bad))
                raise ValueError(f"trace_irradiance: point {i} has the normal {nm[i].tolist()}: finite and not all zero is needed")
        out = np.zeros((n, words), np.float32)
        self._check(lib().hj_trace_irradiance(self._h, points.ctypes.data, n, spp, o, flags, out.ctypes.data, C.byref(st)))
        return (out, stats_dict(st)) if stats else out

    def trace_irradiance_adaptive(self, points, seeds=None, spp_min=4, spp_step=4, spp_max=64, rel_error=0.05, floor=0.01, sphere=False, opts=None,
                                  stats=False, moments=False, indirect=False):
        """hj_trace_irradiance_adaptive: `trace_irradiance` with the number of samples decided per point on the device, by the rounds
        and the stop rule of `trace_paths_adaptive` (spp_min samples, then spp_step more a round up to spp_max, until the standard
        error of the mean luminance is at most rel_error * max(mean luminance, floor)).  -> (n, 8) float32 records as
        `trace_irradiance` gives them, word 3 = the samples the point received: record i is what `trace_irradiance` returns for point
        i with that spp.  There is no sh9.  points, seeds, sphere, opts, the normal check of host arrays and the array / tensor
        handling are `trace_irradiance`'s; moments and stats are `trace_paths_adaptive`'s; indirect as there.  Returns records [, moments]
        [, statistics]."""
        a = self._adaptive_opts("trace_irradiance_adaptive", spp_min, spp_step, spp_max, rel_error, floor)
        flags = (abi.GATHER_SPHERE if sphere else 0) | (abi.GATHER_INDIRECT if indirect else 0)
        st = abi.RenderStats()
        o = C.byref(opts) if opts is not None else None
        points, on_gpu = self._path_rays("trace_irradiance_adaptive", points, seeds)
        n = len(points)
        if on_gpu:
            import torch
            out = torch.empty((n, 8), dtype=torch.float32, device=points.device)
            mom = torch.empty((n, 4), dtype=torch.float32, device=points.device) if moments else None
            torch.cuda.current_stream(points.device).synchronize()    # (the allocations and whatever wrote `points`)
            self._check(lib().hj_trace_irradiance_adaptive(self._h, points.data_ptr() if n else None, n, C.byref(a), o, flags | abi.GATHER_DEVICE_ARRAYS,
                                                           out.data_ptr() if n else None, mom.data_ptr() if moments and n else None, C.byref(st)))
        else:
            if not sphere:
                nm = points[:, 3:6]
                bad = ~np.isfinite(nm).all(axis=1) | (nm == 0).all(axis=1)
                if bad.any():
                    i = int(np.argmax(bad))
                    raise ValueError(f"trace_irradiance_adaptive: point {i} has the normal {nm[i].tolist()}: finite and not all zero is needed")
            out = np.zeros((n, 8), np.float32)
            mom = np.zeros((n, 4), np.float32) if moments else None
            self._check(lib().hj_trace_irradiance_adaptive(self._h, points.ctypes.data, n, C.byref(a), o, flags, out.ctypes.data,
                                                           mom.ctypes.data if moments else None, C.byref(st)))
        res = (out,) + ((mom,) if moments else ()) + ((stats_dict(st),) if stats else ())
        return res if len(res) > 1 else out

    @staticmethod
    def _lightmap_desc(what, width, height, first_triangle, num_triangles, seed, seed_stride, offset, device):
        """The desc of the light-map calls, checked before any call."""
        width, height = int(width), int(height)
        if not (1 <= width <= 16384 and 1 <= height <= 16384 and width * height <= 1 << 26):
            raise ValueError(f"{what}: atlas {width} x {height}: 1 ... 16384 each and at most 2^26 texels")
        offset = float(offset)
        if not np.isfinite(np.float32(offset)):
            raise ValueError(f"{what}: offset {offset} is not finite")
        for name, v in (("first_triangle", first_triangle), ("num_triangles", num_triangles), ("seed", seed), ("seed_stride", seed_stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{what}: {name} {v} is no uint32")
        return abi.LightmapDesc(width, height, int(first_triangle), int(num_triangles), int(seed), int(seed_stride), offset,
                                abi.LIGHTMAP_DEVICE_ARRAYS if device else 0)

    def lightmap_texels(self, width, height, first_triangle=0, num_triangles=0, seed=0, seed_stride=1, offset=0.0, owner=False, device=False):
        """hj_lightmap_texels: the uploaded scene's triangle UVs rasterised into a width x height atlas -> (count, 8) float32 points, one
        per texel that a triangle of [first_triangle, first_triangle + num_triangles) owns (0: all from first_triangle on), in ascending
        texel index t = y * width + x: position (moved by normal * offset), normal, the seed seed + t * seed_stride as the bits of
        word 6, t as the bits of word 7 - a `points` argument of `trace_irradiance` as it stands.  include/hijiki_hip.h spells the
        coverage rule out.  owner=True: also the (height, width) uint32 owner map (abi.LIGHTMAP_NONE: no owner).  device=True: torch
        tensors on the renderer's GPU, written in place on the device; torch's current stream is synchronised first."""
        d = self._lightmap_desc("lightmap_texels", width, height, first_triangle, num_triangles, seed, seed_stride, offset, device)
        count = C.c_size_t(0)
        self._check(lib().hj_lightmap_texels(self._h, C.byref(d), None, 0, None, C.byref(count)))
        n = count.value
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            pts = torch.empty((n, 8), dtype=torch.float32, device=dev)
            own = torch.empty((d.height, d.width), dtype=torch.int32, device=dev) if owner else None
            torch.cuda.current_stream(dev).synchronize()              # (the allocations)
            self._check(lib().hj_lightmap_texels(self._h, C.byref(d), pts.data_ptr() if n else None, n, own.data_ptr() if owner else None,
                                                 C.byref(count)))
            return (pts, own) if owner else pts
        pts = np.zeros((n, 8), np.float32)
        own = np.zeros((d.height, d.width), np.uint32) if owner else None
        if n or owner:
            self._check(lib().hj_lightmap_texels(self._h, C.byref(d), pts.ctypes.data if n else None, n, own.ctypes.data if owner else None,
                                                 C.byref(count)))
        return (pts, own) if owner else pts

    @staticmethod
    def _lightmap_filter(what, iterations, sigma_position, sigma_normal, sigma_color, device):
        """The filter of the light-map calls, checked before any call."""
        iterations = int(iterations)
        if not 0 <= iterations <= abi.LIGHTMAP_FILTER_MAX_ITERATIONS:
            raise ValueError(f"{what}: {iterations} filter iterations outside [0, {abi.LIGHTMAP_FILTER_MAX_ITERATIONS}]")
        for name, v in (("sigma_position", sigma_position), ("sigma_normal", sigma_normal), ("sigma_color", sigma_color)):
            v = np.float32(v)
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"{what}: {name} {v}: finite and >= 0 is needed")
        return abi.LightmapFilter(iterations, float(sigma_position), float(sigma_normal), float(sigma_color), abi.LIGHTMAP_DEVICE_ARRAYS if device else 0)

    def filter_lightmap(self, image, points, iterations, sigma_position, sigma_normal, sigma_color=0.0, device=False):
        """hj_filter_lightmap: `iterations` (0 ... 8) iterations of an edge-avoiding a-trous filter over the (height, width, 4) float32
        atlas `image`, guided by the (count, 8) `points` of `lightmap_texels` over the same atlas (position, normal, the texel index
        in word 7, strictly ascending): a 5 x 5 B3-spline kernel at the steps 1, 2, 4, ..., each tap weighted down by its distance in
        world position (`sigma_position`, world units), normal (`sigma_normal`) and colour (`sigma_color`, halved every
        iteration); a sigma of 0 switches its stop off.  Texels no point names are left as they are; alpha is kept.  -> a new
        (height, width, 4) array.  device=True: `image` and `points` are contiguous float32 torch tensors on the renderer's GPU, the
        points' indices the caller's contract (a point that names no texel is skipped); `image` is filtered IN PLACE and returned;
        torch's current stream is synchronised first."""
        f = self._lightmap_filter("filter_lightmap", iterations, sigma_position, sigma_normal, sigma_color, device)
        if device:
            import torch
            for name, t in (("image", image), ("points", points)):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"filter_lightmap: {name} must be a contiguous float32 tensor on cuda:{self.device}")
            if image.dim() != 3 or image.shape[2] != 4 or points.dim() != 2 or points.shape[1] != 8:
                raise ValueError("filter_lightmap: image (height, width, 4) and points (count, 8) are needed")
            h, w, n = int(image.shape[0]), int(image.shape[1]), int(points.shape[0])
            torch.cuda.current_stream(image.device).synchronize()     # (whatever wrote the tensors)
            self._check(lib().hj_filter_lightmap(self._h, w, h, points.data_ptr() if n else None, n, C.byref(f), image.data_ptr()))
            return image
        img = np.array(image, np.float32, order="C")                     # (a copy: the caller's array is left alone)
        pts = np.ascontiguousarray(points, np.float32)
        if img.ndim != 3 or img.shape[2] != 4 or pts.ndim != 2 or pts.shape[1] != 8:
            raise ValueError("filter_lightmap: image (height, width, 4) and points (count, 8) are needed")
        self._check(lib().hj_filter_lightmap(self._h, img.shape[1], img.shape[0], pts.ctypes.data if len(pts) else None, len(pts), C.byref(f),
                                             img.ctypes.data))
        return img

    def bake_lightmap(self, width, height, spp, gutter=2, first_triangle=0, num_triangles=0, seed=0, seed_stride=1, offset=0.0, opts=None,
                      stats=False, device=False, filter=None, adaptive=None, sample_map=False):
        """hj_bake_lightmap: `lightmap_texels`, the hemisphere gather of `trace_irradiance` at `spp` samples over its points, and the
        records scattered into the atlas, all on the device -> (height, width, 4) float32: a texel with a record holds its irradiance
        (pi / spp x the gathered sum) and alpha 1; `gutter` dilation passes give texels next to covered ones the mean of their covered
        neighbours and alpha 0.5; everything else is zero.  opts as in `trace_irradiance`.  device=True: a torch tensor on the
        renderer's GPU.  stats=True: returns (image, the gather's statistics dict with `texels` = the texels that had a record).
        filter: None, or (iterations, sigma_position, sigma_normal[, sigma_color]) - `filter_lightmap` over the scattered image with the
        bake's own points as guides, before the dilation (hj_bake_lightmap_filtered); `default_filter_sigmas` gives a starting point.
        adaptive: None, or a dict with the keywords of `trace_irradiance_adaptive` (spp_min, spp_step, spp_max, rel_error, floor; its
        defaults for those left out) - hj_bake_lightmap_adaptive: the gather decides each texel's sample count, `spp` is not used (pass
        None), a texel's scale is pi / its own count, and `bounce_rounds` of the statistics is the rounds run.  sample_map=True (only
        with adaptive): also the (height, width) uint32 map (an int32 tensor with device=True) of the samples each texel with a record
        received, 0 elsewhere.  Returns image [, sample map] [, statistics]."""
        if adaptive is not None:
            return self._bake_lightmap_adaptive(width, height, adaptive, int(gutter), first_triangle, num_triangles, seed, seed_stride, offset, opts,
                                                stats, device, filter, sample_map)
        if sample_map:
            raise ValueError("bake_lightmap: sample_map needs adaptive (a fixed-spp bake gives every texel spp samples)")
        spp, gutter = int(spp), int(gutter)
        if not 1 <= spp <= 65536:
            raise ValueError(f"bake_lightmap: spp {spp} outside [1, 65536]")
        if not 0 <= gutter <= abi.LIGHTMAP_MAX_GUTTER:
            raise ValueError(f"bake_lightmap: gutter {gutter} outside [0, {abi.LIGHTMAP_MAX_GUTTER}]")
        d = self._lightmap_desc("bake_lightmap", width, height, first_triangle, num_triangles, seed, seed_stride, offset, device)
        st, count = abi.RenderStats(), C.c_size_t(0)
        o = C.byref(opts) if opts is not None else None
        if filter is None:
            call = lambda p: lib().hj_bake_lightmap(self._h, C.byref(d), spp, gutter, o, p, C.byref(count), C.byref(st))  # noqa: E731
        else:
            if not 2 <= len(filter) - 1 <= 3:
                raise ValueError("bake_lightmap: filter is (iterations, sigma_position, sigma_normal[, sigma_color])")
            f = self._lightmap_filter("bake_lightmap", filter[0], filter[1], filter[2], filter[3] if len(filter) > 3 else 0.0, False)
            call = lambda p: lib().hj_bake_lightmap_filtered(self._h, C.byref(d), spp, gutter, C.byref(f), o, p, C.byref(count), C.byref(st))  # noqa: E731
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            img = torch.empty((d.height, d.width, 4), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            self._check(call(img.data_ptr()))
        else:
            img = np.zeros((d.height, d.width, 4), np.float32)
            self._check(call(img.ctypes.data))
        return (img, dict(stats_dict(st), texels=count.value)) if stats else img

    def _bake_lightmap_adaptive(self, width, height, adaptive, gutter, first_triangle, num_triangles, seed, seed_stride, offset, opts, stats, device,
                                filter, sample_map):
        """`bake_lightmap` with adaptive=dict: hj_bake_lightmap_adaptive."""
        unknown = set(adaptive) - {"spp_min", "spp_step", "spp_max", "rel_error", "floor"}
        if unknown:
            raise ValueError(f"bake_lightmap: adaptive has the unknown keys {sorted(unknown)}")
        kw = dict(dict(spp_min=4, spp_step=4, spp_max=64, rel_error=0.05, floor=0.01), **adaptive)
        a = self._adaptive_opts("bake_lightmap", kw["spp_min"], kw["spp_step"], kw["spp_max"], kw["rel_error"], kw["floor"])
        if not 0 <= gutter <= abi.LIGHTMAP_MAX_GUTTER:
            raise ValueError(f"bake_lightmap: gutter {gutter} outside [0, {abi.LIGHTMAP_MAX_GUTTER}]")
        d = self._lightmap_desc("bake_lightmap", width, height, first_triangle, num_triangles, seed, seed_stride, offset, device)
        st, count = abi.RenderStats(), C.c_size_t(0)
        o = C.byref(opts) if opts is not None else None
        f = None
        if filter is not None:
            if not 2 <= len(filter) - 1 <= 3:
                raise ValueError("bake_lightmap: filter is (iterations, sigma_position, sigma_normal[, sigma_color])")
            f = C.byref(self._lightmap_filter("bake_lightmap", filter[0], filter[1], filter[2], filter[3] if len(filter) > 3 else 0.0, False))
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            img = torch.empty((d.height, d.width, 4), dtype=torch.float32, device=dev)
            smap = torch.empty((d.height, d.width), dtype=torch.int32, device=dev) if sample_map else None
            torch.cuda.current_stream(dev).synchronize()              # (the allocations)
            self._check(lib().hj_bake_lightmap_adaptive(self._h, C.byref(d), C.byref(a), gutter, f, o, img.data_ptr(),
                                                        smap.data_ptr() if sample_map else None, C.byref(count), C.byref(st)))
        else:
            img = np.zeros((d.height, d.width, 4), np.float32)
            smap = np.zeros((d.height, d.width), np.uint32) if sample_map else None
            self._check(lib().hj_bake_lightmap_adaptive(self._h, C.byref(d), C.byref(a), gutter, f, o, img.ctypes.data,
                                                        smap.ctypes.data if sample_map else None, C.byref(count), C.byref(st)))
        res = (img,) + ((smap,) if sample_map else ()) + ((dict(stats_dict(st), texels=count.value),) if stats else ())
        return res if len(res) > 1 else img

    @staticmethod
    def _probe_desc(what, origin, spacing, count, seed=0, seed_stride=1, min_distance=0.0, device=False, indirect_only=False):
        """The desc of the probe calls, checked before any call.  count is (nx, ny, nz), as origin and spacing are (x, y, z).
        indirect_only: abi.PROBES_INDIRECT_ONLY, which the calls that gather read and every other call ignores."""
        origin, spacing = np.asarray(origin, np.float32).reshape(-1), np.asarray(spacing, np.float32).reshape(-1)
        count = [int(c) for c in count]
        if len(origin) != 3 or len(spacing) != 3 or len(count) != 3:
            raise ValueError(f"{what}: origin, spacing and count have three components each")
        if not (all(1 <= c <= abi.PROBE_MAX_COUNT for c in count) and count[0] * count[1] * count[2] <= abi.PROBE_MAX_PROBES):
            raise ValueError(f"{what}: count {count}: 1 ... {abi.PROBE_MAX_COUNT} each and at most 2^22 probes")
        if not np.isfinite(origin).all():
            raise ValueError(f"{what}: origin {origin.tolist()} is not finite")
        if not (np.isfinite(spacing).all() and (spacing > 0).all()):
            raise ValueError(f"{what}: spacing {spacing.tolist()}: finite and > 0 is needed")
        min_distance = np.float32(min_distance)
        if not (np.isfinite(min_distance) and min_distance >= 0):
            raise ValueError(f"{what}: min_distance {min_distance}: finite and >= 0 is needed")
        for name, v in (("seed", seed), ("seed_stride", seed_stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{what}: {name} {v} is no uint32")
        f3, u3 = C.c_float * 3, C.c_uint32 * 3
        return abi.ProbeDesc(f3(*origin.tolist()), f3(*spacing.tolist()), u3(*count), int(seed), int(seed_stride), float(min_distance),
                             (abi.PROBES_DEVICE_ARRAYS if device else 0) | (abi.PROBES_INDIRECT_ONLY if indirect_only else 0))

    def probe_points(self, origin, spacing, count, seed=0, seed_stride=1, device=False):
        """hj_probe_points: the gather points of a grid of count = (nx, ny, nz) probes, probe (x, y, z) at origin + (x, y, z) * spacing
        -> (nx * ny * nz, 8) float32 in ascending p = (z * ny + y) * nx + x: position, a zero normal, the seed seed + p * seed_stride
        as the bits of word 6, p as the bits of word 7 - a `points` argument of `trace_irradiance(sphere=True)` as it stands.  No
        scene is needed.  device=True: a torch tensor on the renderer's GPU, written in place on the device; torch's current stream is
        synchronised first."""
        d = self._probe_desc("probe_points", origin, spacing, count, seed, seed_stride, 0.0, device)
        n = d.count[0] * d.count[1] * d.count[2]
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            pts = torch.empty((n, 8), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            self._check(lib().hj_probe_points(self._h, C.byref(d), pts.data_ptr()))
            return pts
        pts = np.zeros((n, 8), np.float32)
        self._check(lib().hj_probe_points(self._h, C.byref(d), pts.ctypes.data))
        return pts

    def bake_probes(self, origin, spacing, count, spp, min_distance=0.0, seed=0, seed_stride=1, opts=None, stats=False, device=False, indirect_only=False):
        """hj_bake_probes: an irradiance probe volume of the uploaded scene, baked on the device - `probe_points`, the sphere gather of
        `trace_irradiance(sphere=True, sh9=True)` at `spp` samples over them, and the SH sums resolved to irradiance coefficients
        -> (nz, ny, nx, 28) float32: word 3 j + c of a probe is the coefficient of the j-th real spherical harmonic (bands 0..2, the
        gather's order) of the irradiance as a function of the surface normal, channel c; word 27 is 1 when no gather ray hit
        anything nearer than `min_distance`, else 0 (a probe inside or against a wall).  opts as in `trace_irradiance`.  device=True: a
        torch tensor on the renderer's GPU.  stats=True: returns (volume, the gather's statistics dict).  `sample_probes` reads it.
        indirect_only=True (abi.PROBES_INDIRECT_ONLY): the gather is `trace_irradiance(..., indirect=True)` - the volume holds no light
        that reaches a probe directly, which is what `render_direct_lit` adds by tracing."""
        spp = int(spp)
        if not 1 <= spp <= 65536:
            raise ValueError(f"bake_probes: spp {spp} outside [1, 65536]")
        d = self._probe_desc("bake_probes", origin, spacing, count, seed, seed_stride, min_distance, device, indirect_only)
        shape = (d.count[2], d.count[1], d.count[0], abi.PROBE_WORDS)
        st = abi.RenderStats()
        o = C.byref(opts) if opts is not None else None
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            vol = torch.empty(shape, dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            self._check(lib().hj_bake_probes(self._h, C.byref(d), spp, o, vol.data_ptr(), C.byref(st)))
        else:
            vol = np.zeros(shape, np.float32)
            self._check(lib().hj_bake_probes(self._h, C.byref(d), spp, o, vol.ctypes.data, C.byref(st)))
        return (vol, stats_dict(st)) if stats else vol

    def sample_probes(self, volume, origin, spacing, points, normals=None, device=None):
        """hj_sample_probes: the irradiance at points from a (nz, ny, nx, 28) probe volume (`bake_probes`; count comes from its shape)
        whose probe (0, 0, 0) sits at `origin`, `spacing` apart -> (n, 4) float32: the irradiance (r, g, b) on a surface with the
        point's normal, trilinearly interpolated between the eight probes around the position with each probe's validity as a further
        weight, and that weight sum (0, and a black result, where no valid probe stands near).  Positions outside the volume take the
        nearest face's value.  points: (n, 8) in the gather's layout (position, normal of any length but zero, two ignored words), or
        (n, 3) positions with `normals` (n, 3).  numpy arrays give a numpy array: positions and normals must be finite.  Contiguous
        float32 torch tensors on the renderer's GPU (volume and points alike; device=None decides by the volume's type) are read in
        place and give a tensor on that GPU - there nothing in `points` can make the call fault, a NaN just propagates; torch's
        current stream is synchronised first.  No scene is needed."""
        on_gpu = type(volume).__module__.split(".")[0] == "torch" if device is None else bool(device)
        if volume.ndim != 4 or volume.shape[3] != abi.PROBE_WORDS:
            raise ValueError(f"sample_probes: a volume of (nz, ny, nx, {abi.PROBE_WORDS}) is needed (got {tuple(volume.shape)})")
        count = (int(volume.shape[2]), int(volume.shape[1]), int(volume.shape[0]))
        d = self._probe_desc("sample_probes", origin, spacing, count, device=on_gpu)
        if normals is not None:
            if points.ndim != 2 or points.shape[1] != 3 or tuple(normals.shape) != tuple(points.shape):
                raise ValueError("sample_probes: with normals, points and normals are (n, 3) each")
        elif points.ndim != 2 or points.shape[1] != 8:
            raise ValueError(f"sample_probes: points of (n, 8), or (n, 3) with normals, are needed (got {tuple(points.shape)})")
        if on_gpu:
            import torch
            for name, t in (("volume", volume), ("points", points)) + ((("normals", normals),) if normals is not None else ()):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"sample_probes: {name} must be a contiguous float32 tensor on cuda:{self.device}")
            if normals is not None:
                points = torch.cat([points, normals, torch.zeros((points.shape[0], 2), dtype=torch.float32, device=points.device)], 1)
            n = int(points.shape[0])
            out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
            torch.cuda.current_stream(points.device).synchronize()    # (the allocations and whatever wrote the tensors)
            self._check(lib().hj_sample_probes(self._h, C.byref(d), volume.data_ptr(), points.data_ptr() if n else None, n,
                                               out.data_ptr() if n else None))
            return out
        vol = np.ascontiguousarray(volume, np.float32)
        if normals is not None:
            points = np.concatenate([np.asarray(points, np.float32), np.asarray(normals, np.float32), np.zeros((len(points), 2), np.float32)], 1)
        pts = np.ascontiguousarray(points, np.float32)
        bad = ~np.isfinite(pts[:, 0:6]).all(axis=1) | (pts[:, 3:6] == 0).all(axis=1)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"sample_probes: point {i} ({pts[i, 0:6].tolist()}): finite positions and finite normals that are not all zero are needed")
        out = np.zeros((len(pts), 4), np.float32)
        self._check(lib().hj_sample_probes(self._h, C.byref(d), vol.ctypes.data, pts.ctypes.data, len(pts), out.ctypes.data))
        return out

    @staticmethod
    def _probe_vis_desc(what, res, rays_per_texel=1, max_distance=1.0, normal_bias=0.0, backface=True, chebyshev=True, device=False):
        """The hj_probe_vis_desc of the visibility calls, checked before any call."""
        res, rays_per_texel = int(res), int(rays_per_texel)
        if res not in abi.PROBE_VIS_RES:
            raise ValueError(f"{what}: res {res}: one of {abi.PROBE_VIS_RES} is needed")
        if not 1 <= rays_per_texel <= abi.PROBE_VIS_MAX_RAYS_PER_TEXEL:
            raise ValueError(f"{what}: rays_per_texel {rays_per_texel} outside [1, {abi.PROBE_VIS_MAX_RAYS_PER_TEXEL}]")
        max_distance, normal_bias = np.float32(max_distance), np.float32(normal_bias)
        if not (np.isfinite(max_distance) and 0 < max_distance <= np.float32(abi.PROBE_VIS_MAX_DISTANCE)):
            raise ValueError(f"{what}: max_distance {max_distance}: finite, > 0 and at most 1e18 is needed")
        if not (np.isfinite(normal_bias) and normal_bias >= 0):
            raise ValueError(f"{what}: normal_bias {normal_bias}: finite and >= 0 is needed")
        flags = ((abi.PROBE_VIS_DEVICE_ARRAYS if device else 0) | (0 if backface else abi.PROBE_VIS_NO_BACKFACE)
                 | (0 if chebyshev else abi.PROBE_VIS_NO_CHEBYSHEV))
        return abi.ProbeVisDesc(res, rays_per_texel, float(max_distance), float(normal_bias), flags)

    def probe_visibility_rays(self, origin, spacing, count, res=8, rays_per_texel=4, max_distance=1e18, seed=0, seed_stride=1, first_probe=0,
                              num_probes=None, device=False):
        """hj_probe_visibility_rays: the rays `bake_probe_visibility` traces for the probes first_probe ... first_probe + num_probes - 1
        (None: to the last) of a grid -> (num_probes * res * res * rays_per_texel, 8) float32, probe-major: `trace_rays` records -
        the probe's position, a unit direction drawn inside texel (r // rays_per_texel) % res, (r // rays_per_texel) // res of the
        probe's octahedral map from seedRng(seed + p * seed_stride + r), tMin 0, tMax max_distance.  No scene is needed.
        device=True: a torch tensor on the renderer's GPU, written in place on the device."""
        d = self._probe_desc("probe_visibility_rays", origin, spacing, count, seed, seed_stride, 0.0, device)
        v = self._probe_vis_desc("probe_visibility_rays", res, rays_per_texel, max_distance, device=device)
        n = d.count[0] * d.count[1] * d.count[2]
        first_probe = int(first_probe)
        num_probes = n - first_probe if num_probes is None else int(num_probes)
        if not (0 <= first_probe and 0 <= num_probes and first_probe + num_probes <= n):
            raise ValueError(f"probe_visibility_rays: probes {first_probe} ... {first_probe + num_probes} of {n}")
        rows = num_probes * v.res * v.res * v.rays_per_texel
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            rays = torch.empty((rows, 8), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            self._check(lib().hj_probe_visibility_rays(self._h, C.byref(d), C.byref(v), first_probe, num_probes, rays.data_ptr() if rows else None))
            return rays
        rays = np.zeros((rows, 8), np.float32)
        self._check(lib().hj_probe_visibility_rays(self._h, C.byref(d), C.byref(v), first_probe, num_probes, rays.ctypes.data if rows else None))
        return rays

    def bake_probe_visibility(self, origin, spacing, count, res=8, rays_per_texel=4, max_distance=1e18, seed=0, seed_stride=1, device=False):
        """hj_bake_probe_visibility: the visibility atlas of a grid of probes in the uploaded scene -> (nz, ny, nx, res + 2, res + 2, 2)
        float32: per probe an octahedral map of res x res texels (rows: the map's y) with a one-texel border that holds the map's
        wrap-around, per texel the mean and the mean squared distance to the nearest surface over `rays_per_texel` rays drawn inside
        the texel; a ray that hits nothing within `max_distance` counts as max_distance.  `sample_probes_visible` reads it beside
        the volume of `bake_probes` on the same grid.  device=True: a torch tensor on the renderer's GPU."""
        d = self._probe_desc("bake_probe_visibility", origin, spacing, count, seed, seed_stride, 0.0, device)
        v = self._probe_vis_desc("bake_probe_visibility", res, rays_per_texel, max_distance, device=device)
        shape = (d.count[2], d.count[1], d.count[0], v.res + 2, v.res + 2, 2)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            atlas = torch.empty(shape, dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()              # (the allocation)
            self._check(lib().hj_bake_probe_visibility(self._h, C.byref(d), C.byref(v), atlas.data_ptr()))
            return atlas
        atlas = np.zeros(shape, np.float32)
        self._check(lib().hj_bake_probe_visibility(self._h, C.byref(d), C.byref(v), atlas.ctypes.data))
        return atlas

    def sample_probes_visible(self, volume, atlas, origin, spacing, points, normal_bias=0.0, backface=True, chebyshev=True, normals=None,
                              device=None, placement=None):
        """hj_sample_probes_visible: `sample_probes` with the weights against light leaks -> (n, 4) float32.  Each of the eight probes
        about a point is weighted further by a back-face factor (((dot(direction to the probe, normal) + 1) / 2)^2 + 0.2: probes
        behind the surface count less) and by Chebyshev's bound, cubed and at least 0.05, on the share of the probe's rays that reach
        as far as the point moved `normal_bias` along its normal, from the two moments `atlas` (`bake_probe_visibility` on the same
        grid: (nz, ny, nx, res + 2, res + 2, 2); res comes from its shape) holds in the point's direction.  backface=False /
        chebyshev=False switch a factor off; with both off atlas may be None and the result is `sample_probes`'.  volume, points,
        normals and the numpy / torch rules as in `sample_probes`.  placement (None: the grid as it is): the (nz, ny, nx, 4) array of
        `place_probes`, of the volume's kind - hj_sample_probes_visible_placed: both factors see a probe where its offset put it, and
        an inactive probe counts nothing."""
        on_gpu = type(volume).__module__.split(".")[0] == "torch" if device is None else bool(device)
        if volume.ndim != 4 or volume.shape[3] != abi.PROBE_WORDS:
            raise ValueError(f"sample_probes_visible: a volume of (nz, ny, nx, {abi.PROBE_WORDS}) is needed (got {tuple(volume.shape)})")
        count = (int(volume.shape[2]), int(volume.shape[1]), int(volume.shape[0]))
        if atlas is None:
            if backface or chebyshev:
                raise ValueError("sample_probes_visible: an atlas is needed unless backface and chebyshev are both off")
            res = abi.PROBE_VIS_RES[0]
        else:
            if atlas.ndim != 6 or tuple(atlas.shape[0:3]) != tuple(volume.shape[0:3]) or atlas.shape[3] != atlas.shape[4] or atlas.shape[5] != 2:
                raise ValueError(f"sample_probes_visible: an atlas of (nz, ny, nx, res + 2, res + 2, 2) on the volume's grid is needed"
                                 f" (got {tuple(atlas.shape)} beside {tuple(volume.shape)})")
            res = int(atlas.shape[3]) - 2
        d = self._probe_desc("sample_probes_visible", origin, spacing, count, device=on_gpu)
        v = self._probe_vis_desc("sample_probes_visible", res, normal_bias=normal_bias, backface=backface, chebyshev=chebyshev, device=on_gpu)
        if placement is not None:
            _, placement, place_ptr = self._placement("sample_probes_visible", placement, d, on_gpu)
        if normals is not None:
            if points.ndim != 2 or points.shape[1] != 3 or tuple(normals.shape) != tuple(points.shape):
                raise ValueError("sample_probes_visible: with normals, points and normals are (n, 3) each")
        elif points.ndim != 2 or points.shape[1] != 8:
            raise ValueError(f"sample_probes_visible: points of (n, 8), or (n, 3) with normals, are needed (got {tuple(points.shape)})")
        if on_gpu:
            import torch
            for name, t in ((("volume", volume), ("points", points)) + ((("atlas", atlas),) if atlas is not None else ())
                            + ((("normals", normals),) if normals is not None else ())):  # (a placement: checked by _placement)
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                    raise ValueError(f"sample_probes_visible: {name} must be a contiguous float32 tensor on cuda:{self.device}")
            if normals is not None:
                points = torch.cat([points, normals, torch.zeros((points.shape[0], 2), dtype=torch.float32, device=points.device)], 1)
            n = int(points.shape[0])
            out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
            torch.cuda.current_stream(points.device).synchronize()    # (the allocations and whatever wrote the tensors)
            if placement is not None:
                self._check(lib().hj_sample_probes_visible_placed(self._h, C.byref(d), C.byref(v), volume.data_ptr(),
                                                                  atlas.data_ptr() if atlas is not None else None, points.data_ptr() if n else None, n,
                                                                  place_ptr, out.data_ptr() if n else None))
                return out
            self._check(lib().hj_sample_probes_visible(self._h, C.byref(d), C.byref(v), volume.data_ptr(), atlas.data_ptr() if atlas is not None else None,
                                                       points.data_ptr() if n else None, n, out.data_ptr() if n else None))
            return out
        vol = np.ascontiguousarray(volume, np.float32)
        atl = np.ascontiguousarray(atlas, np.float32) if atlas is not None else None
        if normals is not None:
            points = np.concatenate([np.asarray(points, np.float32), np.asarray(normals, np.float32), np.zeros((len(points), 2), np.float32)], 1)
        pts = np.ascontiguousarray(points, np.float32)
        bad = ~np.isfinite(pts[:, 0:6]).all(axis=1) | (pts[:, 3:6] == 0).all(axis=1)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"sample_probes_visible: point {i} ({pts[i, 0:6].tolist()}): finite positions and finite normals that are not all zero are needed")
        out = np.zeros((len(pts), 4), np.float32)
        if placement is not None:
            self._check(lib().hj_sample_probes_visible_placed(self._h, C.byref(d), C.byref(v), vol.ctypes.data, atl.ctypes.data if atl is not None else None,
                                                              pts.ctypes.data, len(pts), place_ptr, out.ctypes.data))
            return out
        self._check(lib().hj_sample_probes_visible(self._h, C.byref(d), C.byref(v), vol.ctypes.data, atl.ctypes.data if atl is not None else None,
                                                   pts.ctypes.data, len(pts), out.ctypes.data))
        return out

    @staticmethod
    def _probe_update(what, n, frame, frame_stride, hysteresis, window, change):
        """The hj_probe_update of the update calls, checked before any call.  window: (first_probe, num_probes), None: all n probes."""
        first, num = (0, n) if window is None else (int(window[0]), int(window[1]))
        if not (0 <= first and 0 <= num and first + num <= n):
            raise ValueError(f"{what}: window {first} ... {first + num} of {n} probes")
        for name, v in (("frame", frame), ("frame_stride", frame_stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{what}: {name} {v} is no uint32")
        h = np.float32(hysteresis)
        if not 0 <= h < 1:
            raise ValueError(f"{what}: hysteresis {hysteresis} outside [0, 1)")
        soft, hard = (np.float32(c) for c in change)
        if not (soft >= 0 and hard >= 0):
            raise ValueError(f"{what}: change {tuple(change)}: two thresholds >= 0 (inf: never) are needed")
        return abi.ProbeUpdate(first, num, int(frame), int(frame_stride), float(h), float(soft), float(hard), 0)

    def _update_target(self, what, array, shape):
        """The array an update call reads and writes: a contiguous float32 torch tensor on the renderer's GPU (updated in place) or a
        numpy array (a contiguous float32 copy is updated and returned) of `shape` -> (on_gpu, the array, its address)"""
        if type(array).__module__.split(".")[0] == "torch":
            if not (array.is_cuda and array.device.index == self.device and str(array.dtype) == "torch.float32" and array.is_contiguous()):
                raise ValueError(f"{what}: a contiguous float32 tensor on cuda:{self.device} is needed")
            if tuple(array.shape) != shape:
                raise ValueError(f"{what}: an array of {shape} is needed (got {tuple(array.shape)})")
            return True, array, array.data_ptr()
        out = np.array(array, np.float32, order="C")
        if out.shape != shape:
            raise ValueError(f"{what}: an array of {shape} is needed (got {out.shape})")
        return False, out, out.ctypes.data

    def update_probes(self, desc, probes, spp, *, frame, frame_stride=abi.PROBE_UPDATE_FRAME_STRIDE, hysteresis, window=None,
                      change=abi.PROBE_UPDATE_CHANGE, opts=None, stats=False, placement=None, indirect_only=False):
        """hj_update_probes: a window of a (nz, ny, nx, 28) probe volume re-baked from the uploaded scene at `spp` samples and folded
        into `probes`.  desc: the grid as a dict of `bake_probes`' keywords (origin, spacing, count, and min_distance, seed,
        seed_stride where they are not the defaults).  The fresh record of a probe is `bake_probes`' with the seed seed + frame *
        frame_stride (uint32 wrap-around): give every update another `frame`.  new = old * hysteresis + fresh * (1 - hysteresis) per
        coefficient; the validity is the fresh one, and a probe that was or becomes invalid takes the fresh coefficients alone.
        change = (soft, hard): where the constant band moved by more than soft (hard) times its old magnitude the hysteresis drops by
        0.15 (to 0); (inf, inf): never.  hysteresis = 0 writes the fresh bake whatever `probes` held, so a first update needs no
        initialised volume.  window = (first_probe, num_probes) in the order p = (z * ny + y) * nx + x, None: the whole volume; probes
        outside it keep every bit.  A contiguous float32 torch tensor on the renderer's GPU is updated in place (torch's current
        stream is synchronised first) and returned; a numpy array gives an updated copy, of which the window alone travelled.
        stats=True: returns (probes, the gather's statistics dict).  placement (None: the grid as it is): the (nz, ny, nx, 4) array of
        `place_probes`, of `probes`' kind - hj_update_probes_placed: the gather points sit at the placed positions, and the window's
        inactive probes are neither traced nor written.  indirect_only=True (or the key in desc): the fresh record is
        `bake_probes(..., indirect_only=True)`'s."""
        spp = int(spp)
        if not 1 <= spp <= 65536:
            raise ValueError(f"update_probes: spp {spp} outside [1, 65536]")
        d = self._probe_desc("update_probes", **dict(desc, indirect_only=bool(indirect_only) or bool(desc.get("indirect_only", False))))
        n = d.count[0] * d.count[1] * d.count[2]
        u = self._probe_update("update_probes", n, frame, frame_stride, hysteresis, window, change)
        on_gpu, vol, ptr = self._update_target("update_probes", probes, (d.count[2], d.count[1], d.count[0], abi.PROBE_WORDS))
        st = abi.RenderStats()
        if on_gpu:
            import torch
            d.flags |= abi.PROBES_DEVICE_ARRAYS
            torch.cuda.current_stream(vol.device).synchronize()       # (whatever wrote the tensor)
        o = C.byref(opts) if opts is not None else None
        if placement is not None:
            _, held, place_ptr = self._placement("update_probes", placement, d, on_gpu)     # (held: a converted copy lives until the call returns)
            self._check(lib().hj_update_probes_placed(self._h, C.byref(d), C.byref(u), spp, o, place_ptr, ptr, C.byref(st)))
            del held
        else:
            self._check(lib().hj_update_probes(self._h, C.byref(d), C.byref(u), spp, o, ptr, C.byref(st)))
        return (vol, stats_dict(st)) if stats else vol

    def update_probe_visibility(self, desc, vis, atlas, *, frame, frame_stride=abi.PROBE_UPDATE_FRAME_STRIDE, hysteresis, window=None, placement=None):
        """hj_update_probe_visibility: a window of a (nz, ny, nx, res + 2, res + 2, 2) visibility atlas re-baked from the uploaded scene
        and folded into `atlas`.  desc as in `update_probes`; vis: a dict of `bake_probe_visibility`'s keywords (res, rays_per_texel,
        max_distance).  Per interior texel and moment new = old * hysteresis + fresh * (1 - hysteresis), the fresh value being
        `bake_probe_visibility`'s under the seed seed + frame * frame_stride; every border texel then copies its interior texel's new
        value.  hysteresis = 0 writes the fresh bake whatever the atlas held.  window, tensors and numpy arrays as in `update_probes`;
        placement as there: hj_update_probe_visibility_placed - the rays start at the placed positions and an inactive probe's texels,
        border included, keep every bit."""
        d = self._probe_desc("update_probe_visibility", **desc)
        v = self._probe_vis_desc("update_probe_visibility", **vis)
        n = d.count[0] * d.count[1] * d.count[2]
        u = self._probe_update("update_probe_visibility", n, frame, frame_stride, hysteresis, window, (0.0, 0.0))
        on_gpu, atl, ptr = self._update_target("update_probe_visibility", atlas, (d.count[2], d.count[1], d.count[0], v.res + 2, v.res + 2, 2))
        if on_gpu:
            import torch
            d.flags, v.flags = d.flags | abi.PROBES_DEVICE_ARRAYS, v.flags | abi.PROBE_VIS_DEVICE_ARRAYS
            torch.cuda.current_stream(atl.device).synchronize()       # (whatever wrote the tensor)
        if placement is not None:
            _, held, place_ptr = self._placement("update_probe_visibility", placement, d, on_gpu)   # (held until the call returns)
            self._check(lib().hj_update_probe_visibility_placed(self._h, C.byref(d), C.byref(v), C.byref(u), place_ptr, ptr))
            del held
        else:
            self._check(lib().hj_update_probe_visibility(self._h, C.byref(d), C.byref(v), C.byref(u), ptr))
        return atl

    def _placement(self, what, placement, d, on_gpu, copy=False):
        """A placement array beside a call's other arrays: (nz, ny, nx, 4) float32 of their kind - a contiguous tensor on the renderer's
        GPU, or a numpy array with finite offsets -> (on_gpu, the array, its address)"""
        shape = (d.count[2], d.count[1], d.count[0], abi.PROBE_PLACE_WORDS)
        is_torch = type(placement).__module__.split(".")[0] == "torch"
        if on_gpu is not None and is_torch != bool(on_gpu):
            raise ValueError(f"{what}: the placement must be a {'tensor on the GPU' if on_gpu else 'numpy array'}, as the call's other arrays are")
        if is_torch:
            return self._update_target(what, placement, shape)
        arr = np.array(placement, np.float32, order="C") if copy else np.ascontiguousarray(placement, np.float32)
        if arr.shape != shape:
            raise ValueError(f"{what}: a placement of {shape} is needed (got {arr.shape})")
        if not np.isfinite(arr[..., 0:3]).all():
            raise ValueError(f"{what}: the placement holds a non-finite offset")
        return False, arr, arr.ctypes.data

    @staticmethod
    def new_placement(count, device=None):
        """A placement of every probe on its grid point, active: zeros of (nz, ny, nx, 4) float32 - numpy, or with device (a torch
        device) a tensor there.  Word 3 of a probe holds its state as uint32 bits: `placement[..., 3].view(uint32)`."""
        shape = (int(count[2]), int(count[1]), int(count[0]), abi.PROBE_PLACE_WORDS)
        if device is None:
            return np.zeros(shape, np.float32)
        import torch
        return torch.zeros(shape, dtype=torch.float32, device=device)

    def place_probes(self, desc, vis, placement, *, frame, min_front_distance, frame_stride=abi.PROBE_UPDATE_FRAME_STRIDE,
                     backface_share=abi.PROBE_PLACE_BACKFACE_SHARE, max_offset=abi.PROBE_PLACE_MAX_OFFSET, window=None, relocate=True, classify=True,
                     indirect_only=False):
        """hj_place_probes: one relocation-and-classification step (Majercik et al. 2021) over a window of a (nz, ny, nx, 4) placement
        (`new_placement`): per probe an offset in world units (words 0-2) and a state (word 3 as uint32 bits, 0 active).  desc, vis, frame,
        frame_stride and window as in `update_probe_visibility` (vis: res, rays_per_texel, max_distance).  From the probe's rays a probe
        that sees more than `backface_share` back faces moves through the nearest one, a probe with a front face nearer than
        `min_front_distance` moves away from it, a probe that has room moves back towards its grid point; no offset leaves
        `max_offset` spacings.  A probe inside geometry, or with no front face within its eight cells, becomes inactive.  The defaults
        0.25 and 0.45 are the paper's and RTXGI's starting points, not tuned here.  relocate / classify = False leave the offsets / the
        states alone.  A tensor on the renderer's GPU is updated in place and returned; a numpy array gives an updated copy.
        indirect_only: the desc's abi.PROBES_INDIRECT_ONLY, accepted and not read - a placement step traces rays and gathers nothing."""
        d = self._probe_desc("place_probes", **dict(desc, indirect_only=bool(indirect_only) or bool(desc.get("indirect_only", False))))
        v = self._probe_vis_desc("place_probes", **vis)
        n = d.count[0] * d.count[1] * d.count[2]
        u = self._probe_update("place_probes", n, frame, frame_stride, 0.0, window, (0.0, 0.0))
        mfd, share, mo = np.float32(min_front_distance), np.float32(backface_share), np.float32(max_offset)
        if not (np.isfinite(mfd) and mfd > 0):
            raise ValueError(f"place_probes: min_front_distance {min_front_distance}: finite and > 0 is needed")
        if not 0 <= share <= 1:
            raise ValueError(f"place_probes: backface_share {backface_share} outside [0, 1]")
        if not 0 <= mo < 0.5:
            raise ValueError(f"place_probes: max_offset {max_offset} outside [0, 0.5)")
        on_gpu, arr, ptr = self._placement("place_probes", placement, d, None, copy=True)
        flags = (0 if relocate else abi.PROBE_PLACE_NO_RELOCATE) | (0 if classify else abi.PROBE_PLACE_NO_CLASSIFY)
        pl = abi.ProbePlace(u.first_probe, u.num_probes, u.frame, u.frame_stride, float(mfd), float(share), float(mo), flags)
        if on_gpu:
            import torch
            d.flags, v.flags = d.flags | abi.PROBES_DEVICE_ARRAYS, v.flags | abi.PROBE_VIS_DEVICE_ARRAYS
            torch.cuda.current_stream(arr.device).synchronize()       # (whatever wrote the tensor)
        self._check(lib().hj_place_probes(self._h, C.byref(d), C.byref(v), C.byref(pl), ptr))
        return arr

    def texture_lookup(self, texture, uv):
        """hj_debug_texture_lookup: the colour the shade stage takes from `texture` at (n, 2) float32 uv -> (n, 3) float32."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(uv), 3), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(lib().hj_debug_texture_lookup(self._h, int(texture), uv.ctypes.data_as(fp), len(uv), out.ctypes.data_as(fp)))
        return out

    def num_probe(self, op, words):
        """hj_debug_num: the device text of the numeric contract (kernels/hj_num.h) on caller-given inputs.  op: a name of
        abi.NUM_OPS (or its index); words: (n, k <= 6) uint32 - the bits of the floats, or RNG states - padded with zeros to the
        record's 6 words.  Returns (n, 4) uint32 (include/hijiki_hip.h says which words an op reads and writes)."""
        w = np.asarray(words, np.uint32)
        w = w.reshape(len(w), -1)
        rec = np.zeros((len(w), abi.NUM_IN_WORDS), np.uint32)
        rec[:, :w.shape[1]] = w
        out = np.zeros((len(w), abi.NUM_OUT_WORDS), np.uint32)
        up = C.POINTER(C.c_uint32)
        self._check(lib().hj_debug_num(self._h, abi.NUM_OPS.index(op) if isinstance(op, str) else int(op), rec.ctypes.data_as(up),
                                       len(rec), out.ctypes.data_as(up)))
        return out

    def shade_step(self, records, opts=None, num_wg=1, parity=0):
        """hj_debug_shade_step: one pass of the shade stage over (n, 18) uint32 records (path state and raw hit: include/hijiki_hip.h
        lists the words) on the uploaded scene.  Returns ((n, 33) uint32 output records, (num_wg, 3) uint32 counters: continuing
        paths, shadow records, next-event samples the light-shaft grid answered)."""
        rec = np.ascontiguousarray(records, np.uint32).reshape(-1, abi.STEP_IN_WORDS)
        out = np.zeros((len(rec), abi.STEP_OUT_WORDS), np.uint32)
        ctr = np.zeros((max(int(num_wg), 1), 3), np.uint32)
        up = C.POINTER(C.c_uint32)
        o = opts if opts is not None else default_opts()
        self._check(lib().hj_debug_shade_step(self._h, C.byref(o), rec.ctypes.data_as(up), len(rec), int(num_wg), int(parity),
                                              out.ctypes.data_as(up), ctr.ctypes.data_as(up)))
        return out, ctr

    def reconstruct(self, blocks, samples, opts=None):
        """hj_debug_reconstruct: one reconstruction pass over caller-given samples into the framebuffer.  blocks: a ctypes array (or
        list) of at most abi.RECON_MAX_BLOCKS abi.ImageBlock; samples: per block a (dim_y, dim_x, 8) float32 array in the layout of
        `samples` (or all of them concatenated)."""
        if not isinstance(blocks, C.Array):
            blocks = (abi.ImageBlock * len(blocks))(*blocks)
        if not isinstance(samples, np.ndarray):
            samples = np.concatenate([np.ascontiguousarray(s, np.float32).ravel() for s in samples]) if len(samples) else np.zeros(0, np.float32)
        smp = np.ascontiguousarray(samples, np.float32).ravel()
        need = sum(8 * b.dimension[0] * b.dimension[1] for b in blocks)
        if smp.size != need:
            raise ValueError(f"reconstruct: {smp.size} sample floats for blocks that hold {need}")
        self._check(lib().hj_debug_reconstruct(self._h, blocks, len(blocks), C.byref(opts) if opts is not None else None,
                                               smp.ctypes.data_as(C.POINTER(C.c_float))))

    def samples(self, block, opts=None):
        """Intermediate image of one block: (dim_y, dim_x, 8) = (rgb, 1, normal, depth)."""
        out = np.zeros((block.dimension[1], block.dimension[0], 8), np.float32)
        self._check(lib().hj_debug_samples(self._h, C.byref(block), C.byref(opts) if opts is not None else None,
                                           out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def read(self):
        """(H, W, 4) float32 accumulation image (sum w*rgb, sum w)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(lib().hj_framebuffer_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def resolve(self):
        """(H, W, 3) float32 rgb / w (src/main.rs:1399)."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        self._check(lib().hj_framebuffer_resolve(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out
