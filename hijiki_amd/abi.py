"""ctypes mirror of include/hijiki_hip.h (POD records + option/stat structs).

Pure declarations; nothing here computes.  Layouts are asserted against the
byte sizes of SURVEY.md Appendix A (= reference std430 / #[repr(C)] layouts).
"""
import ctypes as C

HJ_OK, HJ_ERR_INVALID, HJ_ERR_DEVICE, HJ_ERR_NOMEM, HJ_ERR_STATE, HJ_ERR_UNSUPPORTED = range(6)
STATUS_NAMES = {0: "HJ_OK", 1: "HJ_ERR_INVALID", 2: "HJ_ERR_DEVICE", 3: "HJ_ERR_NOMEM", 4: "HJ_ERR_STATE",
                5: "HJ_ERR_UNSUPPORTED"}

# MaterialType discriminants (reference src/main.rs:34-45)
MAT_DIFFUSE, MAT_DIFFUSECBOARD, MAT_MIRROR, MAT_DIELECTRIC, MAT_EMISSIVE = range(5)
MAT_DIFFUSE_TEXTURED = 5          # no counterpart upstream: diffuse, colour from image texture `index`
TEX_NEAREST, TEX_BILINEAR = 0, 1
MATERIAL_TAG_SHIFT = 24
MATERIAL_INDEX_MASK = 0x00FFFFFF
BVH_INNER = 0xFFFFFFFF
BVH_ROOT_EXIT = 1000000
BLOCK_SIZE = 128
RENDER_TIME_KERNELS = 1
RENDER_SPLIT_KERNELS = 2
RENDER_STATIC_DEAL = 4
RENDER_NO_DRAIN = 8
RENDER_NO_LIGHT_GRID = 16
UPDATE_DEVICE_ARRAYS = 1          # hj_scene_update_shapes flags
UPDATE_NO_LIGHT_GRID = 2
TRACE_ANY_HIT = 1                 # hj_trace_rays flags
TRACE_DEVICE_ARRAYS = 2
PATHS_DEVICE_ARRAYS = 1           # hj_trace_paths flag
GATHER_DEVICE_ARRAYS = 1          # hj_trace_irradiance flags
GATHER_SPHERE = 2
GATHER_SH9 = 4                    # (only together with GATHER_SPHERE)
GATHER_INDIRECT = 16              # the first segment's emission is left out (8 is reserved: refused)
LIGHTMAP_DEVICE_ARRAYS = 1        # hj_lightmap_desc flag
LIGHTMAP_MAX_GUTTER = 64          # hj_bake_lightmap: dilation passes a call
LIGHTMAP_NONE = 0xFFFFFFFF        # owner word of a texel nobody owns
LIGHTMAP_FILTER_MAX_ITERATIONS = 8  # hj_lightmap_filter: iteration i uses the step 1 << i
PROBES_DEVICE_ARRAYS = 1          # hj_probe_desc flags
PROBES_INDIRECT_ONLY = 4          # the bakes and updates gather with GATHER_INDIRECT (2 is reserved: refused)
PROBE_WORDS = 28                  # words of a probe record: 27 SH coefficients of the irradiance, the validity weight
PROBE_MAX_COUNT, PROBE_MAX_PROBES = 1024, 1 << 22   # probes along an axis, probes of a volume
PROBE_VIS_DEVICE_ARRAYS, PROBE_VIS_NO_BACKFACE, PROBE_VIS_NO_CHEBYSHEV = 1, 2, 4   # hj_probe_vis_desc flags
PROBE_VIS_RES = (4, 8, 16)        # interior texels per side of a probe's octahedral map
PROBE_VIS_MAX_RAYS_PER_TEXEL = 64
PROBE_VIS_MAX_DISTANCE = 1e18
PROBE_VIS_SLAB_RAYS = 1 << 19     # the most rays of one slab of hj_bake_probe_visibility
PROBE_UPDATE_WORDS = 8            # words of hj_probe_update
PROBE_UPDATE_SOFT_STEP = 0.15     # what a change beyond change_soft takes off the hysteresis (Majercik et al. 2019)
PROBE_UPDATE_CHANGE = (0.25, 0.8)  # the wrapper's defaults for change_soft, change_hard: the paper's starting point, not tuned
PROBE_UPDATE_FRAME_STRIDE = 0x9E3779B1   # the wrapper's default frame_stride: odd, so that 2^32 frames have 2^32 seeds
PROBE_PLACE_WORDS = 4             # words of a probe's placement: the offset (float32 x 3), the state (uint32: 0 active)
PROBE_PLACE_NO_RELOCATE, PROBE_PLACE_NO_CLASSIFY = 1, 2   # hj_probe_place flags
PROBE_PLACE_BACKFACE_SHARE, PROBE_PLACE_MAX_OFFSET = 0.25, 0.45   # the wrapper's defaults: the paper's and RTXGI's starting points, not tuned
CLOSEST_DEVICE_ARRAYS = 1         # hj_closest_points flag
CLOSEST_WORDS = 8                 # words of a closest-point record: shape index, distance, q.xyz, u, v, side
DISTANCE_UNSIGNED = 1             # hj_distance_field flag
ALLHITS_DEVICE_ARRAYS = 1         # hj_trace_rays_all flag
ALLHITS_MAX_HITS = 8              # the most hit records a ray of hj_trace_rays_all gets
INSIDE_DEVICE_ARRAYS, INSIDE_PARITY = 1, 2   # hj_points_inside flags
# the three directions of hj_points_inside (HJ_INSIDE_DIR0 .. 2): the float32 nearest each literal
INSIDE_DIRECTIONS = ((0.28284273, 0.51961523, 0.8062258), (-0.84261495, 0.2236068, -0.48989794), (0.5477226, -0.7745967, -0.31622776))
MATERIALS_DEVICE_ARRAYS = 1       # hj_eval_materials flag
MATERIALS_WORDS = 8               # words of a material record: albedo.rgb, material word, emission.rgb, 0
MATERIAL_MISS = 0xFFFFFFFF        # ... its word 3 for a miss
AOV_DEVICE_ARRAY = 1              # hj_render_aovs / hj_render_aovs_frame flag
AOV_WORDS = 12                    # words of an AOV pixel: albedo.rgb, samples | normal.xyz, t | emission.rgb, hits - each a sum
AOV_MAX_FOLLOW = 8                # hj_render_aovs_followed / hj_render_aovs_frame_followed: the most continuations of a chain
FOLLOW_DEVICE_ARRAYS = 1          # hj_follow_specular flag
DENOISE_DEVICE_ARRAYS = 1         # hj_denoise_opts flag
DENOISE_MAX_ITERATIONS = 8        # hj_denoise_opts: iteration i uses the step 1 << i
TEMPORAL_WORDS = 12               # words of a history record: I.rgb, N | m1, m2, z, valid word | n.xyz, 0
TEMPORAL_FEEDBACK = 1             # hj_temporal_opts flag: the first iteration's light goes into the history
TEMPORAL_VARIANCE_FRAMES = 4      # a history this long gives the variance of its temporal moments
MOTION_WORDS = 4                  # words of a motion record (hj_render_motion): sx, sy, zp, id bits
MOTION_NONE = 0xFFFFFFFF          # ... its word 3 for a pixel without a previous position
MOTION_DEVICE_SHAPES = 1          # hj_render_motion flag: the previous shape arrays are device pointers
MOTION_DEVICE_OUT = 2             # ... the motion image is a device pointer
MOTION_LEFT = 0xFFFFFFFE          # hj_render_motion_followed: word 3 of a pixel whose chain left a specular surface and hit nothing
PROBE_LIT_WORDS = 4               # words of a probe-lit pixel (hj_render_probe_lit): the sums of L.rgb, the sample count
VERSION = (0, 33, 0)              # the ABI this mirror describes: hj_version() == (major << 16) | (minor << 8) | patch


def probe_vis_words(res):
    """HJ_PROBE_VIS_WORDS: the words of one probe's atlas, (res + 2)^2 texels of two moments"""
    return 2 * (res + 2) * (res + 2)


# hj_debug_num: enum hj_num_op in its order, the record sizes and the cap
NUM_OPS = ("exp", "sincos2pi", "atan2", "asin", "min", "max", "div", "sqrt", "dot3", "cross3", "normalize3", "reflect3", "rng_seed",
           "rng_uint", "rng_float", "rand_cos_hemisphere", "rand_uniform_sphere", "rand_barycentric")
NUM_IN_WORDS, NUM_OUT_WORDS, NUM_MAX_RECORDS = 6, 4, 1 << 20
# hj_debug_shade_step: the record sizes and the cap
STEP_IN_WORDS, STEP_OUT_WORDS, STEP_MAX_RECORDS = 18, 33, 1 << 16
REINSERT_MAX_PASSES = 64         # hj_optimize_bvh_device: passes a call
RECON_MAX_BLOCKS = 64            # hj_debug_reconstruct: blocks a call
VOTE_MAX_LEVELS = 8192           # hj_debug_vote_*: levels of inner nodes the exchange accepts and a ray votes at
VOTE_MAX_RAYS = 1 << 20          # hj_debug_vote_cast: rays a call
VOTE_MAX_SHADOW = 16             # ... and the largest w_shadow (HJ_BVH_VOTE_SHADOW's range)
VOTE_MISS = 0xFFFFFFFF           # ... the leaf position of a ray that hit nothing

f32, u32, u64 = C.c_float, C.c_uint32, C.c_uint64


class Camera(C.Structure):
    _fields_ = [("position", f32 * 4), ("rotation", f32 * 4), ("fov", f32), ("_pad", f32 * 3)]


class SceneInfo(C.Structure):
    _fields_ = [("camera", Camera), ("num_spheres", u32), ("num_quads", u32), ("num_triangles", u32),
                ("num_emitters", u32)]


class BvhNode(C.Structure):
    _fields_ = [("aabb_min", f32 * 3), ("shape_index", u32), ("aabb_max", f32 * 3), ("exit_index", u32)]


def direction_classes(mode):
    """hj_direction_classes (include/hijiki_hip.h): link orderings of a directional tree."""
    if mode <= 0 or mode > 8:
        return 1
    return 6 if mode == 8 else 1 << bin(mode & 7).count("1")


def ray_direction_class(mode, d):
    """hj_ray_direction_class for an (n, 3) float32 array of directions."""
    import numpy as np
    b = np.ascontiguousarray(d, np.float32).view(np.uint32).reshape(-1, 3)
    if mode <= 0 or mode > 8:
        return np.zeros(len(b), np.int64)
    if mode == 8:
        major = np.argmax(b & 0x7FFFFFFF, axis=1)          # (first of equals, as the C text)
        return 2 * major + (b[np.arange(len(b)), major] >> 31).astype(np.int64)
    cls, k = np.zeros(len(b), np.int64), 0
    for a in range(3):
        if mode & (1 << a):
            cls |= (b[:, a] >> 31).astype(np.int64) << k
            k += 1
    return cls


class Sphere(C.Structure):
    _fields_ = [("center", f32 * 3), ("radius", f32)]


class Quad(C.Structure):
    _fields_ = [("origin", f32 * 3), ("_pad1", f32), ("edge1", f32 * 3), ("_pad2", f32), ("edge2", f32 * 3),
                ("_pad3", f32)]


class Triangle(C.Structure):
    _fields_ = [("v", u32 * 3)]


class Vertex(C.Structure):
    _fields_ = [("pos", f32 * 3), ("u", f32), ("normal", f32 * 3), ("v", f32)]


class Emitter(C.Structure):
    _fields_ = [("shape", u32), ("pdf", f32), ("cdf", f32), ("_pad", f32)]


class Diffuse(C.Structure):
    _fields_ = [("color", f32 * 3), ("_pad", f32)]


class DiffuseCB(C.Structure):
    _fields_ = [("color_a", f32 * 3), ("scale_u", f32), ("color_b", f32 * 3), ("scale_v", f32)]


class Dielectric(C.Structure):
    _fields_ = [("extinction", f32 * 3), ("eta", f32)]


class Emissive(C.Structure):
    _fields_ = [("power", f32 * 3), ("_pad", f32)]


class Texture(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("filter", u32), ("first_texel", u32)]


class TextureSet(C.Structure):
    _fields_ = [("textures", C.POINTER(Texture)), ("num_textures", C.c_size_t),
                ("texels", C.POINTER(f32)), ("num_texels", C.c_size_t)]


class Environment(C.Structure):
    """hj_environment (ABI 0.5): texture `texture` of the scene's set lights every ray that leaves the scene (DESIGN.md
    "Environment lighting")."""
    _fields_ = [("texture", u32), ("scale", f32 * 3), ("select_prob", f32), ("_reserved", u32)]


class ImageBlock(C.Structure):
    _fields_ = [("id", u32), ("seed", u32), ("origin", u32 * 2), ("dimension", u32 * 2),
                ("original_dimension", u32 * 2), ("sample_offset", f32 * 2)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("camera", Camera),
        ("bvh", C.POINTER(BvhNode)), ("num_bvh_nodes", C.c_size_t),
        ("spheres", C.POINTER(Sphere)), ("num_spheres", C.c_size_t),
        ("quads", C.POINTER(Quad)), ("num_quads", C.c_size_t),
        ("triangles", C.POINTER(Triangle)), ("num_triangles", C.c_size_t),
        ("vertices", C.POINTER(Vertex)), ("num_vertices", C.c_size_t),
        ("materials", C.POINTER(u32)), ("num_materials", C.c_size_t),
        ("emitters", C.POINTER(Emitter)), ("num_emitters", C.c_size_t),
        ("diffuse", C.POINTER(Diffuse)), ("num_diffuse", C.c_size_t),
        ("diffusecb", C.POINTER(DiffuseCB)), ("num_diffusecb", C.c_size_t),
        ("dielectric", C.POINTER(Dielectric)), ("num_dielectric", C.c_size_t),
        ("emissive", C.POINTER(Emissive)), ("num_emissive", C.c_size_t),
    ]


class RenderOpts(C.Structure):
    _fields_ = [("use_bvh", u32), ("recon_radius", u32), ("recon_stddev", f32), ("max_bounces", u32),
                ("rr_start", u32), ("batch_blocks", u32), ("flags", u32), ("_reserved", u32)]

    @staticmethod
    def default():
        return RenderOpts(use_bvh=1, recon_radius=2, recon_stddev=0.5, max_bounces=1000, rr_start=4, batch_blocks=0)


class AdaptiveOpts(C.Structure):
    """hj_adaptive_opts (ABI 0.13): the rounds and the stop rule of hj_trace_paths_adaptive, hj_trace_irradiance_adaptive and
    hj_bake_lightmap_adaptive."""
    _fields_ = [("spp_min", u32), ("spp_step", u32), ("spp_max", u32), ("rel_error", f32), ("floor", f32)]


class LightmapDesc(C.Structure):
    """hj_lightmap_desc (ABI 0.16): the atlas, the triangle range, the seeds and the offset of hj_lightmap_texels / hj_bake_lightmap."""
    _fields_ = [("width", u32), ("height", u32), ("first_triangle", u32), ("num_triangles", u32), ("seed", u32), ("seed_stride", u32),
                ("offset", f32), ("flags", u32)]


class LightmapFilter(C.Structure):
    """hj_lightmap_filter (ABI 0.17): the iterations and the edge stops of hj_filter_lightmap / hj_bake_lightmap_filtered."""
    _fields_ = [("iterations", u32), ("sigma_position", f32), ("sigma_normal", f32), ("sigma_color", f32), ("flags", u32)]


class DenoiseOpts(C.Structure):
    """hj_denoise_opts (ABI 0.27): the iterations and the edge stops of hj_denoise_frame."""
    _fields_ = [("iterations", u32), ("sigma_normal", f32), ("sigma_depth", f32), ("sigma_luminance", f32), ("sigma_albedo", f32), ("flags", u32)]


class TemporalOpts(C.Structure):
    """hj_temporal_opts (ABI 0.28): the two cameras, the blend weights and the history tests of hj_denoise_frame_temporal."""
    _fields_ = [("camera", Camera), ("prev_camera", Camera), ("alpha", f32), ("alpha_moments", f32), ("depth_tolerance", f32), ("normal_cos", f32),
                ("max_history", u32), ("flags", u32)]


class ProbeDesc(C.Structure):
    """hj_probe_desc (ABI 0.19): the grid, the seeds and the validity rule of hj_probe_points / hj_bake_probes / hj_sample_probes."""
    _fields_ = [("origin", f32 * 3), ("spacing", f32 * 3), ("count", u32 * 3), ("seed", u32), ("seed_stride", u32), ("min_distance", f32),
                ("flags", u32)]


class ProbeVisDesc(C.Structure):
    """hj_probe_vis_desc (ABI 0.21): the octahedral map, the bake's rays and the look-up's bias and switches of
    hj_probe_visibility_rays / hj_bake_probe_visibility / hj_sample_probes_visible."""
    _fields_ = [("res", u32), ("rays_per_texel", u32), ("max_distance", f32), ("normal_bias", f32), ("flags", u32)]


class ProbeLighting(C.Structure):
    """hj_probe_lighting (ABI 0.32): the volume hj_render_probe_lit / hj_render_probe_lit_frame light a frame from - the grid, the
    visibility desc (NULL: hj_sample_probes' weights alone) and the probes, atlas and placement as the selected look-up takes them."""
    _fields_ = [("desc", C.POINTER(ProbeDesc)), ("vis", C.POINTER(ProbeVisDesc)), ("probes", C.c_void_p), ("atlas", C.c_void_p),
                ("placement", C.c_void_p)]


class ProbeUpdate(C.Structure):
    """hj_probe_update (ABI 0.22): the probe window, the frame's seeds, the hysteresis and the change thresholds of hj_update_probes /
    hj_update_probe_visibility."""
    _fields_ = [("first_probe", u32), ("num_probes", u32), ("frame", u32), ("frame_stride", u32), ("hysteresis", f32), ("change_soft", f32),
                ("change_hard", f32), ("flags", u32)]


class ProbePlace(C.Structure):
    """hj_probe_place (ABI 0.23): the probe window, the frame's seeds and the thresholds of hj_place_probes."""
    _fields_ = [("first_probe", u32), ("num_probes", u32), ("frame", u32), ("frame_stride", u32), ("min_front_distance", f32),
                ("backface_share", f32), ("max_offset", f32), ("flags", u32)]


class RenderStats(C.Structure):
    _fields_ = [("paths", u64), ("closest_rays", u64), ("shadow_rays", u64), ("batches", u64),
                ("bounce_rounds", u64), ("trace_closest_ms", C.c_double), ("trace_shadow_ms", C.c_double),
                ("shade_ms", C.c_double), ("reconstruct_ms", C.c_double), ("total_ms", C.c_double),
                ("closest_launches", u64), ("path_ms", C.c_double), ("path_launches", u64),
                ("hits", u64), ("unoccluded_shadow_rays", u64), ("path_busy_ms", C.c_double),
                ("shadow_rays_proven_free", u64)]


# byte sizes of SURVEY.md Appendix A
_SIZES = {Camera: 48, SceneInfo: 64, BvhNode: 32, Sphere: 16, Quad: 48, Triangle: 12, Vertex: 32, Emitter: 16,
          Diffuse: 16, DiffuseCB: 32, Dielectric: 16, Emissive: 16, ImageBlock: 40, Texture: 16}
for _t, _n in _SIZES.items():
    assert C.sizeof(_t) == _n, (_t.__name__, C.sizeof(_t), _n)


class HijikiError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status
