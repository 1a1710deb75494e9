/*
 * hijiki_hip.h — the drop-in boundary of the MI355X path-tracing hot path.
 *
 * Plain C ABI: POD structs, pointers and sizes only.  Every record below is
 * byte-for-byte the record the reference host (`/root/reference/src/main.rs`)
 * writes into its scene buffer and that the reference shaders read; every
 * entry point replaces one piece of the reference's host<->shader contract
 * (there is no plugin interface in the reference — the boundary is what
 * `Renderer::new/render/save_image` hand to wgpu).  A Rust host would bind to
 * this header with an `extern "C"` block.
 *
 * Citations `file:line` are relative to the reference checkout.
 */
#ifndef HIJIKI_HIP_H
#define HIJIKI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* libraries are built with -fvisibility=hidden */
#endif

/* ------------------------------------------------------------------ status */

enum hj_status {
  HJ_OK = 0,
  HJ_ERR_INVALID = 1,     /* bad argument / inconsistent scene (reference: assert!/panic!) */
  HJ_ERR_DEVICE = 2,      /* HIP runtime error                                              */
  HJ_ERR_NOMEM = 3,       /* host or device allocation failed                               */
  HJ_ERR_STATE = 4,       /* call order violated (e.g. render before scene upload)          */
  HJ_ERR_UNSUPPORTED = 5  /* reference behaviour that is undefined / a panic upstream       */
};

/* ------------------------------------------------------- material tag words */

/* MaterialType discriminants, src/main.rs:34-45; shader macros MATERIAL_TAG_*
 * injected at src/main.rs:778-783.  A material word is (tag << 24) + index
 * (src/main.rs:275; decoded at shader/render.glsl:107-109). */
enum hj_material_tag {
  HJ_MAT_DIFFUSE = 0,
  HJ_MAT_DIFFUSECBOARD = 1,
  HJ_MAT_MIRROR = 2,
  HJ_MAT_DIELECTRIC = 3,
  HJ_MAT_EMISSIVE = 4,
  HJ_MAT_DIFFUSE_TEXTURED = 5   /* no counterpart upstream: diffuse, colour from image texture `index` (hj_texture_set) */
};
#define HJ_MATERIAL_TAG_SHIFT 24u
#define HJ_MATERIAL_INDEX_MASK 0x00FFFFFFu
#define HJ_BVH_INNER 0xFFFFFFFFu     /* shape_index of an inner node, src/main.rs:219 */
#define HJ_BVH_ROOT_EXIT 1000000u    /* exit index of the root,       src/main.rs:231 */
#define HJ_BLOCK_SIZE 128u           /* src/main.rs:1485 */

/* ------------------------------------------------- device records (std430) */

/* Camera, src/main.rs:154-160 / shader/render.glsl:12-16.  48 bytes. */
typedef struct hj_camera {
  float position[4];   /* xyz used, w = 0                                  */
  float rotation[4];   /* unit quaternion xyzw                             */
  float fov;           /* HORIZONTAL field of view in degrees              */
  float _pad[3];
} hj_camera;

/* SceneBufferInfo, src/main.rs:400-408 / shader/scene.glsl:1-8.  64 bytes. */
typedef struct hj_scene_info {
  hj_camera camera;
  uint32_t num_spheres, num_quads, num_triangles, num_emitters;
} hj_scene_info;

/* CompiledBVHNode, src/main.rs:92-99 / shader/scene.glsl:10-13.  32 bytes.
 * Pre-order skip-link array; see hj_host.h for the builder. */
typedef struct hj_bvh_node {
  float aabb_min[3];
  uint32_t shape_index;  /* global shape index of a leaf, HJ_BVH_INNER otherwise */
  float aabb_max[3];
  uint32_t exit_index;   /* node to visit when this subtree is skipped / done   */
} hj_bvh_node;

/* Direction classes of a ray (no counterpart upstream: shader/scene.glsl:97-133 visits the two children of a node in ARRAY order
 * whatever the ray's direction).  A "directional" tree is K skip-link arrays over the same boxes and leaves that differ only in
 * which child of a node comes first; a ray walks array hj_ray_direction_class(mode, d) from its root to its end.  The class is
 * a function of the SIGN BITS of the direction's components (mode 1..7: bit a of `mode` selects axis a, K = 2^axes, e.g. 7 = the
 * eight octants) or of its major axis and that component's sign (mode 8, K = 6).  One text for the host compiler, the oracle and
 * the kernels. */
#define HJ_DIR_MODE_NONE 0
#define HJ_DIR_MODE_OCTANTS 7
#define HJ_DIR_MODE_MAJOR_AXIS 8
#define HJ_DIR_MAX_CLASSES 8
static inline int hj_direction_classes(int mode) {
  if (mode <= 0 || mode > 8) return 1;
  if (mode == 8) return 6;
  return 1 << ((mode & 1) + ((mode >> 1) & 1) + ((mode >> 2) & 1));
}
static inline int hj_ray_direction_class(int mode, const float d[3]) {
  uint32_t b[3];
  int a, k = 0, cls = 0;
  if (mode <= 0 || mode > 8) return 0;
  for (a = 0; a < 3; a++) { union { float f; uint32_t u; } c; c.f = d[a]; b[a] = c.u; }
  if (mode == 8) {
    int major = 0;
    uint32_t best = b[0] & 0x7FFFFFFFu;
    for (a = 1; a < 3; a++) if ((b[a] & 0x7FFFFFFFu) > best) { best = b[a] & 0x7FFFFFFFu; major = a; }
    return 2 * major + (int)(b[major] >> 31);
  }
  for (a = 0; a < 3; a++) if (mode & (1 << a)) cls |= (int)(b[a] >> 31) << k++;
  return cls;
}

/* Sphere, src/shape.rs:6-11 / shader/shapes/sphere.glsl:1-3.  16 bytes. */
typedef struct hj_sphere { float center[3]; float radius; } hj_sphere;

/* Quad, src/shape.rs:22-31 / shader/shapes/quad.glsl:1-5.  48 bytes. */
typedef struct hj_quad {
  float origin[3]; float _pad1;
  float edge1[3];  float _pad2;
  float edge2[3];  float _pad3;
} hj_quad;

/* Triangle = 3 indices into the global vertex array, src/main.rs:51,386. */
typedef struct hj_triangle { uint32_t v[3]; } hj_triangle;

/* Vertex, src/main.rs:54-60 / shader/shapes/triangle.glsl:1-4.  32 bytes. */
typedef struct hj_vertex { float pos[3]; float u; float normal[3]; float v; } hj_vertex;

/* Emitter, src/main.rs:368-374 / shader/scene.glsl:33-38.  16 bytes. */
typedef struct hj_emitter { uint32_t shape; float pdf; float cdf; float _pad; } hj_emitter;

/* Material records, src/main.rs:102-146 / shader/materials/{diffuse,diffusecb,dielectric,emissive}.glsl. */
typedef struct hj_diffuse    { float color[3]; float _pad; } hj_diffuse;
typedef struct hj_diffuse_cb { float color_a[3]; float scale_u; float color_b[3]; float scale_v; } hj_diffuse_cb;
typedef struct hj_dielectric { float extinction[3]; float eta; } hj_dielectric;
typedef struct hj_emissive   { float power[3]; float _pad; } hj_emissive;

/* Image texture (no counterpart upstream: the reference's only texture is the procedural checkerboard,
 * shader/materials/diffusecb.glsl).  16 bytes.  A HJ_MAT_DIFFUSE_TEXTURED word's index names a texture directly.
 * Texels are RGBA32F (4 floats, linear, alpha ignored), row-major, row 0 = the TOP of the image (the v = 1 edge);
 * the texture's texels start at texels[4 * first_texel].  The lookup is defined in DESIGN.md ("Image textures"). */
#define HJ_TEX_NEAREST 0u
#define HJ_TEX_BILINEAR 1u
typedef struct hj_texture { uint32_t width, height; uint32_t filter; uint32_t first_texel; } hj_texture;
/* The textures of a scene, borrowed for the duration of the call.  num_texels counts texels (4 floats each). */
typedef struct hj_texture_set {
  const hj_texture* textures; size_t num_textures;
  const float*      texels;   size_t num_texels;
} hj_texture_set;

/* Environment lighting (no counterpart upstream; ABI 0.5): texture `texture` of the scene's hj_texture_set, read as a
 * latitude-longitude map with +y up, lights every ray that leaves the scene.  Radiance from direction d = scale * the texture's
 * colour at (u, v) of d (DESIGN.md "Environment lighting").  select_prob = the probability that next-event estimation at a diffuse
 * hit samples the environment instead of an area emitter.  24 bytes. */
typedef struct hj_environment { uint32_t texture; float scale[3]; float select_prob; uint32_t _reserved; } hj_environment;

/* ImageBlock, src/main.rs:608-617 / shader/block.glsl:1-8.  40 bytes.
 * One per integrator+reconstruction dispatch pair in the reference
 * (src/main.rs:1322-1330). */
typedef struct hj_image_block {
  uint32_t id;
  uint32_t seed;
  uint32_t origin[2];
  uint32_t dimension[2];
  uint32_t original_dimension[2];
  float sample_offset[2];
} hj_image_block;

/* ------------------------------------------------------------ scene upload */

/* What CompiledScene::write_to_buffer (src/main.rs:561-605) packs into the
 * scene buffer, as 11 borrowed (pointer,count) arrays + the camera, in the
 * reference's sub-buffer order.  Global shape index space is
 * [spheres | quads | triangles]; `materials` has one word per shape in that
 * order (src/main.rs:278-287).  Arrays are borrowed for the duration of the
 * call only. */
typedef struct hj_scene_desc {
  hj_camera camera;
  const hj_bvh_node*   bvh;        size_t num_bvh_nodes;
  const hj_sphere*     spheres;    size_t num_spheres;
  const hj_quad*       quads;      size_t num_quads;
  const hj_triangle*   triangles;  size_t num_triangles;
  const hj_vertex*     vertices;   size_t num_vertices;
  const uint32_t*      materials;  size_t num_materials;   /* == number of shapes */
  const hj_emitter*    emitters;   size_t num_emitters;
  const hj_diffuse*    diffuse;    size_t num_diffuse;
  const hj_diffuse_cb* diffusecb;  size_t num_diffusecb;
  const hj_dielectric* dielectric; size_t num_dielectric;
  const hj_emissive*   emissive;   size_t num_emissive;
} hj_scene_desc;

/* Compile-time shader parameters of the reference, as run-time options:
 * USE_BVH (src/main.rs:769-777), RECONSTRUCTION_RADIUS / _STDDEV
 * (src/main.rs:916-921,1279-1286), the 1000-bounce cap and the `bounce > 3`
 * roulette start (shader/render.glsl:92,137). */
typedef struct hj_render_opts {
  uint32_t use_bvh;        /* 1 = skip-link BVH walk, 0 = linear scan (reference CLI default) */
  uint32_t recon_radius;   /* only 2 is supported (reference value)                           */
  float    recon_stddev;   /* 0.5 in the reference                                            */
  uint32_t max_bounces;    /* 1000                                                            */
  uint32_t rr_start;       /* roulette applies when bounce > rr_start - 1, i.e. 4 -> b > 3    */
  uint32_t batch_blocks;   /* blocks traced per wavefront batch; 0 = library default          */
  uint32_t flags;          /* HJ_RENDER_* bits                                                */
  uint32_t _reserved;
} hj_render_opts;

#define HJ_RENDER_TIME_KERNELS 1u   /* bracket every kernel with HIP events on its launch stream (fills *_ms) */
#define HJ_RENDER_SPLIT_KERNELS 2u  /* diagnostic: one launch per stage per bounce instead of the fused kernel */
#define HJ_RENDER_STATIC_DEAL 4u    /* hj_render_frame, world > 1: keep all passes of a block on one rank          */
#define HJ_RENDER_NO_DRAIN 8u       /* hj_render_frame: return when the frame's batches are ENQUEUED (hj_pipeline_wait) */
#define HJ_RENDER_NO_LIGHT_GRID 16u /* walk every shadow ray, also those the light-shaft grid proves unoccluded (same image) */

/* Per-render statistics (device counters; all in units of events). */
typedef struct hj_render_stats {
  uint64_t paths;            /* camera paths started (= sum of block areas)         */
  uint64_t closest_rays;     /* intersectScene(ray, its) calls                      */
  uint64_t shadow_rays;      /* intersectScene(ray) calls                           */
  uint64_t batches;          /* wavefront batches launched                          */
  uint64_t bounce_rounds;    /* per-bounce kernel rounds over all batches           */
  double   trace_closest_ms; /* HIP-event time of the closest-hit kernels (if timed)*/
  double   trace_shadow_ms;
  double   shade_ms;
  double   reconstruct_ms;
  double   total_ms;         /* host wall time of the call (all batches, both streams) */
  uint64_t closest_launches; /* number of closest-hit kernel launches timed         */
  double   path_ms;          /* HIP-event time of the fused k_path_wavefront launches (sum; launches overlap) */
  uint64_t path_launches;
  uint64_t hits;             /* closest-hit rays that hit a shape                   */
  uint64_t unoccluded_shadow_rays; /* shadow rays that reached their light           */
  double   path_busy_ms;     /* union of the path kernels' intervals = their exclusive GPU time (if timed) */
  uint64_t shadow_rays_proven_free; /* of shadow_rays (and of unoccluded_shadow_rays): answered by the light-shaft grid, no walk */
} hj_render_stats;

typedef struct hj_context hj_context;

/* ---------------------------------------------------------------- lifecycle */

/* Replaces GPU::new + Renderer::new resource creation (src/main.rs:684-713,
 * 1167-1314).  One context per GPU; no global state. */
int hj_context_create(int device_ordinal, hj_context** out_ctx);
void hj_context_destroy(hj_context* ctx);
/* Replaces unwrap()/panic! text: message of the last failing call on ctx, copied into a buffer of the CALLING thread
 * (valid until that thread's next hj_last_error call; the context's worker thread may fail at any time).  ctx may be
 * NULL for create errors. */
const char* hj_last_error(const hj_context* ctx);
/* Library / ABI version: (major<<16)|(minor<<8)|patch. */
uint32_t hj_version(void);
void hj_default_render_opts(hj_render_opts* opts);

/* -------------------------------------------------------------------- scene */

/* Replaces the staging copy of the packed scene buffer (src/main.rs:1186-1244)
 * and the bind-group plumbing (src/main.rs:808-855).  Validates the same
 * invariants the reference asserts (src/main.rs:562-565) plus index ranges,
 * copies, and re-lays the data out for the kernels (same boxes, same leaves, same visiting order per ray: DESIGN.md 4).
 * scene->bvh (NULL with num_bvh_nodes == 0: the tree hj_build_bvh_device left on the device, see there) must be what Scene::compile flattens (src/main.rs:203-231): a binary tree in pre-order with skip links (left child =
 * next record, its exit = the right child, a node's exit = the record behind its subtree or, on the right spine, any index >= the
 * node count); the boxes may be anything (a box that does not bound its subtree just culls what the reference would cull), other
 * link structures return HJ_ERR_INVALID.
 * Limit: the device node array - 32 bytes per record, TWO copies of the tree (the re-laid-out one and the reference's own, which
 * rays with a zero or non-finite direction component walk: DESIGN.md 4) - must fit in 4 GiB: about 67 M records per tree = 33 M shapes;
 * larger trees return HJ_ERR_UNSUPPORTED.
 * The previous scene is released first; the new one replaces it only when every stage has succeeded.  An upload that fails leaves
 * the context without a scene, and leaves the tree on the device (hj_build_bvh_device) as it was, ready for a retry. */
int hj_scene_upload(hj_context* ctx, const hj_scene_desc* scene);
/* hj_scene_upload with image textures (no counterpart upstream); hj_scene_upload(ctx, s) is hj_scene_upload_textured(ctx, s, NULL).
 * A HJ_MAT_DIFFUSE_TEXTURED word whose index is >= num_textures (any such word with textures == NULL), a texture with a zero
 * width or height, a filter other than HJ_TEX_NEAREST / HJ_TEX_BILINEAR, or texels beyond num_texels: HJ_ERR_INVALID (checked
 * before anything else happens, so a tree left by hj_build_bvh_device stays on the device); more than 2^32 texels, or a width or
 * height above 2^24: HJ_ERR_UNSUPPORTED.  The texels are copied to the device with the rest of the scene. */
int hj_scene_upload_textured(hj_context* ctx, const hj_scene_desc* scene, const hj_texture_set* textures /* may be NULL */);
/* hj_scene_upload_textured with an environment (ABI 0.5); env == NULL is hj_scene_upload_textured.  Checked before anything else
 * happens, each HJ_ERR_INVALID: texture index out of range, a scale component negative or not finite, a non-finite texel of the
 * environment, select_prob outside [0, 1], select_prob other than 1 with no emitters, select_prob > 0 when every cell of the
 * sampling distribution weighs 0.  An environment of more than 2^28 texels: HJ_ERR_UNSUPPORTED.  The sampling distribution (an
 * alias table over the texels) is built with the rest of the scene; an upload that fails keeps none of it. */
int hj_scene_upload_env(hj_context* ctx, const hj_scene_desc* scene, const hj_texture_set* textures, const hj_environment* env);

/* -------------------------------------------------------------- framebuffer */

/* Replaces creation of `final_texture` (W x H RGBA32F = (sum w*rgb, sum w),
 * src/main.rs:1209-1234).  Zero-initialised.  If `external_device_rgba` is
 * non-NULL the context accumulates into that caller-owned device buffer of
 * W*H*4 floats (tight pitch) instead of allocating its own — this is how a
 * torch/RCCL host shares the buffer for the multi-GPU reduce. */
int hj_framebuffer_create(hj_context* ctx, uint32_t width, uint32_t height,
                          void* external_device_rgba);
int hj_framebuffer_clear(hj_context* ctx);
/* Device pointer of the accumulation buffer (W*H*4 floats). */
void* hj_framebuffer_device_ptr(hj_context* ctx);
/* Replaces Renderer::save_image's texture->buffer copy + map (src/main.rs:
 * 1357-1394), tight pitch instead of ceil256(W) texels. */
int hj_framebuffer_read(hj_context* ctx, float* host_rgba /* W*H*4 */);
/* rgb / w of every pixel (src/main.rs:1395-1400, shader/preview.glsl:11). */
int hj_framebuffer_resolve(hj_context* ctx, float* host_rgb /* W*H*3 */);

/* ------------------------------------------------------------------- render */

/* Optional set-up step (no counterpart upstream: Renderer::new creates every resource it needs, src/main.rs:1167-1314):
 * allocates the batch slots - path state and sample buffers - that a render call of `total_blocks` ImageBlocks with
 * these options will use (for hj_render_frame: spp x blocks per pass / world), so that the first frame does not pay for
 * them (50 GB and 0.8 s for the benchmark's frames at the defaults).  A render call allocates whatever is missing.
 * Preconditions: a scene has been uploaded and a framebuffer created (HJ_ERR_STATE otherwise, as for a render call: the
 * sizes depend on both); no asynchronous frame in flight.  MEMORY: the defaults take up to 17 % of a 288 GB device (three
 * batch slots of 12.4 GB of path state + 4.3 GB of samples each, for calls of 32768 ImageBlocks and more; a call of n
 * blocks takes about n x 2.7 MB up to that; HJ_POOL).  Both hj_reserve and the render calls first fit their request to the free
 * device memory (hipMemGetInfo) and, when an allocation fails all the same - another context or the host application took
 * the memory in between -, give back every slot, halve the positions per workgroup (down to 1024), then the batch (down to
 * 64 ImageBlocks), then run ONE batch slot instead of three, and try again: HJ_ERR_NOMEM is returned only when the smallest
 * configuration (about 100 MB) does not fit, or hj_render_opts::batch_blocks fixed a batch that does not.  Slots keep what they hold until the context is destroyed or a larger request re-allocates them. */
int hj_reserve(hj_context* ctx, size_t total_blocks, const hj_render_opts* opts /* NULL = defaults */);

/* Replaces the body of Renderer::render (src/main.rs:1316-1355): for every
 * block IN ORDER, integrate (shader/render.glsl:149-175) and accumulate
 * (shader/reconstruction.glsl:22-66).  The result equals running the
 * reference's two dispatches per block sequentially; internally many blocks
 * are traced as one wavefront batch.  Blocks must satisfy
 * dimension <= 128 and original_dimension == framebuffer size.
 * Synchronous: returns when the framebuffer holds the result. */
int hj_render_blocks(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks,
                     const hj_render_opts* opts /* NULL = defaults */,
                     hj_render_stats* stats /* may be NULL */);

/* Deterministic ImageBlockGenerator (src/main.rs:619-682) + render of the
 * blocks owned by `rank` out of `world` (hj_block_owner: a diagonal deal over the block grid that
 * moves one step per pass), for passes [pass_begin, pass_end).  With world == 1 this is the whole frame.
 * The reference seeds blocks from the OS RNG (src/main.rs:643,670,675);
 * here seeds/offsets come from hj_block_seed / hj_pass_offset below. */
int hj_render_frame(hj_context* ctx, uint32_t spp, uint64_t master_seed,
                    uint32_t pass_begin, uint32_t pass_end,
                    uint32_t rank, uint32_t world,
                    const hj_render_opts* opts, hj_render_stats* stats);

/* ------------------------------------------------------------- BVH on device */

/* The tree of `Scene::compile` (src/main.rs:199-231) built on the device instead of by the host's SAH builder
 * (SURVEY.md 8f #2): a Morton-code LBVH over the shapes of `scene` (scene->bvh is ignored; camera, materials and emitters feed the
 * ray vote at its end: hj_tune_bvh_device), written to
 * out_nodes in the reference's flattened format - one shape per leaf, pre-order with skip links, every record
 * holding the bounds of its own subtree, 2 * shapes - 1 records.  Start-up path for large meshes (1 M triangles
 * in milliseconds); its topology is not the host builder's, which changes images only through epsilon-ties and
 * traversal cost.  Put the result into scene->bvh before hj_scene_upload. */
int hj_build_bvh_device(hj_context* ctx, const hj_scene_desc* scene, hj_bvh_node* out_nodes /* may be NULL */, size_t capacity,
                        size_t* out_num_nodes /* may be NULL */);
/* The device route without the host in the middle: the tree hj_build_bvh_device builds also STAYS on the device, with the shape
 * arrays it was built over, until the next build, until an upload takes it over, or until the context ends.
 *   hj_build_bvh_device(ctx, scene, NULL, 0, &n)      builds; nothing is copied to the host
 *   hj_scene_upload(ctx, scene) with scene->bvh == NULL and scene->num_bvh_nodes == 0
 *                                                     derives the kernels' records from that tree on the device (the same shape
 *                                                     counts as at the build: HJ_ERR_INVALID otherwise; no tree: HJ_ERR_STATE);
 *                                                     the upload that succeeds consumes the tree, an upload that fails leaves
 *                                                     the tree on the device
 *   hj_bvh_device_read(ctx, out_nodes, capacity, &n)  a copy of the tree for a host that wants one (out_nodes NULL: only n)
 * 1 M triangles: build + upload in tens of milliseconds (profiles/r06_startup_1M_triangles.txt).  Results are those of the same
 * tree handed over through the host, bit for bit. */
int hj_bvh_device_read(hj_context* ctx, hj_bvh_node* out_nodes, size_t capacity, size_t* out_num_nodes /* may be NULL */);

/* The boxes of a tree recomputed for shapes that have moved; the links stay (a REFIT, for deforming meshes and moving spheres:
 * one pass over the tree instead of a new build).  `scene` carries the shape arrays as they are NOW (same counts as the
 * topology's: the number of leaves is the number of shapes).  Topology:
 *   scene->bvh != NULL   any valid pre-order skip-link tree with one shape per leaf (Scene::compile's, hj_build_bvh_device's,
 *                        hj_tune_bvh_device's); only shape_index and exit_index are read, its boxes are ignored.  The context
 *                        KEEPS a copy of the links on the device (8 bytes per record, and as much again for the parents and
 *                        counters derived from them) until the context ends or another topology replaces it;
 *   scene->bvh == NULL && scene->num_bvh_nodes == 0   the links kept by the last refit that brought some (none: HJ_ERR_STATE;
 *                        those of another shape count: HJ_ERR_INVALID).
 * Record i of the result keeps shape_index and exit_index; a leaf's box is its shape's (as hj_build_bvh_device computes it), an
 * inner node's the union of its two children's (IEEE min / max: exact, the same whatever the order of evaluation).  So the refit
 * of a tree hj_build_bvh_device built, with the shapes unmoved, is that tree bit for bit.
 * The refitted tree stays on the device exactly as hj_build_bvh_device's does (it replaces such a tree): hj_scene_upload* with
 * scene->bvh == NULL takes it over, hj_bvh_device_read copies it out; out_nodes (may be NULL) receives it as well.
 * out_cost (may be NULL): sum over inner nodes of area(node) / area(root), accumulated in double - the tree's surface-area
 * cost, for a caller who wants to decide when a deformation has gone far enough to rebuild.
 * Refused with HJ_ERR_INVALID before the tree on the device or the kept links are touched: null arguments or shape arrays, fewer
 * than 2 shapes, a triangle that names an unknown vertex, num_bvh_nodes != 2 * shapes - 1, links that are not a pre-order skip-link
 * tree, a shape that is in no leaf or in two.  A failure after that (out of memory) leaves no tree on the device but keeps the
 * links.  hj_build_bvh_device neither reads nor drops the kept links; an upload consumes the tree, not the links.
 * Frame loop of an animation: move the shapes, hj_refit_bvh_device(ctx, scene with bvh = NULL, NULL, 0, NULL, NULL),
 * hj_scene_upload(ctx, scene with bvh = NULL), render. */
int hj_refit_bvh_device(hj_context* ctx, const hj_scene_desc* scene, hj_bvh_node* out_nodes /* may be NULL */, size_t capacity,
                        size_t* out_num_nodes /* may be NULL */, double* out_cost /* may be NULL */);

/* hj_optimize_bvh_device (ABI 0.15): the tree hj_build_bvh_device or hj_refit_bvh_device left on the device, optimised there by
 * parallel reinsertion (Meister & Bittner 2018; objective and bound of the host's insertion-based pass): at most `passes` (<= 64)
 * passes, each of which lets every node but the root and its children look for the node whose sibling it should become, resolves
 * the conflicts (a move locks the nodes whose links it rewrites; the larger gain, then the larger node index wins; a pass that
 * does not lower the cost is taken back and repeated with every node on a move's path locked, which makes the gains independent)
 * and applies the winners; a pass without a move ends the call, and the cost never rises.  The result is a function of the input records and
 * `passes` alone.  It replaces the tree on the device (hj_scene_upload* with scene->bvh == NULL takes it over, hj_bvh_device_read
 * copies it out; the shape arrays kept with the tree stay): a valid pre-order skip-link array of the same records, record 0 the
 * root, every leaf's box bit for bit what it was, every inner box the union of its two children's, the root's exit by
 * hj_build_bvh_device's rule.  scene != NULL (its shape counts must be the tree's): the call ends with the ray-voted child order
 * over the new tree, as the build does (camera, materials and emitters of `scene`, HJ_LBVH_VOTE_PATHS paths; a moved parent holds
 * its children in the order (new sibling, moved node)); scene == NULL: no vote.  out_cost_before / out_cost_after: the surface-area
 * cost (hj_refit_bvh_device's out_cost) of the input and of the final records; out_moves: subtrees moved, summed over the passes.
 * passes == 0, a tree of fewer than 7 records, or a first pass without a move: HJ_OK, the tree untouched, both costs equal.
 * Refused, the tree on the device left as it was: passes > 64 or a node buffer that is too small (HJ_ERR_INVALID), a null context,
 * a frame in flight, no tree on the device (HJ_ERR_STATE), a scene with other shape counts (HJ_ERR_INVALID).  A device failure
 * midway leaves no tree on the device, as a failed refit does.  A call that moved something also drops the links
 * hj_refit_bvh_device kept: they are the old topology's, so the next refit must bring one (scene->bvh = the optimised records;
 * with scene->bvh == NULL it is refused with HJ_ERR_STATE). */
int hj_optimize_bvh_device(hj_context* ctx, const hj_scene_desc* scene /* may be NULL */, uint32_t passes,
                           hj_bvh_node* out_nodes /* may be NULL */, size_t capacity, size_t* out_num_nodes /* may be NULL */,
                           double* out_cost_before /* may be NULL */, double* out_cost_after /* may be NULL */,
                           uint32_t* out_moves /* may be NULL: subtrees moved, summed over the passes */);

/* The uploaded scene's shapes moved IN PLACE (ABI 0.7): the frame loop of an animation becomes "move the shapes,
 * hj_scene_update_shapes, render" - no refit + upload, no re-layout, no allocation after the first call.
 * `scene` carries the shapes as they are NOW: spheres, quads, vertices, emitters (pdf and cdf change with area) and camera; every
 * count equals the uploaded scene's.  bvh, triangles, materials and the material tables are NOT read: the uploaded scene's links,
 * index triples, materials, textures and environment stay.  Afterwards the scene is what hj_scene_upload* would render from these
 * shapes with the uploaded topology and refitted boxes: a leaf's box is its shape's, an inner node's the union of its two
 * children's (hj_refit_bvh_device's pass), guard boxes follow the upload's formula from the moved shape and the new root box joined
 * with the camera, the pre-gathered triangle, pair and emitter records are gathered again.  Which nodes the upload collapsed, paired
 * or called hot, where the records lie, root, root2, num_hot and the tuning fields do not change ("Refit").
 * flags: HJ_UPDATE_DEVICE_ARRAYS - scene->spheres / quads / vertices are DEVICE pointers on the context's device, read on the
 * context's stream (the caller has finished writing them; no host copy is made unless a light-shaft grid is rebuilt);
 * HJ_UPDATE_NO_LIGHT_GRID - a scene that has a light-shaft grid loses it instead of getting a new one (same image, no next-event
 * sample proven free).  The old grid is never kept: its proofs are about the old geometry.
 * out_cost (may be NULL): as hj_refit_bvh_device's.
 * Refused before anything of the scene is written - the previous frame still renders bit for bit -: no scene (HJ_ERR_STATE); null
 * arguments, other counts, unknown flag bits, a coordinate, radius or camera field that is not finite, an emitter whose shape is
 * out of range or not emissive (HJ_ERR_INVALID); an uploaded tree that is not one leaf per shape - among them a scene uploaded
 * without a tree (num_bvh_nodes == 0, rendered by linear scan) and a scene of a single shape, which have no boxes to refit: upload
 * those again - (HJ_ERR_UNSUPPORTED); a frame in
 * flight (HJ_ERR_STATE, as for an upload).  After those checks only a device error can fail; the context is then without a scene,
 * as after a failed upload.  The call neither reads nor changes the tree hj_build_bvh_device / hj_refit_bvh_device left on the
 * device, nor the refit's kept links: it owns the uploaded topology's link set, derived at the first update and kept with the scene. */
#define HJ_UPDATE_DEVICE_ARRAYS 1u
#define HJ_UPDATE_NO_LIGHT_GRID 2u
int hj_scene_update_shapes(hj_context* ctx, const hj_scene_desc* scene, uint32_t flags, double* out_cost /* may be NULL */);
/* Probe: the device node array (8 floats per record, capacity_records of room; NULL: only info), info = num_nodes, root, root2,
 * num_hot, and (map != NULL) per node i of the uploaded array - num_nodes - root2 of them - two words: its record in the
 * re-laid-out copy and its guard's record, 0xFFFFFFFF for none.  Record root2 + i is node i in the second copy. */
int hj_debug_scene_tree(hj_context* ctx, float* records /* may be NULL */, size_t capacity_records, uint32_t info[4], uint32_t* map /* may be NULL */);

/* The child order of a flattened tree, voted by a sample of the scene's own rays - on the device (no counterpart upstream: the
 * reference walks the tree the `bvh` crate hands it, src/main.rs:199-231, children in array order, shader/scene.glsl:97-133; host
 * form of the same pass: hjh_compiled_tune_bvh).  `vote_paths` camera paths of `scene` (camera, materials, emitters) are traced
 * through scene->bvh; every ray that hits votes, at the ancestors of its leaf, for the order that would have spared it more of
 * the other child; where the sample says so the two children of a node change places.  out_nodes receives the same tree - same
 * boxes, same leaves - as another valid pre-order skip-link array of scene->num_bvh_nodes records (60 000 paths: a few
 * milliseconds at 1 M triangles).  hj_build_bvh_device ends with this pass (HJ_LBVH_VOTE_PATHS, default 60000, 0 = off).  Images
 * change only through epsilon-ties, traversal cost falls. */
int hj_tune_bvh_device(hj_context* ctx, const hj_scene_desc* scene, hj_bvh_node* out_nodes, size_t capacity, size_t vote_paths);

/* ------------------------------------------------- asynchronous frame, progress */

/* hj_render_frame on the context's worker thread (one persistent thread per context, started by the first call):
 * returns at once, hj_sync waits for the frame and returns its status and statistics.  One host thread can so keep one
 * context per GPU rendering at the same time, and the drain of one context overlaps whatever the host does next (the
 * reduce waits for all of them).  At most one frame in flight per context: until it has finished every other entry
 * point that touches the context's device state (scene upload, framebuffer create / clear / read / resolve, the render
 * calls, the probes, hj_build_bvh_device) returns HJ_ERR_STATE.  The result of the last asynchronous frame stays
 * retrievable - hj_sync after hj_comm_reduce_framebuffers, which joins the frames itself, still returns the statistics -
 * until the next hj_render_frame_async; hj_sync on a context that never ran one returns HJ_OK and leaves *stats alone.
 * (No counterpart in the reference, whose submit loop src/main.rs:1316-1355 is synchronous with respect to the host but
 * never waits for the device.) */
int hj_render_frame_async(hj_context* ctx, uint32_t spp, uint64_t master_seed,
                          uint32_t pass_begin, uint32_t pass_end, uint32_t rank, uint32_t world,
                          const hj_render_opts* opts);
int hj_sync(hj_context* ctx, hj_render_stats* stats /* may be NULL */);

/* Frames BACK TO BACK without draining the batch pipeline between them.  (Upstream the queue never drains either: render()
 * submits one command buffer per block and never waits, src/main.rs:1341-1347; a blocking hj_render_frame ends with the
 * path-depth tail of its last batches running alone - 3 ms of a 160 ms frame on one GPU, of a 20 ms share on eight.)
 *   hj_render_frame(..., opts->flags | HJ_RENDER_NO_DRAIN, stats = NULL)
 *       returns when the frame's batches are enqueued; it blocks only while all batch slots are still busy with EARLIER
 *       batches (the natural back-pressure).  The frame accumulates into the framebuffer that is bound at the time of the
 *       call; it must have been zeroed (or hold what the frame is to be added to) before the call.
 *   hj_framebuffer_bind(ctx, device_ptr)
 *       frames submitted from now on accumulate into this caller-owned W x H RGBA32F buffer (16-byte aligned; same size as the
 *       one hj_framebuffer_create was given) - no synchronisation, frames already submitted keep their buffer: two buffers in
 *       turn let frame k + 1 render while frame k is reduced / read.
 *   hj_pipeline_wait(ctx, keep, totals)
 *       waits until at most `keep` of the submitted frames are still in flight (oldest first).  keep = 0 drains everything
 *       and returns in *totals (may be NULL) the statistics of ALL frames since the last drain (times: kernels of all of
 *       them); with keep > 0 *totals is left alone.
 * While frames are in flight the other entry points that touch the context's device state return HJ_ERR_STATE (as with an
 * asynchronous frame), except hj_framebuffer_bind and hj_framebuffer_device_ptr.  Results are the blocking call's, bit for bit. */
int hj_framebuffer_bind(hj_context* ctx, void* external_device_ptr);
int hj_pipeline_wait(hj_context* ctx, uint32_t keep, hj_render_stats* totals /* may be NULL */);

/* Replaces the window-title percentage the reference updates every `present_interval` blocks (src/main.rs:1335-1340):
 * `fn(user, blocks_done, blocks_total)` is called from the thread that drives the render whenever at least
 * `interval_blocks` more ImageBlocks have COMPLETED on the device (granularity: one wavefront batch), and once at the
 * end of the call.  fn == NULL switches reporting off. */
typedef void (*hj_progress_fn)(void* user, uint64_t blocks_done, uint64_t blocks_total);
void hj_set_progress_callback(hj_context* ctx, hj_progress_fn fn, void* user, uint32_t interval_blocks);

/* Number of HIP devices visible to the process (0 without a GPU). */
int hj_device_count(void);

/* ---------------------------------------------------------------- multi-GPU */

/* New with the multi-GPU tile sharding (no counterpart in the reference).  A communicator holds the `n` contexts of
 * THIS process (one per GPU) and their RCCL communicators (ncclCommInitAll once, reused by every reduce; RCCL is loaded
 * with dlopen on first use, a copy the process has already mapped is reused; n == 1 needs no RCCL). */
typedef struct hj_comm hj_comm;
int hj_comm_create(hj_context* const* ctxs, int n, hj_comm** out_comm);
void hj_comm_destroy(hj_comm* comm);
/* Element-wise SUM of the framebuffers (equal sizes) into ctxs[root]: waits for frames in flight (hj_sync) on every
 * context, then one ncclReduce per GPU inside a group call over xGMI.  Resolve rgb/w only after the reduce.  Errors
 * are reported on ctxs[root].  Hosts that run one process per GPU reduce the external framebuffer themselves instead
 * (hijiki_amd/dist.py does, through torch.distributed). */
int hj_comm_reduce_framebuffers(hj_comm* comm, int root);
/* The same without a communicator object: the communicators of the context list are created on the first call and
 * kept until one of the contexts is destroyed. */
int hj_reduce_framebuffers(hj_context* const* ctxs, int n, int root);

/* -------------------------------------------------------------- ray queries */

/* hj_trace_rays (ABI 0.10): caller-given rays through the uploaded scene's tree, by the path kernel's own walk (no counterpart in
 * the reference; intersectScene, shader/scene.glsl:92-175, per ray).
 *   rays: n x 8 floats (origin.xyz, direction.xyz, tMin, tMax) - hj_debug_trace's layout; directions of any length.
 *   hits: n x 4 floats (objectID as int32 bits or -1, t, u, v of the raw hit; a miss: -1, 0, 0, 0).
 *   surface (may be NULL): n x 16 floats per ray - p.xyz, n.xyz, u, v, ft.xyz, fb.xyz (the populated intersection: hit point
 *     fma(t, d, o), shading normal, texture coordinates, tangent frame), [14] = the hit shape's material word (tag << 24 | index)
 *     as uploaded, [15] = 0; all 16 words 0 for a miss.
 *   HJ_TRACE_ANY_HIT: the walk stops at the first accepted hit in its visiting order (the shadow-ray form): only `objectID >= 0`
 *     is the reference's answer; the record is still a function of ray and tree alone.  No surface with it.
 *   HJ_TRACE_DEVICE_ARRAYS: rays / hits / surface are device pointers on the context's GPU, 16-byte aligned, read and written in
 *     place (the caller orders its own streams before the call).  Without it they are host arrays, staged through buffers the
 *     context keeps.
 * The tree is always walked (there is no linear-scan form).  Runs on the context's stream and returns when the results are complete;
 * record i depends on ray i and the scene alone.  n == 0: HJ_OK, nothing touched.
 * Origin domain: agreement with the reference bit for bit is claimed for origins within the scene's extent of it - hj_trace_paths below says why.
 * HJ_ERR_INVALID: null rays or hits, unknown flag bits, n above 2^31 - 1, surface together with HJ_TRACE_ANY_HIT, misaligned
 *   device arrays - checked before anything else, without a device; with a null context the text is in hj_last_error(NULL).
 * A null context: HJ_ERR_DEVICE in a process without a HIP device (which cannot hold a context), HJ_ERR_INVALID otherwise.
 * HJ_ERR_STATE: no scene, an asynchronous frame in flight, frames submitted with HJ_RENDER_NO_DRAIN not yet drained. */
#define HJ_TRACE_ANY_HIT 1u
#define HJ_TRACE_DEVICE_ARRAYS 2u
int hj_trace_rays(hj_context* ctx, const float* rays, size_t n, uint32_t flags, float* hits, float* surface);

/* ------------------------------------------------------------- path queries */

/* hj_trace_paths (ABI 0.12): the path-traced radiance that arrives along caller-given rays - integrateRay (shader/render.glsl:81-147)
 * per ray instead of per camera pixel; no counterpart in the reference.  For light-map and probe baking, radiance caches, sensors
 * that are no pinhole camera.
 *   rays: n x 8 words per ray - words 0-2 the origin, 3-5 the direction (used as given, never normalised, as the reference uses a
 *     ray's), word 6 a uint32 seed stored as bits, word 7 reserved and ignored.  The first six words are hj_trace_rays' layout.
 *   spp: samples per ray, 1 ... 65536.  Sample k of ray i starts exactly as a camera path does (render.glsl:86-90,156): RNG state
 *     seedRng(seed_i + k) with uint32 wrap-around, throughput 1, extinction 0, wasDiscrete, bounce 0, first segment tMin = eps and
 *     tMax = inf; later segments as integrateRay continues them.  So a block's camera rays with seed = block.seed + lx + ly *
 *     dimension.x give hj_debug_samples' records.
 *   samples: n x 8 floats per ray in hj_debug_samples' layout - rgb = the float32 sum over k = 0, 1, ... in that order of the samples'
 *     radiance, starting from +0; [3] = (float)spp; [4..7] = the first hit's shading normal and t (the same for every k; all zero
 *     for a miss).  Record i depends on ray i, spp, opts and the scene alone: not on the workgroup count, the pool or chunk size
 *     (HJ_PATHS_WGS, HJ_PATHS_POOL, HJ_PATHS_CHUNK, read when the context is created), nor on which lane carried the path.
 *   opts (NULL: the defaults): max_bounces, rr_start and HJ_RENDER_NO_LIGHT_GRID mean what they mean in a render call; use_bvh == 0 is
 *     HJ_ERR_UNSUPPORTED (the tree is always walked, as in hj_trace_rays); any other HJ_RENDER_* bit is HJ_ERR_INVALID; the
 *     reconstruction fields and batch_blocks are ignored.
 *   stats (may be NULL): paths (= n * spp), closest_rays, shadow_rays, hits, unoccluded_shadow_rays, shadow_rays_proven_free, batches
 *     (= launches of the path kernel) and total_ms; every other field 0.
 *   HJ_PATHS_DEVICE_ARRAYS: rays and samples are device pointers on the context's GPU, 16-byte aligned, read and written in place on the
 *     context's stream (the caller orders its own streams before the call).  Without it they are host arrays, staged through buffers
 *     the context keeps.
 * The query owns its path state (about 250 bytes per position in flight, at most HJ_PATHS_WGS x HJ_PATHS_POOL = 2048 x 2048 positions =
 * 1 GB at the defaults, plus 32 bytes per sample of a launch, at most 2^22), kept with the context; it borrows nothing of the batch
 * slots: a query between two frames leaves them and the framebuffer alone.  Returns when the results are complete.  n == 0: HJ_OK,
 * nothing touched.
 * Origin domain: the uploaded tree's leaf guards are padded for ray origins inside the scene's root box joined with the camera (2e-4
 *   for scenes up to 50 units, 4e-6 of the extent beyond).  Agreement with the reference bit for bit is claimed for origins within
 *   that extent of the scene; a caller whose rays start farther away uploads under HJ_LEAF_GUARDS=0 (no guards: the reference's own
 *   leaf tests, slower).  hj_trace_rays has the same limit.
 * HJ_ERR_INVALID, checked before anything else and without a device (with a null context the text is in hj_last_error(NULL)): null
 *   rays or samples with n > 0, unknown flag bits, spp == 0 or above 65536, n above 2^31 - 1, misaligned device arrays, max_bounces
 *   == 0 (and the refusals of opts above).  A null context: HJ_ERR_DEVICE in a process without a HIP device, HJ_ERR_INVALID otherwise.
 * HJ_ERR_STATE: an asynchronous frame in flight, frames submitted with HJ_RENDER_NO_DRAIN not yet drained, no scene.  A refused call
 *   writes nothing. */
#define HJ_PATHS_DEVICE_ARRAYS 1u
int hj_trace_paths(hj_context* ctx, const float* rays, size_t n, uint32_t spp, const hj_render_opts* opts /* NULL = defaults */,
                   uint32_t flags, float* samples, hj_render_stats* stats /* may be NULL */);

/* hj_trace_paths_adaptive (ABI 0.13): hj_trace_paths with the number of samples decided per ray, on the device - for baking, where most
 * rays converge in a handful of samples and a minority needs many.  rays, samples, flags (HJ_PATHS_DEVICE_ARRAYS), opts and the origin
 * domain are exactly hj_trace_paths'; no counterpart in the reference.
 *   Rounds.  Round 0 gives every ray spp_min samples; round r >= 1 gives every ray that is still active min(spp_step, spp_max - n_i)
 *     samples, n_i being the samples ray i has had, with the sample index k continuing at n_i (sample k starts from seedRng(seed_i + k),
 *     as in hj_trace_paths).  1 + ceil((spp_max - spp_min) / spp_step) rounds at most, and at most 64.
 *   Running sums per ray, all float32, from +0, in ascending k, uncontracted, continued from round to round (never re-associated as
 *     per-round partial sums):  R += r; G += g; B += b;  Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;  S1 += Y;  S2 += Y * Y.
 *   Stop rule, evaluated after each round with m = n_i (float32, in this order, divisions correctly rounded, max = fmaxf):
 *       mean = S1 / (float)m;   var = max(0, S2 - S1 * mean) / (float)(m - 1);   sem2 = var / (float)m;
 *       thr = rel_error * max(mean, floor);   ray i stops when sem2 <= thr * thr or n_i == spp_max
 *     - the standard error of the mean luminance is at most rel_error * max(mean luminance, floor).  A NaN sem2 compares false: such a
 *     ray stops only at spp_max.  Stopping on a ray's own samples biases its estimate (rays stop more readily while their samples
 *     happen to be dark and alike); spp_min and floor bound that, rel_error = 0 removes it (every ray gets spp_max).
 *   samples: n x 8 floats, hj_trace_paths' record with [3] = (float)n_i.  Record i is bit for bit what hj_trace_paths returns for ray i
 *     with spp = n_i; it depends on ray i, the adaptive opts, opts and the scene alone.
 *   moments (may be NULL): n x 4 floats - S1, S2, the sem2 of the last evaluation, n_i as uint32 bits.
 *   stats (may be NULL): paths = the sum of n_i; closest_rays, shadow_rays, hits, unoccluded_shadow_rays, shadow_rays_proven_free summed
 *     over all launches; batches = launches of the path kernel; bounce_rounds = adaptive rounds run; total_ms; every other field 0.
 * Beside hj_trace_paths' path state the context keeps, per ray of the largest call, 64 bytes (running sums, flags, two index lists,
 * the next round's rays); host arrays are staged whole, once per call (80 bytes per ray more).  The call synchronises once per round.
 * HJ_ERR_INVALID, checked before anything else and without a device, in hj_trace_paths' order: what hj_trace_paths refuses of rays,
 *   samples, flags, n and opts; null adaptive opts, spp_min < 2, spp_step == 0, spp_max < spp_min, spp_max > 65536, a rel_error or
 *   floor that is NaN, negative or infinite, more than 64 rounds, misaligned moments with device arrays.  The null context,
 *   HJ_ERR_STATE and n == 0 as in hj_trace_paths.  A refused call writes nothing. */
typedef struct hj_adaptive_opts {
  uint32_t spp_min;    /* samples of the first round, >= 2                                   */
  uint32_t spp_step;   /* samples of every later round, >= 1                                 */
  uint32_t spp_max;    /* a ray never gets more; spp_min <= spp_max <= 65536                 */
  float    rel_error;  /* stop when the standard error of the mean luminance is at most      */
  float    floor;      /*   rel_error * max(mean luminance, floor); both finite, >= 0        */
} hj_adaptive_opts;
int hj_trace_paths_adaptive(hj_context* ctx, const float* rays, size_t n, const hj_adaptive_opts* adaptive, const hj_render_opts* opts /* NULL = defaults */,
                            uint32_t flags, float* samples, float* moments /* may be NULL */, hj_render_stats* stats /* may be NULL */);

/* hj_trace_irradiance (ABI 0.14): the radiance gathered at caller-given points, over the hemisphere about a normal or over the
 * sphere - the query of a light-map texel or a probe.  The directions are drawn on the device from the call's own RNG, so a record is
 * reproducible; no counterpart in the reference.  opts, stats and the path state are exactly hj_trace_paths'.
 *   points: n x 8 words per point - words 0-2 the position, 3-5 the normal (used as given, never normalised, as hj_trace_paths uses
 *     its directions), word 6 a uint32 seed stored as bits, word 7 reserved and ignored.  Words 0-2 and word 6 sit where
 *     hj_trace_rays and hj_trace_paths have origin and seed.
 *   spp: samples per point, 1 ... 65536.  Sample k of point i: RNG state s = seedRng(seed_i + k) with uint32 wrap-around; two draws
 *     give the direction d_k,
 *       default (hemisphere): l = randCosHemisphere(s) in populateTriangle's frame about the normal n (shader/shapes/triangle.glsl):
 *           bt = |n.x| > |n.y| ? (0,1,0) : (1,0,0);  t = normalize(cross(n, bt));  b = cross(n, t);  d = (t * l.x + b * l.y) + n * l.z
 *         - the expression of a diffuse bounce (material.glsl:37-46), in the numeric contract's cross and normalize;
 *       HJ_GATHER_SPHERE: d = randUniformSphere(s); the normal is ignored.
 *     A path then starts at (position_i, d_k) exactly as a sample of hj_trace_paths does, with the RNG state CONTINUED behind the two
 *     draws and not reseeded: throughput 1, extinction 0, wasDiscrete, bounce 0, first segment tMin = eps and tMax = inf.  No
 *     next-event sample is taken at the gather point; a light the gather ray hits counts through wasDiscrete.  L_k: its radiance.
 *   out: n x 8 floats per point, n x 36 with HJ_GATHER_SH9 -
 *     [0..2] the float32 sum of L_k over k = 0, 1, ... in that order, starting from +0;  [3] (float)spp;
 *     [4] the number of samples whose first segment hit something (first-hit t > 0), as a float;
 *     [5] the smallest first-hit t among those samples, +inf if there is none;  [6], [7] zero.
 *     Irradiance is pi / spp x [0..2] (hemisphere), ambient occlusion [4] / spp.
 *     HJ_GATHER_SH9 (only together with HJ_GATHER_SPHERE): [8 + 3 j + c] is the running float32 sum over ascending k, from +0, of
 *     Y_j(d_k) * L_k[c] - one multiply, then one add, no contraction; [35] zero.  d_k = (x, y, z) as drawn, not renormalised.  The
 *     real spherical-harmonic basis of bands 0..2, float32, in this order and operation order:
 *         Y_0 = c0            Y_1 = c1 * y                          Y_2 = c1 * z            Y_3 = c1 * x
 *         Y_4 = c2 * (x * y)  Y_5 = c2 * (y * z)                    Y_6 = c3 * ((3.0f * z) * z - 1.0f)
 *         Y_7 = c2 * (x * z)  Y_8 = c4 * (x * x - y * y)
 *         c0 = 0x1.20dd76p-2f  c1 = 0x1.f45438p-2f  c2 = 0x1.17b142p+0f  c3 = 0x1.42f602p-2f  c4 = 0x1.17b142p-1f
 *         (0.28209479, 0.48860252, 1.0925485, 0.31539157, 0.54627424)
 *     Record i depends on point i, spp, flags, opts and the scene alone: not on HJ_PATHS_WGS, HJ_PATHS_POOL or HJ_PATHS_CHUNK, nor on
 *     which lane carried a path.
 *   HJ_GATHER_DEVICE_ARRAYS: points and out are device pointers on the context's GPU, 16-byte aligned, read and written in place on
 *     the context's stream (the caller orders its own streams before the call).  Without it they are host arrays, staged through
 *     buffers the context keeps.
 *   HJ_GATHER_INDIRECT (ABI 0.33): the INDIRECT-only gather.  A path starts with wasDiscrete clear - its flags word is 0u where a
 *     full gather's is 1u, bounce 0 - and everything else is unchanged: the directions, the RNG states, the first tMin, the records,
 *     the hit count, the nearest t.  So a first segment that ends on an emitter adds nothing and ends; a first segment that leaves
 *     into an uploaded environment adds nothing; from the first diffuse hit on the path is the integrator's, next-event samples
 *     included.  What such a gather leaves out is exactly the light that reaches the point directly.  Bit 8u is reserved and stays
 *     refused as an unknown flag bit.
 * A launch takes whole points (at most HJ_PATHS_CHUNK samples; one point when spp alone exceeds it); the path state is
 * hj_trace_paths' own, kept with the context.  Returns when the results are complete (one synchronisation).  n == 0: HJ_OK, nothing
 * touched.
 * Origin domain: hj_trace_paths' - agreement with the reference's arithmetic bit for bit is claimed for positions inside the scene's
 *   root box joined with the camera (the leaf guards' padding; HJ_LEAF_GUARDS=0 beyond).
 * Normals: in hemisphere mode a normal must be finite and not all zero (the frame normalises cross(n, bt)).  With host arrays the call
 *   checks every point before anything is written; with HJ_GATHER_DEVICE_ARRAYS that is the caller's contract, as the directions of
 *   hj_trace_paths are.
 * HJ_ERR_INVALID, checked before anything else and without a device, in hj_trace_paths' order: null points or out with n > 0, unknown
 *   flag bits, HJ_GATHER_SH9 without HJ_GATHER_SPHERE, spp == 0 or above 65536, n above 2^31 - 1, misaligned device arrays, the
 *   refusals of opts, a bad normal in host arrays.  The null context, HJ_ERR_STATE and n == 0 as in hj_trace_paths.  A refused call
 *   writes nothing. */
#define HJ_GATHER_DEVICE_ARRAYS 1u
#define HJ_GATHER_SPHERE 2u
#define HJ_GATHER_SH9 4u   /* only together with HJ_GATHER_SPHERE */
#define HJ_GATHER_INDIRECT 16u   /* the first segment's emission is left out (8u is reserved: refused) */
int hj_trace_irradiance(hj_context* ctx, const float* points, size_t n, uint32_t spp, const hj_render_opts* opts /* NULL = defaults */,
                        uint32_t flags, float* out, hj_render_stats* stats /* may be NULL */);

/* hj_lightmap_texels (ABI 0.16): the uploaded scene's triangle UVs rasterised into gather points, on the device - from "uploaded
 * scene" to the `points` of hj_trace_irradiance without a trip through the host.  Reads the triangles and the hj_vertex records the
 * scene was uploaded with (u, v, pos, normal; hj_scene_update_shapes rewrites them).  No counterpart in the reference.
 * Every arithmetic operation below is float32, one rounding per operation, no contraction; vector operations are the numeric
 * contract's (cross, normalize, v * s, v + v of kernels/hj_num.h: DESIGN.md 3); division is IEEE `/`.
 *   Texel t = y * width + x has its centre at p = (((float)x + 0.5f) / (float)width, ((float)y + 0.5f) / (float)height).
 *   Triangle i has vertex uv a, b, c (hj_vertex::u / v of its three vertices, not wrapped).  With
 *       edge(s, t, p) = (t.u - s.u) * (p.v - s.v) - (t.v - s.v) * (p.u - s.u)
 *       e0 = edge(b, c, p)   e1 = edge(c, a, p)   e2 = edge(a, b, p)   s = (e0 + e1) + e2
 *   triangle i COVERS the texel when all six uv are finite; min(a.u, b.u, c.u) <= p.u <= max(a.u, b.u, c.u) and the same in v (exact
 *   comparisons: the closed box); (e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0) - both windings count -; and
 *   s != 0 - a zero-area footprint covers nothing.
 *   The OWNER of a texel is the lowest covering triangle index in [first_triangle, first_triangle + num_triangles).  For the owner:
 *       hu = e1 / s   hv = e2 / s   l0 = (1.0f - hu) - hv
 *       P = (A.pos * l0 + B.pos * hu) + C.pos * hv
 *       n = normalize((A.normal * l0 + B.normal * hu) + C.normal * hv)              (populateTriangle's expressions)
 *   A texel whose n has a non-finite component, or is all zero, has NO owner: the call never emits a normal that the hemisphere
 *   gather could not build its frame about.  The emitted position is P + n * offset.
 *   points (may be NULL: the call only counts): the owned texels in ascending t, 8 words each - 0-2 the position, 3-5 the normal,
 *     6 the seed seed + t * seed_stride (uint32 wrap-around) as bits, 7 t as uint32 bits.  Word 7 is the word hj_trace_irradiance
 *     ignores: the array is a valid `points` argument as it stands and carries its own scatter address.
 *   owner (may be NULL): width * height words, the owning triangle index or 0xFFFFFFFF.
 *   *out_count: the number of owned texels, written whenever the call returns HJ_OK - and when capacity_points is below it: the call
 *     then returns HJ_ERR_INVALID and writes nothing else.
 *   HJ_LIGHTMAP_DEVICE_ARRAYS: points and owner are device pointers on the context's GPU, 16-byte aligned, written on the context's
 *     stream; the call returns after one synchronisation.  Without it they are host arrays.
 *   The result depends on the scene and the desc alone: not on HJ_LIGHTMAP_LANE_TEXELS or HJ_LIGHTMAP_SLICES, nor on any launch shape.
 * The owner map (4 bytes a texel) and the scan's counts are kept with the context, grown on demand.
 * HJ_ERR_INVALID, checked before anything else and without a device (with a null context the text is in hj_last_error(NULL)): a null
 *   desc or out_count, unknown flag bits, width or height outside [1, 16384] or width * height above 2^26, a non-finite offset,
 *   misaligned device arrays; then, with the scene at hand, a triangle range beyond the scene's triangles.  A null context:
 *   HJ_ERR_DEVICE in a process without a HIP device, HJ_ERR_INVALID otherwise.  HJ_ERR_STATE: an asynchronous frame in flight, frames
 *   submitted with HJ_RENDER_NO_DRAIN not yet drained, no scene.  No triangle in range: HJ_OK and a count of 0.  A refused call
 *   writes nothing. */
#define HJ_LIGHTMAP_DEVICE_ARRAYS 1u
typedef struct hj_lightmap_desc {
  uint32_t width, height;      /* the atlas: 1 ... 16384 each, width * height <= 2^26                      */
  uint32_t first_triangle;     /* index into the scene's triangle array                                    */
  uint32_t num_triangles;      /* 0 = all from first_triangle to the end                                   */
  uint32_t seed, seed_stride;  /* texel t gets seed + t * seed_stride (uint32 wrap-around)                 */
  float    offset;             /* the position is moved by normal * offset; finite                         */
  uint32_t flags;              /* HJ_LIGHTMAP_DEVICE_ARRAYS                                                */
} hj_lightmap_desc;
int hj_lightmap_texels(hj_context* ctx, const hj_lightmap_desc* desc, float* points /* may be NULL */, size_t capacity_points,
                       uint32_t* owner /* may be NULL */, size_t* out_count);

/* hj_bake_lightmap (ABI 0.16): from the uploaded scene to the atlas image - hj_lightmap_texels, the hemisphere gather of
 * hj_trace_irradiance over its points, and the records scattered into an image - without the points leaving the device.
 *   1. The texels of desc, as hj_lightmap_texels emits them, into a buffer the context keeps.
 *   2. hj_trace_irradiance over them (hemisphere mode, device arrays), spp samples each, with opts.
 *   3. scale = 3.14159274f / (float)spp.  A texel with a record is (sum.r * scale, sum.g * scale, sum.b * scale, 1.0f) - its
 *      irradiance, alpha 1 -, every other texel (0, 0, 0, 0).
 *   4. `gutter` dilation passes (0 ... 64), each from one image into another: a texel with alpha == 0 in the pass's input and at
 *      least one 8-neighbour with alpha > 0 becomes (sum / (float)k, 0.5f): sum the float32 sum from +0 of those neighbours' rgb
 *      in the order dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, k their number, one division per channel; neighbours outside the
 *      atlas do not exist; every other texel is copied.
 *   image: width * height * 4 floats, row y = 0 first - a host array, or with HJ_LIGHTMAP_DEVICE_ARRAYS a 16-byte-aligned device
 *     pointer.  *out_count (may be NULL): the texels that had a record.  stats (may be NULL): the gather's (all zero when there is
 *     no texel to gather at).
 * spp and opts have hj_trace_irradiance's domain and refusals.  The context keeps, beside hj_lightmap_texels' buffers, 64 bytes per
 * owned texel (points and records) and up to two images.
 * HJ_ERR_INVALID, before anything else and without a device: what hj_lightmap_texels refuses of desc, a null image, spp == 0 or
 *   above 65536, gutter above 64, a misaligned device image, the refusals of opts.  Context, state and the triangle range as in
 *   hj_lightmap_texels.  A refused call writes nothing. */
#define HJ_LIGHTMAP_MAX_GUTTER 64u
int hj_bake_lightmap(hj_context* ctx, const hj_lightmap_desc* desc, uint32_t spp, uint32_t gutter, const hj_render_opts* opts /* NULL = defaults */,
                     float* image, size_t* out_count /* may be NULL */, hj_render_stats* stats /* may be NULL */);

/* hj_filter_lightmap (ABI 0.17): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a light-map atlas on the device -
 * the stage between hj_bake_lightmap's raw Monte-Carlo estimate and a usable light map.  A 5 x 5 B3-spline kernel whose taps move
 * apart by powers of two, with edge stops on world position, normal and, optionally, colour, which keep charts that sit side by
 * side in the atlas, and walls that meet in a corner, from bleeding into each other.  No counterpart in the reference.
 *   points: `count` records of 8 words, exactly as hj_lightmap_texels emits them - position in words 0-2, normal in words 3-5, word 7
 *     the texel index t = y * width + x, strictly ascending (word 6 is ignored).  A texel is GUIDED when a point names it; the
 *     image's alpha plays no part in that.
 *   image: width * height * 4 floats, row y = 0 first, read and written.
 *   Every operation is float32 with one rounding and no contraction: no fused multiply-add outside hj_exp.
 *       sq(v) = (v.x * v.x + v.y * v.y) + v.z * v.z                                     (deliberately not the contract's dot3)
 *   Computed on the host, once: ip = sigma_position > 0 ? 1.0f / (sigma_position * sigma_position) : 0.0f; in_ the same of
 *   sigma_normal; ic_0 the same of sigma_color; ic_i = ic_{i-1} * 4.0f (the colour stop halves every iteration).
 *   Iteration i = 0 ... iterations - 1 reads image I, writes image O and uses the step s = 1 << i.  A texel that is not guided is
 *   copied, all four words.  For a guided texel at (x, y) with rgb c in I, position P and normal n: sum = (+0, +0, +0), wsum = +0,
 *   then for dy = -2 ... 2 (outer), dx = -2 ... 2 (inner):
 *     1. the tap is q = (x + dx * s, y + dy * s); it is skipped when it lies outside the atlas or is not guided;
 *     2. h = k[|dx|] * k[|dy|] with k = {0.375f, 0.25f, 0.0625f} (the products are exact);
 *     3. a = (sq(P_q - P) * ip + sq(n_q - n) * in_) + sq(c_q - c) * ic_i;
 *     4. w = h * hj_exp(-a) - the numeric contract's exp (kernels/hj_num.h; HJ_NUM_EXP of hj_debug_num);
 *     5. sum.r = sum.r + c_q.r * w, likewise g and b;   6. wsum = wsum + w.
 *   O.rgb = sum / wsum, one IEEE division per channel; O.a = I.a.  For finite data the centre tap alone gives wsum >= 0.140625.
 *   Agreement bit for bit with that text is claimed for finite images and guides; non-finite values just propagate.
 *   After the last iteration the result is in `image`.  iterations == 0: HJ_OK, nothing touched.  The result depends on (width,
 *   height, points, filter, image) alone: not on HJ_LIGHTMAP_FILTER_LDS_STEP, nor on any launch shape.
 *   HJ_LIGHTMAP_DEVICE_ARRAYS (filter->flags): points and image are device pointers on the context's GPU, 16-byte aligned, read and
 *     written on the context's stream; the call returns after one synchronisation.  The texel indices are then the caller's
 *     contract; a word 7 that is not below width * height names no texel and its point is skipped - it cannot fault.  Without the
 *     flag they are host arrays, checked before anything is written and staged through buffers the context keeps.
 * The context keeps 32 bytes per texel of guide data and one more image, grown on demand, freed with the context.
 * HJ_ERR_INVALID, before anything else and without a device, in this order: a null filter or image, null points with count > 0;
 *   unknown flag bits; iterations above 8; a negative or non-finite sigma; width or height outside hj_lightmap_texels' limits;
 *   count above width * height; misaligned device arrays; with host arrays a texel index that is not strictly ascending or not
 *   below width * height, or a non-finite position or normal.  The null context and HJ_ERR_STATE as in hj_lightmap_texels.  A
 *   refused call writes nothing. */
#define HJ_LIGHTMAP_FILTER_MAX_ITERATIONS 8u
typedef struct hj_lightmap_filter {
  uint32_t iterations;      /* 0 ... 8; iteration i uses the step s = 1 << i                                          */
  float    sigma_position;  /* world units; 0 = this stop is off                                                      */
  float    sigma_normal;    /* on |n_q - n|; 0 = off                                                                  */
  float    sigma_color;     /* on |c_q - c| of the iteration's input; halves every iteration; 0 = off                 */
  uint32_t flags;           /* HJ_LIGHTMAP_DEVICE_ARRAYS                                                              */
} hj_lightmap_filter;
int hj_filter_lightmap(hj_context* ctx, uint32_t width, uint32_t height, const float* points, size_t count, const hj_lightmap_filter* filter,
                       float* image /* width * height * 4, read and written */);

/* hj_bake_lightmap_filtered (ABI 0.17): steps 1-3 of hj_bake_lightmap, then hj_filter_lightmap's iterations over the scattered image
 * with the bake's own points as guides - they never leave the device -, then step 4, the gutter dilation.  With filter == NULL or
 * iterations == 0 it IS hj_bake_lightmap, bit for bit, statistics included (one host routine serves both).  The filter's
 * HJ_LIGHTMAP_DEVICE_ARRAYS bit is ignored: desc->flags says where the image lives.
 * HJ_ERR_INVALID: hj_bake_lightmap's refusals in its order, with the filter's (unknown flag bits, iterations above 8, a negative or
 *   non-finite sigma) between the misaligned device image and the refusals of opts. */
int hj_bake_lightmap_filtered(hj_context* ctx, const hj_lightmap_desc* desc, uint32_t spp, uint32_t gutter, const hj_lightmap_filter* filter /* NULL = none */,
                              const hj_render_opts* opts /* NULL = defaults */, float* image, size_t* out_count /* may be NULL */,
                              hj_render_stats* stats /* may be NULL */);

/* hj_trace_irradiance_adaptive (ABI 0.18): hj_trace_irradiance with the number of samples decided per point, on the device - the gather
 * of a bake whose texels mostly converge in a handful of samples while penumbrae and corners need many.  points, opts, the origin
 * domain and the normal rules are exactly hj_trace_irradiance's; adaptive is hj_trace_paths_adaptive's hj_adaptive_opts with its
 * domain; no counterpart in the reference.
 *   flags: HJ_GATHER_DEVICE_ARRAYS, HJ_GATHER_SPHERE, HJ_GATHER_INDIRECT (as in hj_trace_irradiance).  HJ_GATHER_SH9 is refused.
 *   Rounds.  As in hj_trace_paths_adaptive: round 0 gives every point spp_min samples; round r >= 1 gives every point that is still
 *     active min(spp_step, spp_max - n_i) samples, the sample index k continuing at n_i (sample k of point i starts from
 *     seedRng(seed_i + k) and draws its direction as in hj_trace_irradiance).  At most 64 rounds.
 *   Running state per point, float32, from +0, in ascending k, uncontracted, continued from round to round and never re-associated:
 *     R, G, B, S1, S2 exactly as hj_trace_paths_adaptive gives them (Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b); the number of
 *     samples whose first segment hit something (first-hit t > 0); the minimum (fminf) of those t, starting from +inf.
 *   Stop rule: hj_trace_paths_adaptive's, evaluated after each round with m = n_i - one text serves both queries.  The note on its
 *     bias holds here as there: a point stops more readily while its samples happen to be dark and alike, so a texel in a penumbra
 *     that has seen no light yet may stop dark; spp_min and floor bound that, rel_error = 0 removes it.
 *   out: n x 8 floats in hj_trace_irradiance's layout with [3] = (float)n_i.  Record i is bit for bit what hj_trace_irradiance returns
 *     for point i alone with spp = n_i and the same flags.  It depends on point i, adaptive, flags, opts and the scene alone: not on
 *     HJ_PATHS_WGS, HJ_PATHS_POOL or HJ_PATHS_CHUNK, nor on the other points of the call.
 *   moments (may be NULL): n x 4 words - S1, S2, the sem2 of the last evaluation, n_i as uint32 bits.
 *   stats (may be NULL): as hj_trace_paths_adaptive's - paths = the sum of n_i, bounce_rounds = adaptive rounds run, batches =
 *     launches of the path kernel, the walk's counts summed over all launches, total_ms; every other field 0.
 * Beside hj_trace_paths_adaptive's buffers the context keeps 8 bytes per point (hit count, nearest hit).  One synchronisation per round.
 * HJ_ERR_INVALID, checked before anything else and without a device, in hj_trace_irradiance's order: null points or out with n > 0,
 *   unknown flag bits, HJ_GATHER_SH9; then, where hj_trace_irradiance checks spp, the adaptive refusals of hj_trace_paths_adaptive in
 *   its order (null adaptive opts ... more than 64 rounds); n above 2^31 - 1; misaligned device arrays (moments included); the
 *   refusals of opts; a bad normal in host arrays.  The null context, HJ_ERR_STATE and n == 0 (HJ_OK) as in hj_trace_irradiance.  A
 *   refused call writes nothing. */
int hj_trace_irradiance_adaptive(hj_context* ctx, const float* points, size_t n, const hj_adaptive_opts* adaptive, const hj_render_opts* opts /* NULL = defaults */,
                                 uint32_t flags, float* out, float* moments /* may be NULL */, hj_render_stats* stats /* may be NULL */);

/* hj_bake_lightmap_adaptive (ABI 0.18): hj_bake_lightmap_filtered with step 2 replaced by hj_trace_irradiance_adaptive (hemisphere
 * mode, device arrays) over the context's own point buffer, so that a texel gets the samples its own variance asks for.
 *   3. scale is per texel: a texel with a record is (sum.r * s, sum.g * s, sum.b * s, 1.0f) with s = 3.14159274f / (float)n_i, one
 *      correctly rounded float32 division - the value hj_bake_lightmap computes when n_i == spp.
 *   sample_map (may be NULL): width * height uint32 words, n_i for a texel with a record and 0 elsewhere (the gutter included) - a
 *     host array, or with HJ_LIGHTMAP_DEVICE_ARRAYS a 16-byte-aligned device pointer, as image is.
 *   The filter and the dilation are hj_bake_lightmap_filtered's, unchanged.  stats (may be NULL): the adaptive gather's.
 * With spp_min == spp_max == spp (>= 2) the image, *out_count and every statistic but total_ms and bounce_rounds (1 here: the rounds
 * run) are bit for bit hj_bake_lightmap_filtered's at that spp.
 * HJ_ERR_INVALID: hj_bake_lightmap_filtered's refusals in its order, with the adaptive refusals of hj_trace_paths_adaptive in the
 *   place of spp's and a misaligned device sample map behind the misaligned device image.  A refused call writes nothing. */
int hj_bake_lightmap_adaptive(hj_context* ctx, const hj_lightmap_desc* desc, const hj_adaptive_opts* adaptive, uint32_t gutter,
                              const hj_lightmap_filter* filter /* NULL = none */, const hj_render_opts* opts /* NULL = defaults */, float* image,
                              uint32_t* sample_map /* may be NULL */, size_t* out_count /* may be NULL */, hj_render_stats* stats /* may be NULL */);

/* Irradiance probe volumes (ABI 0.19): a regular grid of probes, each the order-2 spherical-harmonic coefficients of the irradiance at
 * its position as a function of the surface normal, baked from the uploaded scene on the device, and the look-up of such a volume at
 * caller-given points - lighting for what a light map cannot cover: moving objects, meshes without UVs, volumetric effects.  No
 * counterpart in the reference.  Every arithmetic operation below is float32, one rounding per operation, no contraction; vector
 * operations are the numeric contract's (normalize of kernels/hj_num.h: DESIGN.md 3); division is IEEE `/`.
 *   A volume has n = count[0] * count[1] * count[2] probes.  Probe (x, y, z) has the index p = (z * count[1] + y) * count[0] + x and
 *   sits at origin[a] + (float)i_a * spacing[a] in axis a (one product, then one sum).  A probe record is HJ_PROBE_WORDS = 28 words:
 *   [3 j + c] the coefficient of Y_j (hj_trace_irradiance's basis, in its order) for channel c, [27] the validity weight.
 *
 * hj_probe_points: the n gather points of desc in ascending p, 8 words each - 0-2 the position, 3-5 +0 (sphere mode never reads the
 *   normal), 6 the seed seed + p * seed_stride (uint32 wrap-around) as bits, 7 p as uint32 bits: a valid `points` argument of
 *   hj_trace_irradiance as it stands, as hj_lightmap_texels' output is.  Needs a context but no scene.
 *
 * hj_bake_probes: from the uploaded scene to the volume without the points or the gather's records leaving the device.
 *   1. The points of desc, as hj_probe_points emits them, into a buffer the context keeps.
 *   2. hj_trace_irradiance over them with HJ_GATHER_SPHERE | HJ_GATHER_SH9 (device arrays), spp samples each, with opts.
 *   3. s = 12.5663706f / (float)spp - the Monte-Carlo weight of a uniform sphere sample, 4 pi / spp.  Word 3 j + c of probe p is
 *      (sum[8 + 3 j + c] * s) * A_band(j) with A_0 = 3.14159274f (j = 0), A_1 = 2.09439516f (j = 1 ... 3), A_2 = 0.785398185f
 *      (j = 4 ... 8): pi, 2 pi / 3, pi / 4, the convolution with the clamped cosine lobe (Ramamoorthi and Hanrahan 2001).  Word 27 is
 *      1.0f when word 5 of the gather's record - the nearest first hit, +inf if there is none - is >= min_distance, else 0.0f: a probe
 *      that close to a surface most likely sits inside or behind it.
 *   probes: n x 28 floats.  stats (may be NULL): the gather's.  spp and opts have hj_trace_irradiance's domain and refusals, and the
 *   origin domain is the gather's: the bit-for-bit claim holds for probes inside the scene's root box joined with the camera.  The
 *   result depends on the scene, desc, spp and opts alone.  The context keeps 176 bytes per probe (points and records).
 *
 * hj_sample_probes: irradiance at n points from the eight probes around each.  points: n x 8 words in the gather's layout - words 0-2
 *   the position, 3-5 the normal (any length but zero; normalised here), 6-7 ignored.  Needs a context but no scene.
 *   Per axis a, with m = count[a] - 1:
 *       g = (pos[a] - origin[a]) / spacing[a];   g = (g >= 0.0f) ? g : 0.0f  (a NaN becomes 0);   g = (g <= (float)m) ? g : (float)m;
 *       i0 = min((uint32_t)g, m > 0 ? m - 1 : 0);   f = g - (float)i0;   i1 = min(i0 + 1, m);   the weights are 1.0f - f of i0 and f of i1.
 *   The eight corners in the order dz outer, dy, dx inner (d = 0: i0, d = 1: i1), probe q each:
 *       w = ((wx * wy) * wz) * probes[q][27];   a corner with w == 0 is skipped - an invalid probe, the far plane at f == 0 and a
 *       single-plane axis contribute nothing, and a NaN coefficient behind a zero weight cannot leak;
 *       otherwise acc[k] = acc[k] + probes[q][k] * w for k = 0 ... 26, from +0, and wsum = wsum + w, from +0.
 *   wsum == 0: out = (0, 0, 0, 0).  Otherwise c[k] = acc[k] / wsum, nn = normalize(normal), Y_j(nn) hj_trace_irradiance's basis with
 *   its constants and operation order, E[c] = the sum over j = 0 ... 8, ascending, from +0, of c[3 j + c] * Y_j, and
 *   out = (E[0], E[1], E[2], wsum): the irradiance on a surface with that normal, and how much valid weight stood behind it.
 *   No index is formed from a value that has not been clamped: with device arrays nothing in `points` can make the call fault.  The
 *   result depends on (desc, probes, points) alone, not on any launch shape.  Of desc the seeds and min_distance are not used.
 *
 * HJ_PROBES_DEVICE_ARRAYS (desc->flags): every array argument is a device pointer on the context's GPU, 16-byte aligned, read and
 *   written in place on the context's stream; hj_probe_points and hj_sample_probes return after one synchronisation, hj_bake_probes
 *   after the gather's and one more.  Without it they are host arrays, staged through buffers the context keeps (a volume whole, and
 *   48 bytes per sample point); hj_sample_probes then checks before anything is written that every position and normal is finite
 *   and that no normal is all zero - with device arrays that is the caller's contract, and a bad normal gives a NaN, not a fault.
 * HJ_PROBES_INDIRECT_ONLY (desc->flags, ABI 0.33): the calls that gather - hj_bake_probes, hj_update_probes, hj_update_probes_placed -
 *   pass HJ_GATHER_INDIRECT to hj_trace_irradiance, so the volume holds indirect light alone: the volume hj_render_direct_lit is
 *   meant for.  Every other reader of a desc - the look-ups, hj_probe_points, the visibility calls, hj_place_probes (it traces rays
 *   and gathers nothing), hj_distance_field, the lighting of hj_render_probe_lit and hj_render_direct_lit - accepts the bit and
 *   ignores it.  Bit 2u is reserved and stays refused as an unknown flag bit.
 * HJ_ERR_INVALID, checked before anything else and without a device (with a null context the text is in hj_last_error(NULL)), in
 *   this order: a null desc or array argument (hj_sample_probes: only with n > 0); unknown flag bits; a count outside [1, 1024] or
 *   a product above 2^22; a non-finite origin; a spacing that is not finite or not > 0; a min_distance that is negative or not
 *   finite; then spp == 0 or above 65536; misaligned device arrays; the refusals of opts; n above 2^31 - 1; a bad position or normal
 *   in host arrays.  A null context: HJ_ERR_DEVICE in a process without a HIP device, HJ_ERR_INVALID otherwise.  HJ_ERR_STATE: an
 *   asynchronous frame in flight, frames submitted with HJ_RENDER_NO_DRAIN not yet drained, and for hj_bake_probes no scene.
 *   hj_sample_probes with n == 0: HJ_OK, nothing touched.  A refused call writes nothing.
 * Not here: no adaptive probe bake (hj_trace_irradiance_adaptive refuses HJ_GATHER_SH9).  The weights against light leaks - back face and
 *   visibility (Chebyshev) - are hj_sample_probes_visible's, below; hj_sample_probes itself knows the min_distance rule alone. */
#define HJ_PROBES_DEVICE_ARRAYS 1u
#define HJ_PROBES_INDIRECT_ONLY 4u   /* the bakes and updates gather with HJ_GATHER_INDIRECT (2u is reserved: refused) */
#define HJ_PROBE_WORDS 28u
typedef struct hj_probe_desc {
  float    origin[3];          /* probe (0,0,0); finite                                              */
  float    spacing[3];         /* finite, > 0                                                        */
  uint32_t count[3];           /* 1 ... 1024 each, product <= 2^22                                   */
  uint32_t seed, seed_stride;  /* probe p gets seed + p * seed_stride (uint32 wrap-around)           */
  float    min_distance;       /* finite, >= 0: a probe with a first hit nearer than this is invalid */
  uint32_t flags;              /* HJ_PROBES_DEVICE_ARRAYS, HJ_PROBES_INDIRECT_ONLY                   */
} hj_probe_desc;
int hj_probe_points(hj_context* ctx, const hj_probe_desc* desc, float* points /* n x 8 */);
int hj_bake_probes(hj_context* ctx, const hj_probe_desc* desc, uint32_t spp, const hj_render_opts* opts /* NULL = defaults */,
                   float* probes /* n x 28 */, hj_render_stats* stats /* may be NULL */);
int hj_sample_probes(hj_context* ctx, const hj_probe_desc* desc, const float* probes, const float* points, size_t n, float* out /* n x 4 */);

/* Probe visibility (ABI 0.21): per probe an octahedral map of the mean and the mean squared distance to the nearest surface, baked
 * from the uploaded scene on the device, and a look-up of a probe volume that weights each of the eight probes about a point by a
 * back-face factor and by Chebyshev's bound on the share of the probe's rays that reach the point - the weights against light leaks
 * of Majercik et al. 2019, "Dynamic Diffuse Global Illumination with Ray-Traced Irradiance Fields" (their constants 0.2, 0.05 and
 * the cube).  Without them trilinear interpolation pulls light through every wall thinner than one spacing.  No counterpart in the
 * reference.  The numeric rules are the probe volumes' above: float32, one rounding per operation, no contraction; normalize, dot,
 * length and the RNG are the numeric contract's (kernels/hj_num.h: dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), length =
 * sqrt(dot(a, a)), normalize(a) = a * (1.0f / length(a))); min and max are minNum and maxNum; sg(x) = x >= 0.0f ? 1.0f : -1.0f.
 *   Of hj_probe_desc these calls use origin, spacing, count, seed and seed_stride; its flags must be 0 or HJ_PROBES_DEVICE_ARRAYS and
 *   must agree with HJ_PROBE_VIS_DEVICE_ARRAYS of hj_probe_vis_desc; min_distance is checked and not used.  T = res + 2.
 *
 * The atlas.  Probe p owns T * T texels of two floats, HJ_PROBE_VIS_WORDS(res) words behind word p * HJ_PROBE_VIS_WORDS(res): texel
 *   (bx, by) at index by * T + bx holds m1, the mean distance, and m2, the mean squared distance.  The interior is 1 ... res in both;
 *   interior texel (tx, ty), 0-based, is (tx + 1, ty + 1) and covers the square [tx, tx + 1] x [ty, ty + 1] * (2 / res) - 1 of the
 *   octahedral map.  The one-texel border holds the octahedral wrap: border (i + 1, 0) is interior (res - 1 - i, 0), border
 *   (i + 1, res + 1) is interior (res - 1 - i, res - 1), border (0, j + 1) is interior (0, res - 1 - j), border (res + 1, j + 1) is
 *   interior (res - 1, res - 1 - j), and each of the four corners is the diagonally opposite interior corner - so that the look-up
 *   is a plain bilinear fetch.
 *
 * hj_probe_visibility_rays: the rays of the bake for the probes first_probe ... first_probe + num_probes - 1, probe-major, res * res
 *   * rays_per_texel each in ascending r, as hj_trace_rays' records (8 words).  With s = rays_per_texel, ray r = (ty * res + tx) * s + k
 *   of probe p is sample k < s of interior texel (tx, ty):
 *       state = seedRng(seed + p * seed_stride + r)  (uint32 wrap-around);   u = rng_float(state);   v = rng_float(state);
 *       ex = ((float)tx + u) * (2.0f / (float)res) - 1.0f;   ey = ((float)ty + v) * (2.0f / (float)res) - 1.0f;
 *       az = (1.0f - |ex|) - |ey|;   d = az >= 0.0f ? (ex, ey, az) : ((1.0f - |ey|) * sg(ex), (1.0f - |ex|) * sg(ey), az);
 *       words 0-2 the probe's position (above), 3-5 normalize(d), 6 tMin = 0.0f, 7 tMax = max_distance.
 *   Needs a context but no scene.  num_probes == 0: HJ_OK, nothing touched.
 *
 * hj_bake_probe_visibility: from the uploaded scene to the atlas, in slabs of whole probes of at most HJ_PROBE_VIS_SLAB_RAYS rays (at
 *   least 32 probes).  Per slab: 1. its rays, as hj_probe_visibility_rays emits them; 2. hj_trace_rays over them with
 *   HJ_TRACE_DEVICE_ARRAYS, closest hit, no surface; 3. per atlas texel of the slab's probes, border included (a border texel takes
 *   the rays of the interior texel it copies), from a1 = a2 = +0, for k = 0 ... s - 1 ascending:
 *       dist = hit ? min(t, max_distance) : max_distance;   a1 = a1 + dist;   a2 = a2 + dist * dist;
 *   then m1 = a1 / (float)s and m2 = a2 / (float)s.  The atlas depends on the scene and the two descs alone, not on the slab size or a
 *   launch shape.  The context keeps one slab's rays and hits (48 bytes a ray, 24 MB at most) and, for a host-side atlas, one slab's
 *   part of it: nothing that grows with the volume.  The origin domain is hj_trace_rays'.
 *
 * hj_sample_probes_visible: hj_sample_probes with the two factors in each corner's weight.  probes, points, m (hj_sample_probes' n)
 *   and out as there.  Per point: x = words 0-2, nn = normalize(words 3-5), xb[a] = x[a] + nn[a] * normal_bias.  Axes, corners and
 *   q exactly as in hj_sample_probes (from x, not xb).  Per corner, P the probe's position from the corner's indices:
 *     back face:  wb = 1.0f if P == x in every component or with HJ_PROBE_VIS_NO_BACKFACE; otherwise
 *         t = normalize(P - x);   h = (dot(t, nn) + 1.0f) * 0.5f;   wb = h * h + 0.2f.
 *     Chebyshev:  e = xb - P;  wv = 1.0f if every component of e is zero or with HJ_PROBE_VIS_NO_CHEBYSHEV; otherwise rr = length(e),
 *         l1 = (|e.x| + |e.y|) + |e.z|;   px = e.x / l1;   py = e.y / l1;
 *         if e.z < 0.0f: (px, py) = ((1.0f - |py|) * sg(px), (1.0f - |px|) * sg(py)), both from the old values;
 *         cx = (px * 0.5f + 0.5f) * (float)res + 0.5f;   cy likewise;   per axis hj_sample_probes' clamp with origin 0, spacing 1 and
 *         count T gives i0, i1 and f (a NaN becomes 0);   with t00 = texel (ix0, iy0), t10 = (ix1, iy0), t01 = (ix0, iy1), t11 = (ix1, iy1),
 *         per moment  m = (t00 * (1.0f - fx) + t10 * fx) * (1.0f - fy) + (t01 * (1.0f - fx) + t11 * fx) * fy;
 *         if rr > m1:  var = |m1 * m1 - m2|;   dl = rr - m1;   c = var / (var + dl * dl);   wv = max((c * c) * c, 0.05f);   else wv = 1.0f.
 *     w = ((((wx * wy) * wz) * probes[q][27]) * wb) * wv;  from here on hj_sample_probes word for word: the w == 0 skip, acc, wsum,
 *     the basis at nn, out = (E[0], E[1], E[2], wsum).
 *   No index is formed from a value that has not been clamped: with device arrays nothing in points, probes or atlas can make the
 *   call fault; a NaN moment gives wv = 0.05f or 1.0f; a non-finite position gives NaN factors and a NaN result (a NaN, of no defined sign
 *   or payload), unless both factors are off.  With both NO_ flags atlas may be NULL and is not read, and the result is bit
 *   for bit hj_sample_probes'.  Needs a context but no scene.  m == 0: HJ_OK, nothing touched.
 *
 * HJ_PROBE_VIS_DEVICE_ARRAYS: as HJ_PROBES_DEVICE_ARRAYS - every array argument is a device pointer on the context's GPU, 16-byte aligned.
 *   Without it they are host arrays, staged through buffers the context keeps (hj_sample_probes_visible: volume and atlas whole, 48
 *   bytes per point); hj_sample_probes_visible then refuses non-finite positions and normals and all-zero normals as hj_sample_probes does.
 * HJ_ERR_INVALID, checked before anything else and without a device (with a null context the text is in hj_last_error(NULL)), in
 *   this order: a null desc, vis or array argument (hj_probe_visibility_rays: rays only with num_probes > 0; hj_sample_probes_visible:
 *   arrays only with m > 0, atlas only unless both NO_ flags are set); the refusals of hj_probe_desc in their order above; unknown bits
 *   in vis->flags; device-array flags that disagree; res other than 4, 8, 16; rays_per_texel outside [1, 64] and a max_distance that
 *   is not finite, not > 0 or above 1e18f (the rays and the bake; the look-up ignores both); a normal_bias that is negative or not
 *   finite (the look-up; the others ignore it, and the NO_ flags); first_probe + num_probes above the volume's probes; misaligned
 *   device arrays; m above 2^31 - 1; a bad position or normal in host arrays.  A null context: HJ_ERR_DEVICE in a process without a
 *   HIP device, HJ_ERR_INVALID otherwise.  HJ_ERR_STATE: hj_trace_rays' - an asynchronous frame in flight, frames submitted with
 *   HJ_RENDER_NO_DRAIN not yet drained, and for hj_bake_probe_visibility no scene.  A refused call writes nothing.
 * Not here: no adaptive bake, no multi-GPU split, no CLI.  (Blending an atlas over time: hj_update_probe_visibility, below; probes that sit in
 *   or against a wall and a look-up that knows where they moved to: "Probe placement", hj_sample_probes_visible_placed, below.) */
#define HJ_PROBE_VIS_DEVICE_ARRAYS 1u
#define HJ_PROBE_VIS_NO_BACKFACE 2u    /* look-up only */
#define HJ_PROBE_VIS_NO_CHEBYSHEV 4u   /* look-up only */
#define HJ_PROBE_VIS_SLAB_RAYS 524288u /* 2^19: the most rays of one slab of hj_bake_probe_visibility */
typedef struct hj_probe_vis_desc {
  uint32_t res;             /* octahedral map, res x res interior texels: 4, 8 or 16               */
  uint32_t rays_per_texel;  /* s, 1 ... 64 (rays and bake)                                         */
  float    max_distance;    /* finite, > 0, <= 1e18f: rays end here, a miss counts as this         */
  float    normal_bias;     /* finite, >= 0 (look-up)                                              */
  uint32_t flags;           /* HJ_PROBE_VIS_*                                                      */
} hj_probe_vis_desc;
#define HJ_PROBE_VIS_WORDS(res) (2u * ((res) + 2u) * ((res) + 2u))   /* 72, 200, 648: a probe's atlas is a multiple of 16 bytes */
int hj_probe_visibility_rays(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, uint32_t first_probe, uint32_t num_probes,
                             float* rays /* num_probes * res * res * rays_per_texel x 8 */);
int hj_bake_probe_visibility(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, float* atlas /* n x HJ_PROBE_VIS_WORDS(res) */);
int hj_sample_probes_visible(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes /* n x 28 */,
                             const float* atlas, const float* points /* m x 8 */, size_t m, float* out /* m x 4 */);

/* Probe updates (ABI 0.22): a window of a probe volume, or of its visibility atlas, re-baked from the uploaded scene under a frame's
 * own seeds and folded into the values the caller holds - the temporal blend ("hysteresis") of Majercik et al. 2019.  A scene that
 * changes (hj_scene_update_shapes, hj_refit_bvh_device) is followed with a few samples per probe per frame instead of a whole bake at
 * full spp, and a large volume is spread over several frames window by window.  No counterpart in the reference.  The numeric rules
 * are the probe volumes' above: float32, one rounding per operation, no contraction; min and max are minNum and maxNum; a comparison
 * with a NaN is false.
 *
 * The window and the fresh value.  The window is the probes first_probe ... first_probe + num_probes - 1 of desc's volume.  Let desc' be
 *   desc with seed' = seed + frame * frame_stride (uint32 wrap-around) in place of seed.  The fresh record F of probe p is record p of
 *   hj_bake_probes(desc', spp, opts); the fresh interior texels of probe p are those of hj_bake_probe_visibility(desc', vis).  A gather
 *   point carries its own seed, seed' + p * seed_stride, and ray r of probe p has the seed seed' + p * seed_stride + r: F does not
 *   depend on the window, nor on which other probes are updated with p.
 *
 * hj_update_probes: per probe of the window, with O the record now in `probes`, h = hysteresis and F[27] as hj_bake_probes defines it:
 *       new[27] = F[27];   keep = (O[27] > 0.0f) && (F[27] > 0.0f)  (a NaN compares false);   hh = 0.0f without keep; with it
 *       d = max(max(|F[0] - O[0]|, |F[1] - O[1]|), |F[2] - O[2]|);   m = max(max(|O[0]|, |O[1]|), |O[2]|)  - the constant band's three channels;
 *       hh = h;   if d > change_hard * m: hh = 0.0f;   else if d > change_soft * m: hh = max(h - 0.15f, 0.0f);
 *       for k = 0 ... 26:  new[k] = F[k] if hh == 0.0f, otherwise new[k] = O[k] * hh + F[k] * (1.0f - hh)  - two products and one sum,
 *       1.0f - hh formed once.
 *   The step 0.15 is the paper's, and its 0.25 and 0.8 are the Python wrapper's defaults for change_soft and change_hard: the paper's
 *   starting point, not values tuned here.  An infinite threshold never triggers (with m == 0 its product is a NaN, and the comparison false).
 *   With h == 0 the window becomes the fresh bake whatever the memory held before - NaN included, so a volume needs no
 *   initialisation.  A probe that was or becomes invalid never mixes coefficients.  Probes outside the window keep every bit.
 *   stats (may be NULL): the gather's.  spp and opts have hj_bake_probes' domain and refusals.
 *
 * hj_update_probe_visibility: per probe of the window, per interior texel, per moment, with O the old interior value and F the fresh one:
 *       new = F if h == 0.0f, otherwise new = O * h + F * (1.0f - h).
 *   Every border texel is then the new value of the interior texel it copies (the bake's mapping, under "The atlas" above).  A border
 *   texel's old value is never read: an atlas whose border disagreed with its interior is repaired by one update.  change_soft and
 *   change_hard are checked and not used.  A NaN in O (with h > 0) gives a NaN, of no defined sign or payload.  The call works in slabs of whole probes of at most HJ_PROBE_VIS_SLAB_RAYS rays, as the bake
 *   does; the result does not depend on the slab size or a launch shape.
 *
 * Arrays: with the device-array flags of the descs `probes` and `atlas` are device pointers, 16-byte aligned, updated in place on the
 *   context's stream.  Without them they are host arrays, of which the window's part alone is staged in, blended and copied back
 *   (hj_update_probe_visibility: slab by slab).  The context keeps 176 bytes per probe of the window (points and records) or one slab's
 *   rays and hits, and the staging of a host-side window or slab: memory that grows with the window, never with the volume.
 * HJ_ERR_INVALID, checked before anything else and without a device, in this order: the refusals of hj_bake_probes (of
 *   hj_bake_probe_visibility) up to and including the descs', in their order - a null desc, vis or array argument first -; a null
 *   update; non-zero update flags; first_probe + num_probes (in 64 bits) above the volume's probes; a hysteresis outside [0, 1), a
 *   NaN included; a change_soft, then a change_hard that is negative or a NaN (+inf is allowed: never); then spp == 0 or above 65536,
 *   misaligned device arrays and the refusals of opts (hj_update_probes).  A null context and HJ_ERR_STATE as for the bakes: both calls
 *   need a scene.  num_probes == 0: HJ_OK after all of these, nothing touched.  A refused call writes nothing.
 * Not here: no adaptive update (a per-probe spp), no multi-GPU split, no CLI flag.  (Probe relocation and classification: hj_place_probes
 *   and the _placed updates, "Probe placement" below.) */
#define HJ_PROBE_UPDATE_WORDS 8u
typedef struct hj_probe_update {
  uint32_t first_probe, num_probes;   /* the window: probes first_probe ... first_probe + num_probes - 1, inside the volume     */
  uint32_t frame, frame_stride;       /* this update's seeds: desc->seed + frame * frame_stride (uint32 wrap-around)            */
  float    hysteresis;                /* h, 0 <= h < 1: the share of the old value that is kept                                 */
  float    change_soft, change_hard;  /* >= 0, +inf allowed (= never), NaN refused; hj_update_probes only                       */
  uint32_t flags;                     /* must be 0                                                                              */
} hj_probe_update;                    /* 32 bytes */
int hj_update_probes(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_update* update, uint32_t spp, const hj_render_opts* opts /* NULL = defaults */,
                     float* probes /* n x 28, read and written */, hj_render_stats* stats /* may be NULL */);
int hj_update_probe_visibility(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const hj_probe_update* update,
                               float* atlas /* n x HJ_PROBE_VIS_WORDS(res), read and written */);

/* Probe placement (ABI 0.23): per probe an offset from its grid point and an active / inactive state, found from the uploaded scene -
 * the probe relocation and classification of Majercik et al. 2021, "Scaling Probe-Based Real-Time Dynamic Global Illumination" - and
 * the updates and the look-up that read them.  A probe that the grid puts inside a wall, or nearer to one than min_distance, is
 * switched off whole by hj_bake_probes' validity word, and the look-up loses a corner exactly where surfaces are: relocation moves it
 * out of the wall instead.  A probe with no geometry in any of its eight cells is gathered and traced by every update for nobody:
 * classification marks it inactive, and the placed updates leave it out.  No counterpart in the reference.  The numeric rules are the
 * probe volumes' above: float32, one rounding per operation, no contraction; dot and length are the numeric contract's; min is
 * minNum; a comparison with a NaN is false.
 *
 * The placement array.  HJ_PROBE_PLACE_WORDS = 4 words per probe, n x 4, in probe order: words 0-2 the offset o in world units
 *   (float32), word 3 the state as uint32 bits - 0: active, anything else: inactive (the calls write 1).  The placed position of probe
 *   (x, y, z) is P[a] = (origin[a] + (float)i_a * spacing[a]) + o[a]: the existing product and sum, then one more sum.  An array of
 *   zero bits places every probe on its grid point, active.  Whether it is a host or a device array follows the descs' device-array
 *   flag; a device array is 16-byte aligned.  A host array with a non-finite offset (in the window; the look-up: anywhere) is
 *   refused; with device arrays a non-finite offset is the caller's contract and yields NaN, never a fault: no index is formed from
 *   a value that has not been clamped or compared.
 *
 * hj_place_probes: one relocation-and-classification step over the window first_probe ... first_probe + num_probes - 1, in place.
 *   The call works in slabs of whole probes of at most HJ_PROBE_VIS_SLAB_RAYS rays, exactly as hj_bake_probe_visibility does; the
 *   context keeps one slab's rays, hits and surface records (112 bytes a ray, 56 MB at most) and nothing that grows with the volume.
 *   Per probe p of the window, with O its old offset: the R = res * res * rays_per_texel rays are hj_probe_visibility_rays' rays of
 *   desc' (seed' = seed + frame * frame_stride, uint32 wrap-around) - directions and seeds identical -, the origin the placed position
 *   under O.  Every probe of the window is traced, inactive ones included, so that they can wake up; by hj_trace_rays with device
 *   arrays, closest hit, with the surface record.  Per ray r, ascending, with d = ray words 3-5 and n = surface words 3-5:
 *       hit = objectID >= 0;   dist = hit ? min(t, max_distance) : max_distance;   back = hit && dot(d, n) > 0.0f.
 *   nb = the number of back rays;  (cb, rb) = the least dist over back rays and its ray;  (cf, rf) = the least dist over non-back rays,
 *   misses included;  (ff, rq) = the greatest dist over non-back rays;  ties go to the lowest r.  inside = (float)nb > backface_share * (float)R.
 *   Relocation (skipped with HJ_PROBE_PLACE_NO_RELOCATE: the offset keeps its bits).  cand = O; the first case that matches:
 *       inside:                                                cand = O + d[rb] * (cb + min_front_distance * 0.5f);
 *       else a non-back ray exists and cf < min_front_distance:  if dot(d[rf], d[rq]) <= 0.5f:  cand = O + d[rq] * min(ff, min_front_distance);
 *       else a non-back ray exists and cf > min_front_distance:  L = length(O);  if L > 0.0f:  back = min(cf - min_front_distance, L);
 *                                                                cand[a] = O[a] - (O[a] / L) * back.
 *     Each vector step is one product and one sum per component.  The new offset is cand when |cand[a]| <= max_offset * spacing[a]
 *     on every axis (a NaN compares false); otherwise the offset stays O, bit for bit.
 *   Classification (skipped with HJ_PROBE_PLACE_NO_CLASSIFY: the state keeps its bits), from the same rays and the old O: inactive if
 *     inside; otherwise active exactly when some ray has hit && !back and |O[a] + d[a] * t| <= spacing[a] on all three axes - a
 *     front face lies inside the eight cells the probe serves; otherwise inactive.
 *   The reduction runs one wave per probe; its count is an integer and its extremes are (dist, r) keys, so the result depends on
 *   (scene, desc, vis, place, old placement) alone, not on the slab size or a launch shape.  backface_share 0.25 and max_offset 0.45
 *   (the Python wrapper's defaults) are the paper's and RTXGI's starting points, not values tuned here.  Of vis the call uses res,
 *   rays_per_texel and max_distance.
 *
 * The placed consumers take `const float* placement` in front of the array they write.
 * hj_update_probes_placed: hj_update_probes with the gather points at the placed positions.  The window's inactive probes are left
 *   out of the gather: they get no point, are not traced, and their records keep every bit.  The active probes are compacted in order
 *   on the device; their number comes back to the host once, to size the gather.  All inactive: HJ_OK, nothing written (stats
 *   included).  stats counts only what was traced.
 * hj_update_probe_visibility_placed: hj_update_probe_visibility by the same rule with the same list: the rays start at the placed
 *   positions, slabs are cut from the list, and an inactive probe's texels, border included, keep every bit.  A host-side atlas
 *   travels the window at a time.
 * hj_sample_probes_visible_placed: hj_sample_probes_visible with two changes.  P is the placed position in both the back-face and the
 *   Chebyshev factor; the cell indices and the trilinear weights stay the unplaced grid's, as in the paper.  A corner whose probe is
 *   inactive has w = 0 and is skipped whatever its record holds: an inactive probe's record may never have been written.
 * With a placement of all +0 offsets and state 0 each of the three is bit for bit its unplaced counterpart, with one exception:
 *   x + 0.0f turns a probe coordinate of -0 into +0.
 * There are no placed bakes: with hysteresis 0 over the whole volume an update is the bake (ABI 0.22).
 *
 * HJ_ERR_INVALID, checked before anything else and without a device, in this order.  hj_place_probes: a null desc, vis or placement;
 *   the refusals of hj_bake_probe_visibility's descs in their order; a null place; unknown place flags; first_probe + num_probes (in
 *   64 bits) above the volume's probes; a min_front_distance that is not finite or not > 0; a backface_share outside [0, 1]; a
 *   max_offset outside [0, 0.5) (a NaN is outside); a misaligned device array; a bad host offset.  The placed consumers: their unplaced
 *   counterpart's refusals in its order, with a null placement among the null arguments (the look-up: whatever m is), placement
 *   among the misaligned device arrays, and a bad host offset last.  A null context and HJ_ERR_STATE as for the unplaced calls:
 *   hj_place_probes and the placed updates need a scene.  num_probes == 0: HJ_OK after all of these, nothing touched.  A refused
 *   call writes nothing.
 * Not here: no CLI flag, no multi-GPU split, no fusion of the placement rays with the visibility update's trace (hj_place_probes
 *   and hj_update_probe_visibility_placed each trace their own rays). */
#define HJ_PROBE_PLACE_WORDS 4u
#define HJ_PROBE_PLACE_NO_RELOCATE 1u
#define HJ_PROBE_PLACE_NO_CLASSIFY 2u
typedef struct hj_probe_place {
  uint32_t first_probe, num_probes;   /* the window: probes first_probe ... first_probe + num_probes - 1, inside the volume     */
  uint32_t frame, frame_stride;       /* this step's seeds: desc->seed + frame * frame_stride (uint32 wrap-around)              */
  float    min_front_distance;        /* finite, > 0: how near a front face may be                                              */
  float    backface_share;            /* in [0, 1]: more back-face rays than this share of R, and the probe is inside geometry  */
  float    max_offset;                /* in [0, 0.5): the offset stays within this share of the spacing on every axis           */
  uint32_t flags;                     /* HJ_PROBE_PLACE_*                                                                       */
} hj_probe_place;                     /* 32 bytes */
int hj_place_probes(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const hj_probe_place* place,
                    float* placement /* n x 4, read and written */);
int hj_update_probes_placed(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_update* update, uint32_t spp,
                            const hj_render_opts* opts /* NULL = defaults */, const float* placement /* n x 4 */,
                            float* probes /* n x 28, read and written */, hj_render_stats* stats /* may be NULL */);
int hj_update_probe_visibility_placed(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const hj_probe_update* update,
                                      const float* placement /* n x 4 */, float* atlas /* n x HJ_PROBE_VIS_WORDS(res), read and written */);
int hj_sample_probes_visible_placed(hj_context* ctx, const hj_probe_desc* desc, const hj_probe_vis_desc* vis, const float* probes /* n x 28 */,
                                    const float* atlas, const float* points /* m x 8 */, size_t m, const float* placement /* n x 4 */,
                                    float* out /* m x 4 */);

/* ------------------------------------------------------------------- probes */

/* Function-level probes used by the parity tests (no counterpart in the
 * reference; they expose intermediate values of the same kernels).
 * hj_debug_trace: intersectScene (shader/scene.glsl:92-175) for caller-given
 *   rays.  rays = n x 8 floats (origin.xyz, direction.xyz, tMin, tMax);
 *   hits = n x 4 floats (objectID as int32 bits or -1, t, u, v of the raw hit
 *   before populate*).  any_hit != 0 stops at the first accepted hit (the
 *   shadow-ray form): then only `objectID >= 0` is meaningful.
 * hj_debug_samples: the intermediate image of ONE block (layers 0 and 1 of
 *   shader/render.glsl:172-173): dimension.y x dimension.x x 8 floats
 *   (radiance rgb, 1, first-hit normal xyz, first-hit t), no reconstruction,
 *   framebuffer untouched. */
int hj_debug_trace(hj_context* ctx, const float* rays, size_t n, uint32_t use_bvh, uint32_t any_hit, float* hits);
int hj_debug_samples(hj_context* ctx, const hj_image_block* block, const hj_render_opts* opts, float* samples);
/* hj_debug_texture_lookup: the colour the shade stage takes from texture `texture` of the uploaded scene at n (u, v) pairs
 *   (uv = n x 2 floats, rgb = n x 3 floats), by the same device function.  No scene: HJ_ERR_STATE; texture out of range:
 *   HJ_ERR_INVALID. */
int hj_debug_texture_lookup(hj_context* ctx, uint32_t texture, const float* uv, size_t n, float* rgb);
/* hj_debug_env_lookup: the radiance the uploaded environment sends along n directions (dirs = n x 3 floats, any length; rgb =
 *   n x 3 floats), by the device function misses and next-event samples use.  No environment: HJ_ERR_STATE.
 * hj_debug_env_sample: one environment sample per RNG state (n uint32), drawn as next-event estimation draws it after picking the
 *   environment (coin = rng_float, then two rng_uint): out = n x 8 floats = direction xyz (unit), pdf (solid angle, without the
 *   selection probability), texel index (float), Le / pdf rgb.  No environment: HJ_ERR_STATE.
 * hj_debug_env_distribution: the sampling distribution hj_scene_upload_env builds for `env` over `textures` (pure host code: no
 *   context, no GPU), W x H entries in texel order (row 0 = top): cell probability P (may be NULL), pdf = P / solid angle (may be
 *   NULL), alias-table threshold and alias cell (may be NULL).  weight_sum (may be NULL) = the sum of the cell weights; 0: black. */
int hj_debug_env_lookup(hj_context* ctx, const float* dirs, size_t n, float* rgb);
int hj_debug_env_sample(hj_context* ctx, const uint32_t* rng_states, size_t n, float* out);
int hj_debug_env_distribution(const hj_texture_set* textures, const hj_environment* env, float* prob, float* pdf, float* alias_prob,
                              uint32_t* alias, double* weight_sum);
/* hj_debug_light_grid: the light-shaft visibility grid hj_scene_upload would build for `scene` (pure host code: no context,
 *   no GPU).  Returns the cells per axis (0: nothing can be proven for this scene).  bits (may be NULL) = res^3 bytes, x fastest:
 *   bit e of a cell set = every next-event shadow ray from a hit point in that cell to emitter e is unoccluded; the cell of a
 *   point p along axis k is (int)((p[k] - lo[k]) * inv[k]) in float arithmetic; stats = cells that hold a surface, cells whose
 *   surfaces lie in one plane, (cell, emitter) pairs proven free.  tests/test_light_grid.py attacks the claim with the oracle. */
int hj_debug_light_grid(const hj_scene_desc* scene, uint32_t res, uint8_t* bits, float lo[3], float inv[3], uint64_t stats[3]);
/* hj_debug_light_grid_planes: the same grid with its two kinds of proof apart.  planar (res^3 bytes): bits that hold for EVERY hit
 *   point of the cell (all shapes of the cell in one plane); mesh (res^3 bytes): bits of cells on meshes and in corners, which hold
 *   for a hit point that lies on its shape - a grazing hit leaves the reference's hit point off it, so the shade stage checks
 *   (DESIGN.md section 4): with recs, 8 floats per quad and triangle (shape index - num_spheres) = unit normal n, margin delta;
 *   vertex a, 0 (triangle) / 1 (quad), and limits = {sin_in, slide}: |d.n| >= sin_in |d|, (|n.(p - a)| + 3e-7 |p - a|_1) |d| <= slide |d.n|,
 *   min(u, v, 1 - u - v) >= delta (a quad: u, v, 1 - u, 1 - v) for the ray (o, d) that hit and its (t, u, v).
 *   hj_debug_light_grid's bits = planar | mesh.  Any output may be NULL. */
int hj_debug_light_grid_planes(const hj_scene_desc* scene, uint32_t res, uint8_t* planar, uint8_t* mesh, float* recs, float limits[2],
                               float lo[3], float inv[3], uint64_t stats[3]);
/* hj_debug_num: the device text of the numeric contract (kernels/hj_num.h) on caller-given inputs - the
 *   functions the path kernels call, one thread per record, no scene needed.  in = n x HJ_NUM_IN_WORDS words, out = n x
 *   HJ_NUM_OUT_WORDS words; a word is the bits of a float, or a uint32 for the RNG; words an op does not read are ignored, words
 *   it does not write come back 0.  With a = word 0, b = word 1, p = words 0-2, q = words 3-5, s = word 0 as an RNG state:
 *     EXP exp(a); SINCOS2PI sin, cos of 2 pi a; ATAN2 atan2(y = a, x = b); ASIN asin(a); MIN / MAX min / max(a, b); DIV a / b;
 *     SQRT sqrt(a); DOT3 p . q; CROSS3 p x q (3 words); NORMALIZE3 p / |p| (3 words); REFLECT3 reflect(I = p, N = q) (3 words);
 *     RNG_SEED the hash of s; RNG_UINT / RNG_FLOAT the next draw, then the state after it; RAND_COS_HEMISPHERE /
 *     RAND_UNIFORM_SPHERE / RAND_BARYCENTRIC the sample (3 words), then the state after it.
 *   Refused with HJ_ERR_INVALID: a null argument, an op that is none of these, n == 0, n above HJ_NUM_MAX_RECORDS. */
enum hj_num_op {
  HJ_NUM_EXP = 0, HJ_NUM_SINCOS2PI, HJ_NUM_ATAN2, HJ_NUM_ASIN, HJ_NUM_MIN, HJ_NUM_MAX, HJ_NUM_DIV, HJ_NUM_SQRT, HJ_NUM_DOT3,
  HJ_NUM_CROSS3, HJ_NUM_NORMALIZE3, HJ_NUM_REFLECT3, HJ_NUM_RNG_SEED, HJ_NUM_RNG_UINT, HJ_NUM_RNG_FLOAT,
  HJ_NUM_RAND_COS_HEMISPHERE, HJ_NUM_RAND_UNIFORM_SPHERE, HJ_NUM_RAND_BARYCENTRIC, HJ_NUM_OPS
};
#define HJ_NUM_IN_WORDS 6
#define HJ_NUM_OUT_WORDS 4
#define HJ_NUM_MAX_RECORDS 1048576u   /* 2^20 */
int hj_debug_num(hj_context* ctx, uint32_t op, const uint32_t* in, size_t n, uint32_t* out);
/* hj_debug_shade_step: ONE pass of the shade stage over n caller-given path states and raw hits on the uploaded scene - the
 *   stage's own kernel of the split path, launched once over a batch this call fabricates; nothing of its arithmetic is restated.
 *   in = n x HJ_STEP_IN_WORDS words (the bits of a float unless said otherwise):
 *      0-2 ray origin, 3-5 ray direction, 6 raw hit t, 7 object id (int32; negative: the ray left the scene), 8-9 raw hit u, v,
 *      10-12 throughput, 13-15 extinction, 16 RNG state (uint32), 17 flags as the stage stores them (bit 0 wasDiscrete, bits 1..
 *      the bounce index).
 *   Record i is sample i and goes to the next position of workgroup i % num_wg's queue segment, in the path arrays of round parity
 *   `parity` (0 or 1); hits are binned by material tag in queue order as the hit compaction bins them, misses go to the miss bin of
 *   a scene with an environment and are dropped otherwise.  opts gives max_bounces, rr_start and HJ_RENDER_NO_LIGHT_GRID (use_bvh =
 *   0 switches the light-shaft grid off as well), as in a render call.
 *   out = n x HJ_STEP_OUT_WORDS words, matched to the records by the sample index the stage's appends carry; all zero but for:
 *      0 alive (1: the path continues; words 1-14 are its next record), 1-3 next origin, 4-6 next direction, 7-9 throughput,
 *      10 flags, 11 RNG state, 12-14 extinction (0 unless a dielectric of the scene has one: the stage then keeps none),
 *      15 shadow record present (1), 16-18 its origin, 19-21 direction, 22 tMax, 23-25 the pending next-event contribution,
 *      26-28 the sample's radiance (emission seen directly, the environment behind a miss, or a next-event contribution the
 *      light-shaft grid proved unoccluded), 29-32 the sample's first-hit normal and t (written at bounce 0).
 *   counters = num_wg x 3 words: continuing paths appended, shadow records appended, next-event samples the grid answered.
 *   No scene: HJ_ERR_STATE.  HJ_ERR_INVALID: a null argument, n == 0, n above HJ_STEP_MAX_RECORDS, num_wg == 0 or above n (a
 *   workgroup without a record), parity above 1, an object id that is no shape of the scene.
 *   Reach: explicit path records through the stage's instantiation with ordinary loads and stores.  Implicit camera paths (no
 *   record: state derived from the sample index), the streaming (non-temporal) instantiation of large trees and the fused kernel's
 *   call wrapper are not reached from here; frames pin those. */
#define HJ_STEP_IN_WORDS 18
#define HJ_STEP_OUT_WORDS 33
#define HJ_STEP_MAX_RECORDS 65536u
int hj_debug_shade_step(hj_context* ctx, const hj_render_opts* opts, const uint32_t* in, size_t n, uint32_t num_wg, uint32_t parity,
                        uint32_t* out, uint32_t* counters);
/* hj_debug_reconstruct: ONE reconstruction pass (shader/reconstruction.glsl:22-66) over caller-given samples, accumulated into the
 *   context's framebuffer (created or bound) exactly as a batch's reconstruction is: the nb blocks are staged in a batch slot, the
 *   per-tile block lists and the launch are the render calls' own; nothing of the kernel or of the lists is restated.
 *   samples = the blocks' sample images in hj_debug_samples' layout, one after the other in list order: dimension.y x dimension.x
 *   x 8 floats per block (rgb, weight, normal xyz, depth), of any value.  Of a block only origin, dimension, original_dimension and
 *   sample_offset are read; of opts (NULL: the defaults) only recon_stddev, and the checks every render call makes.  Every sample
 *   slot of the batch outside a block's dimension holds 1e30 in every word before the launch - finite, because the kernel skips a
 *   tap whose product is a NaN and would so hide a stray read of one.
 *   No scene is needed.  No framebuffer: HJ_ERR_STATE.  HJ_ERR_INVALID: a null argument, nb == 0, nb above HJ_RECON_MAX_BLOCKS, a
 *   dimension outside (0, HJ_BLOCK_SIZE], an original_dimension that is not the framebuffer's, recon_stddev not > 0, max_bounces
 *   == 0; HJ_ERR_UNSUPPORTED: recon_radius != 2.  A block none of whose extended rectangle lies in the image is no error.
 *   Reach: one batch in slot 0.  The order between batches of different slots (the reconstruction event chain) is not reached
 *   from here; frames pin it. */
#define HJ_RECON_MAX_BLOCKS 64u
int hj_debug_reconstruct(hj_context* ctx, const hj_image_block* blocks, size_t nb, const hj_render_opts* opts, const float* samples);
/* The two stages of the device ray vote (hj_tune_bvh_device, kernels/hj_vote.h) apart, on caller-given inputs (ABI 0.20): the same
 *   device functions and kernels, the same host routines as the vote's; nothing of them is restated.  All arrays on the host.
 * hj_debug_vote_cast: what n caller-given rays add to the gains of scene->bvh (scene->num_bvh_nodes = N records).  rays = n x 8
 *   floats in hj_trace_rays' layout, the direction used as it is (the sampler's are unit vectors; the sphere test assumes one, the slab
 *   test does not).  any_hit != 0: every ray votes as a shadow ray (all of ci, times w_shadow); 0: as a closest-hit ray
 *   ((ci - ct) * 4).  w_shadow: explicit, 0 ... 16 (HJ_BVH_VOTE_SHADOW's range).  given_hits (may be NULL) = n x 2 words: the array
 *   position of the leaf the ray hit (0xFFFFFFFF: the ray missed) and t (float bits): hj::vote::closest is then skipped and
 *   hj::vote::cast runs on that hit - the counts become a function of the boxes, the ray and t alone.  NULL: cast runs on what
 *   closest finds.  gain_l, gain_r = `capacity` (>= N) 64-bit words each, of which N are written; found = n x 4 words: leaf position
 *   (0xFFFFFFFF: none), shape (int32, -1: none), t (float bits), 0 - of closest, or the given hit echoed.
 *   A ray votes at every ancestor of its leaf down to level HJ_VOTE_MAX_LEVELS, the depth the exchange accepts.
 * hj_debug_vote_exchange: the exchange on caller-given gains.  nodes = N records of a pre-order skip-link tree (boxes and shape
 *   words are carried, not read; the root's exit may be N or HJ_BVH_ROOT_EXIT or anything >= N); gain_l, gain_r = N words.  The
 *   children of node i change places where gain_r[i] > gain_l[i] (ties stay).  out_nodes (capacity >= N) = the re-ordered records,
 *   info = levels that held an inner node, nodes exchanged, the kernels' error bits, 0.  Statuses as the vote's: links that are not a
 *   tree's HJ_ERR_INVALID (checked on the host, before the device: the exchange sizes its writes by them), more than
 *   HJ_VOTE_MAX_LEVELS levels HJ_ERR_UNSUPPORTED.
 * hj_debug_vote_gains: gain_l, gain_r (capacity >= N words each) exactly as the sampler leaves them after `paths` camera paths of
 *   `scene` through scene->bvh - what hj_tune_bvh_device(scene, ..., paths) hands to its exchange; w_shadow from HJ_BVH_VOTE_SHADOW /
 *   the tree's size, as there.  paths == 0 or N < 3: all zero.
 * Refused with HJ_ERR_INVALID before the device is touched: a null argument, a scene without a tree or one hj_scene_upload would
 *   refuse, capacity < N, n == 0 or above HJ_VOTE_MAX_RAYS, w_shadow > 16, a given position that is neither 0xFFFFFFFF nor a leaf
 *   of the tree, N == 0.  Then the gates of hj_tune_bvh_device: a frame in flight, frames in the pipeline (HJ_ERR_STATE). */
#define HJ_VOTE_MAX_LEVELS 8192u
#define HJ_VOTE_MAX_RAYS 1048576u   /* 2^20 */
int hj_debug_vote_cast(hj_context* ctx, const hj_scene_desc* scene, const float* rays, size_t n, uint32_t any_hit, uint32_t w_shadow,
                       const uint32_t* given_hits /* may be NULL */, uint64_t* gain_l, uint64_t* gain_r, size_t capacity, uint32_t* found);
int hj_debug_vote_exchange(hj_context* ctx, const hj_bvh_node* nodes, size_t N, const uint64_t* gain_l, const uint64_t* gain_r,
                           hj_bvh_node* out_nodes, size_t capacity, uint32_t info[4]);
int hj_debug_vote_gains(hj_context* ctx, const hj_scene_desc* scene, size_t paths, uint64_t* gain_l, uint64_t* gain_r, size_t capacity);

/* ---------------------------------------------------------- distance queries */

/* Distance queries (ABI 0.24): the nearest surface point of the uploaded scene to caller-given points - the query that starts from no
 * ray (no counterpart in the reference).  Every arithmetic operation below is float32, one rounding per operation, no contraction
 * except dot3 / cross3 of the numeric contract (dot3(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), len3 = sqrt of
 * dot3); `/` and sqrt are IEEE.  kernels/hj_closest.h and tests/closest_ref.py are the two texts of this one specification.
 *
 * Per shape, a pure function of the point p and the shape's uploaded record -> (q, d2, u, v, side):
 *   sphere (c, r):  w = p - c, l = len3(w);  q = c + w * (r / l), and c + (r, 0, 0) when l == 0;  d2 = (l - r) * (l - r);  u = v = 0;
 *     side = +1 when l >= r, else -1.
 *   triangle (a, b, c):  on ab = b - a, ac = c - a, ap = p - a, bp = ap - ab, cp = ap - ac, the region walk of Ericson, Real-Time
 *     Collision Detection 5.1.5 - the three vertices, then the edges ab, ac, bc, then the face - with every dot product a dot3;
 *     kernels/hj_closest.h states the seven tests and their order.  (u, v) are the coefficients of ab and ac, the barycentric pair
 *     of hj_trace_rays' raw hit;  q = (a + ab * u) + ac * v;  d2 = dot3(p - q, p - q);  side = +1 when
 *     dot3(p - q, cross3(ab, ac)) >= 0, else -1.  A degenerate triangle comes out as that text computes it, NaN included.
 *   quad (origin, edge1, edge2), a parallelogram:  w = p - origin;  s = dot3(w, edge1) / dot3(edge1, edge1),
 *     t = dot3(w, edge2) / dot3(edge2, edge2), each clamped to [0, 1] (a NaN stays);  (u, v) = (s, t);
 *     q = (origin + edge1 * s) + edge2 * t;  d2 and side as for the triangle, with cross3(edge1, edge2).  The two separate
 *     projections give the nearest point for rectangles only; for a sheared quad q is a point of the quad, not the nearest.
 * The answer for a point (p, r), r the search radius (+inf: unbounded), r2 = r * r: a shape is a candidate when its d2 is not NaN and
 *   d2 <= r2; the answer is the candidate with the smallest key (d2 as uint32 bits, global shape index), so ties resolve to the lower
 *   index.  A NaN or negative r, a non-finite coordinate of p, or no candidate gives a miss.  The answer depends on the point and
 *   the shapes alone: not on the tree, the visiting order, the launch shape or the lane that carried the point.
 * The tree only decides what is skipped, by a bound on the COMPUTED d2 with an absolute slack of 2^-18 times the largest coordinate
 *   magnitude of the root box (DESIGN.md has the derivation).  Equality with the brute-force answer over all shapes is claimed for
 *   trees whose boxes bound their subtrees: every tree the host compiler, hj_build_bvh_device, hj_refit_bvh_device,
 *   hj_optimize_bvh_device and hj_scene_update_shapes produce.  For caller-supplied boxes that do not bound their subtrees the
 *   answer is whatever the skipping gives.  Magnitudes: a sphere or quad gets an answer while the squares of
 *   coordinate differences stay finite (below 2^60); a triangle multiplies two dot products and gets one only while coordinate
 *   differences stay below about 2^31 - beyond that its areas are inf - inf, its d2 is NaN and it is no candidate.
 * side is the facing of the nearest shape - which side of its plane, or of the sphere's surface, p is on.  It is not a robust
 *   inside / outside test: at an edge or a vertex shared by faces that face differently, the shape with the lower index decides.
 *
 * hj_closest_points:  points: n x 4 floats (p.xyz, r).  out: n x HJ_CLOSEST_WORDS floats - [0] the shape index as int32 bits or -1,
 *     [1] sqrt(d2), [2..4] q, [5] u, [6] v, [7] side; a miss is -1 followed by seven zeros.
 *   stats (may be NULL; always a host pointer): [0] nodes visited, [1] shapes tested, over all points of the call; a function of the
 *     points and the uploaded tree alone.
 *   HJ_CLOSEST_DEVICE_ARRAYS: points / out are device pointers on the context's GPU, 16-byte aligned, read and written in place (the
 *     caller orders its own streams before the call).  Without it they are host arrays, staged through buffers the context keeps.
 *   Runs on the context's stream and returns when the results are complete.  n == 0: HJ_OK, nothing touched.
 *   HJ_ERR_INVALID, checked before anything else and before the device is touched, in this order: null points or out (n > 0);
 *     unknown flag bits; n above 2^31 - 1; with device arrays, points or out misaligned, or stats given as anything but a host pointer.  With a
 *     null context the text is in hj_last_error(NULL).  A refused call writes nothing.
 *   A null context: HJ_ERR_DEVICE in a process without a HIP device, HJ_ERR_INVALID otherwise.  HJ_ERR_STATE: hj_trace_rays' - no
 *     scene, an asynchronous frame in flight, frames submitted with HJ_RENDER_NO_DRAIN not yet drained.
 *
 * hj_distance_field:  the grid of desc (hj_probe_points' positions; of desc the seeds and min_distance are not used) through the
 *     query with r = max_distance, without the points or the records leaving the device.  field: count[0] * count[1] * count[2]
 *     floats in ascending p: side * sqrt(d2), or sqrt(d2) alone with HJ_DISTANCE_UNSIGNED; a miss gives max_distance (signed: +).
 *   desc->flags HJ_PROBES_DEVICE_ARRAYS: field is a device pointer, 16-byte aligned.
 *   HJ_ERR_INVALID, in this order: a null desc or field; the refusals of desc (hj_probe_points'); unknown distance flag bits; a
 *     max_distance that is NaN or negative; a misaligned device array.  Then hj_closest_points' gate.
 * Not here: no surface record or material at q (hj_trace_rays' surface is for ray hits); no multi-GPU split; probe validity and
 *   relocation still come from rays. */
#define HJ_CLOSEST_DEVICE_ARRAYS 1u
#define HJ_CLOSEST_WORDS 8u
#define HJ_DISTANCE_UNSIGNED 1u
int hj_closest_points(hj_context* ctx, const float* points /* n x 4: p.xyz, radius */, size_t n, uint32_t flags,
                      float* out /* n x 8 */, uint64_t* stats /* may be NULL: [0] nodes visited, [1] shapes tested */);
int hj_distance_field(hj_context* ctx, const hj_probe_desc* desc, float max_distance, uint32_t flags, float* field);

/* ---------------------------------------------------------- all-hit queries */

/* All-hit queries (ABI 0.25): every hit along a ray - the third form beside hj_trace_rays' closest hit and HJ_TRACE_ANY_HIT: the K
 * nearest hits in order, how many there are, and the signed sum of their crossings; and from that sum whether a point lies inside
 * closed geometry (no counterpart in the reference; multi-hit traversal: Gribble et al. 2014).  Every arithmetic
 * operation below is float32, one rounding per operation, no contraction except dot3 / cross3 of the numeric contract;
 * `/` and sqrt are IEEE.  kernels/hj_multihit.h and tests/allhits_ref.py are the two texts of this one specification.
 *
 * The contract is a function of the ray (o, d, tMin, tMax) and the uploaded tree alone:
 *   Candidates: the pre-order skip-link walk of the uploaded tree as it was uploaded (every node, every leaf), with the caller's
 *     [tMin, tMax] never shrunk.  An inner node is entered iff its box passes the box test below; leaf boxes are not tested; every
 *     shape whose leaf is reached is tested with the caller's range.  A quad or a triangle gives one candidate (t, u, v) when the
 *     shape test of hj_trace_rays accepts it.  A sphere gives up to two: with l = o - c, b = 2 * dot3(d, l), cc = dot3(l, l) - r * r,
 *     D = b * b - 4 * cc (no candidate when D < 0), s = sqrt(D), t0 = -0.5 * (b + s), t1 = -0.5 * (b - s) - the closest-hit test's
 *     arithmetic, which takes d as a unit vector -, each root with tMin <= t <= tMax is a candidate, with u = 0 for t0, 1 for t1,
 *     and v = 0.
 *   Box test, without fused multiply-add: inv = 1 / d per axis;  t1 = (lo - o) * inv, t2 = (hi - o) * inv;  tn = t1 < t2 ? t1 : t2,
 *     tp = t1 < t2 ? t2 : t1;  T0 = the three tn folded x, y, z by a < b ? b : a;  T1 = the three tp folded by a < b ? a : b;
 *     enter iff !(T0 > T1) && !(T0 > tMax) && !(T1 < tMin).  A NaN T0, T1, tMin or tMax never culls.  This is not the closest-hit walk's test (fused,
 *     with an epsilon, against a shrinking tMax): a shape whose box a ray grazes may be a candidate here and no hit there, or the
 *     reverse.  Like every slab test it can miss a box that a ray with a zero direction component touches on its face.
 *   Key: (t as a float, shape index, root), compared in that order: equal t goes to the lower shape index, a sphere's t0 before t1.
 *   Crossing: +1 for a candidate that leaves through its surface (dot3(d, n_g) > 0), -1 for one that enters (< 0), 0 otherwise;
 *     n_g = cross3(edge1, edge2) for a quad, cross3(b - a, c - a) for a triangle; a sphere's t0 enters, its t1 leaves.  A point
 *     inside a closed surface whose n_g point outward gets +1 along any direction.
 *   Record i depends on ray i and the scene alone: not on the lane, the workgroup, the launch or the chunk that carried it.
 *
 * hj_trace_rays_all:  rays: n x 8 floats in hj_trace_rays' layout (origin, direction of any length, tMin, tMax).  max_hits K: 0 ...
 *     HJ_ALLHITS_MAX_HITS; with K = 0 hits may be NULL (counting only).
 *   counts: n x 2 words - [0] (uint32) the number of candidates, [1] (int32) the signed crossing sum.
 *   hits: n x K x 4 floats - record j of ray i is (objectID bits, t, u, v) as hj_trace_rays writes it; the first min(count, K)
 *     records are the candidates with the smallest key in ascending key order, the rest are (-1, 0, 0, 0).
 *   HJ_ALLHITS_DEVICE_ARRAYS: rays / counts / hits are device pointers on the context's GPU, 16-byte aligned, read and written in
 *     place (the caller orders its own streams before the call).  Without it they are host arrays, staged in chunks of
 *     HJ_TRACE_CHUNK rays through buffers the context keeps.
 *   Runs on the context's stream and returns when the results are complete.  n == 0: HJ_OK, nothing touched.
 *   HJ_ERR_INVALID, checked before anything else and before the device is touched, in this order: null rays or counts (n > 0); null
 *     hits with K > 0 (n > 0); K above HJ_ALLHITS_MAX_HITS; unknown flag bits; n above 2^31 - 1; with device arrays, a misaligned
 *     array.  With a null context the text is in hj_last_error(NULL).  A refused call writes nothing.
 *   A null context: HJ_ERR_DEVICE in a process without a HIP device, HJ_ERR_INVALID otherwise.  HJ_ERR_STATE: hj_trace_rays'.
 *
 * hj_points_inside:  points: n x 4 floats (p.xyz, reserved).  Per point three rays from p with tMin = 0, tMax = +inf along
 *     HJ_INSIDE_DIR0, 1, 2 below - fixed, pairwise non-parallel, no zero component and no two components of one direction equal in
 *     magnitude, so that axis-aligned scenes are in general position; of length 1 to float32's rounding - through the counting walk
 *     without leaving the device.  A ray votes inside when its crossing sum is > 0; with HJ_INSIDE_PARITY, for surfaces without a
 *     consistent orientation, when its number of candidates is odd.
 *   out: n x 2 uint32 - [0] 1 when at least two rays vote inside, else 0; [1] the number of rays that voted inside.
 *   HJ_INSIDE_DEVICE_ARRAYS: as above.  HJ_ERR_INVALID in this order: null points or out (n > 0); unknown flag bits; n above
 *     2^31 - 1; a misaligned device array.  Then hj_trace_rays_all's gate.
 * Not here: a surface record per hit (the caller has id, t, u, v); K above 8; a multi-GPU split; hj_distance_field's sign and the
 *   probe classification do not use the count. */
#define HJ_ALLHITS_DEVICE_ARRAYS 1u
#define HJ_ALLHITS_MAX_HITS 8u
#define HJ_INSIDE_DEVICE_ARRAYS 1u
#define HJ_INSIDE_PARITY 2u
#define HJ_INSIDE_DIR0_X 0.28284273f
#define HJ_INSIDE_DIR0_Y 0.51961523f
#define HJ_INSIDE_DIR0_Z 0.8062258f
#define HJ_INSIDE_DIR1_X -0.84261495f
#define HJ_INSIDE_DIR1_Y 0.2236068f
#define HJ_INSIDE_DIR1_Z -0.48989794f
#define HJ_INSIDE_DIR2_X 0.5477226f
#define HJ_INSIDE_DIR2_Y -0.7745967f
#define HJ_INSIDE_DIR2_Z -0.31622776f
int hj_trace_rays_all(hj_context* ctx, const float* rays /* n x 8 */, size_t n, uint32_t max_hits, uint32_t flags,
                      uint32_t* counts /* n x 2 */, float* hits /* n x max_hits x 4; may be NULL with max_hits 0 */);
int hj_points_inside(hj_context* ctx, const float* points /* n x 4: p.xyz, reserved */, size_t n, uint32_t flags, uint32_t* out /* n x 2 */);

/* ------------------------------------------- frame AOVs and material queries */

/* Frame AOVs and material queries (ABI 0.26): what colour a surface has, and a frame's auxiliary buffers - albedo, normal, depth,
 * emission, coverage - from the frame's own primary rays (no counterpart in the reference, which evaluates a material only inside
 * its path loop).  The colour functions are the shade stage's own - the checkerboard (shader/materials/diffusecb.glsl) and the image
 * texture look-up (hj_texture above) -, called through one tag dispatch (kernels/hj_aov.h eval_material); tests/aov_ref.py restates
 * the contract in numpy.
 *
 * A material record, 8 floats: [0..2] albedo, [3] the uploaded material word as bits (tag << 24 | index), [4..6] emitted radiance,
 *   [7] 0.  By tag: HJ_MAT_DIFFUSE: albedo = the material's colour.  HJ_MAT_DIFFUSECBOARD: with fu = (0.5 * u) / scale_u and
 *   fv = (0.5 * v) / scale_v, each minus its floor, albedo = color_b when (fu < 0.5) != (fv < 0.5), else color_a - every operation
 *   float32.  HJ_MAT_DIFFUSE_TEXTURED: the texture look-up of texture `index` at (u, v).  HJ_MAT_MIRROR, HJ_MAT_DIELECTRIC: albedo
 *   (1, 1, 1).  HJ_MAT_EMISSIVE: albedo 0, emission = the material's power - what a path adds for a discrete hit at throughput 1.
 *   Everything not named is 0.  A miss - an id outside [0, shapes), -1 included - is all zero except word 3 = 0xFFFFFFFF.
 *
 * hj_eval_materials:  hits (n x 4) and surface (n x 16) are the two arrays hj_trace_rays writes: the shape id is hits[4i] as bits,
 *     (u, v) are surface[16i + 6] and surface[16i + 7].  The material word is read from the uploaded scene by id, not from
 *     surface[16i + 14]: a miss's all-zero record would read as "diffuse, index 0".  out: n material records.
 *   HJ_MATERIALS_DEVICE_ARRAYS: the three arrays are device pointers on the context's GPU, 16-byte aligned, used in place (the caller
 *     orders its own streams before the call).  Without it they are host arrays, staged in chunks of HJ_TRACE_CHUNK records.
 *   Runs on the context's stream and returns when the results are complete.  n == 0: HJ_OK, nothing touched.
 *   HJ_ERR_INVALID, checked before anything else and before the device is touched, in this order: a null array (n > 0); unknown flag
 *     bits; n above 2^31 - 1; with device arrays, a misaligned array.  With a null context the text is in hj_last_error(NULL).  A
 *     refused call writes nothing.  Then hj_trace_rays' gate: a null context (HJ_ERR_DEVICE in a process without a HIP device,
 *     HJ_ERR_INVALID otherwise); HJ_ERR_STATE for an asynchronous frame in flight, undrained frames, no scene.
 *
 * hj_render_aovs:  for every sample of every block - local pixel (lx, ly) with lx < dimension.x, ly < dimension.y and both inside
 *     original_dimension, exactly the samples hj_render_blocks takes - the camera ray of that sample (origin camera.position,
 *     tMin = eps, tMax = +inf) goes through the uploaded tree by the path kernel's walk, and its first hit is populated as the path
 *     kernel populates it (hit point fma(t, d, o)).  The sample's record, HJ_AOV_WORDS floats:
 *       [0..3] albedo.rgb, 1     [4..7] shading normal n.xyz, t     [8..11] emission.rgb, 1
 *     with albedo and emission as in a material record; a miss gives 0, 0, 0, 1 and eight zeros.
 *   aov: height x width x HJ_AOV_WORDS floats, OVERWRITTEN: pixel (origin + l) is the float32 sum of its samples' records, block by
 *     block in the order of the list, starting from +0; a pixel no sample covers is twelve zeros (a sample whose pixel lies outside
 *     the image is dropped).  So word 3 is the sample count, word 11 the hit count, words 4..6 over word 11 the mean normal, word 7
 *     over word 11 the mean depth of the hits, words 0..2 over word 3 the mean albedo.  A record depends on the blocks, the scene
 *     and the camera alone: not on HJ_TRACE_CHUNK, the workgroup count or the lane that carried a ray.
 *   Every block needs original_dimension == (width, height) and dimension <= HJ_BLOCK_SIZE per axis.  No framebuffer is needed, and
 *     the framebuffer and the batch slots are left alone, as by the queries.
 *   HJ_AOV_DEVICE_ARRAY: aov is a device pointer on the context's GPU, 16-byte aligned, written in place.
 *   HJ_ERR_INVALID, before the device is touched, in this order: null blocks (num_blocks > 0) or aov; unknown flag bits; a zero width
 *     or height or one above 16384; a block whose original_dimension differs or whose dimension is above HJ_BLOCK_SIZE; a misaligned
 *     device array.  Then hj_trace_rays' gate.  num_blocks == 0: HJ_OK behind the gate, with an all-zero output.
 * hj_render_aovs_frame:  hj_render_aovs over exactly the block list hj_render_frame generates for world == 1 with the same spp,
 *     master_seed and pass range (width x height takes the framebuffer's place): the AOVs of that frame's primary rays.  Behind the
 *     refusals above: pass_begin > pass_end or pass_end > spp is HJ_ERR_INVALID.  An empty pass range: HJ_OK, an all-zero output.
 * Not here: an environment's radiance for a miss; a material at a closest-point or all-hit record (those carry no texture
 *   coordinates yet); a multi-GPU split.  (Following mirror or glass to the first diffuse surface: hj_render_aovs_followed below.  A
 *   denoiser: hj_denoise_frame below.) */
#define HJ_MATERIALS_DEVICE_ARRAYS 1u
#define HJ_MATERIALS_WORDS 8
#define HJ_AOV_DEVICE_ARRAY 1u
#define HJ_AOV_WORDS 12
int hj_eval_materials(hj_context* ctx, const float* hits /* n x 4 */, const float* surface /* n x 16 */, size_t n, uint32_t flags,
                      float* out /* n x 8 */);
int hj_render_aovs(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height, uint32_t flags,
                   float* aov /* height x width x 12 */);
int hj_render_aovs_frame(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin,
                         uint32_t pass_end, uint32_t flags, float* aov /* height x width x 12 */);

/* Followed AOVs (ABI 0.30): what a mirror or glass SHOWS.  hj_render_aovs stops at the first hit, so a pixel on a mirror or on glass
 * gets the guide of the mirror itself - albedo 1, the sphere's normal, the sphere's depth - and nothing in it separates the red wall
 * from the white floor inside a reflection.  The calls below take the chain through specular surfaces that the path kernel takes
 * (kernels/hj_stages.h stage_shade), made deterministic: an AOV cannot toss the Fresnel coin.  The continuation is one text
 * (kernels/hj_follow.h follow_continue) for the per-record query and the frame kernel; tests/follow_ref.py restates it in numpy.
 *
 * The specular continuation of a ray (o, d) with raw hit (id, t, u, v):  hit point p = fma(t, d, o), populated as the path kernel
 *   populates it (shading normal n).  The material word is read from the uploaded scene by id.
 *     HJ_MAT_MIRROR:      wo = reflect(d, n) = d - n * (2 * dot(n, d)) - about the stored normal, from the back side too.
 *     HJ_MAT_DIELECTRIC:  the path kernel's expressions, float32, no contraction, in this order: eta = the material's, etaInv = 1 / eta,
 *       cosI = -dot(n, d), normal = n; when cosI < 0: eta = etaInv, etaInv = 1 / eta, normal = -normal, cosI = -cosI.
 *       k = 1 - (etaInv * etaInv) * (1 - cosI * cosI).  When k > 0: cosO = sqrt(k), rpar = (eta * cosI - cosO) / (eta * cosI + cosO),
 *       rorth = (cosI - eta * cosO) / (cosI + eta * cosO), fr = 0.5 * (rpar * rpar + rorth * rorth).
 *       The branch, without the random draw: reflect when k <= 0 or fr >= 0.5f, else refract - the branch the path kernel takes more
 *       often than not.  Reflect: wo = reflect(d, normal).  Refract: par = d - normal * dot(d, normal), wo = par * etaInv - normal *
 *       cosO, not normalised, as the reference leaves it.
 *     Every other tag, a miss, an id outside the scene: the chain ends here.
 *   The continued ray is (p, wo, tMin = eps, tMax = +inf): the next segment of a path.
 *   A record no walk gives - t, d, u or v not finite, or a product that overflows - can make words of p and wo NaN.  Such a word is
 *   a NaN and no more is promised of it: the sign and payload of a NaN that an operation generates (inf - inf, 0 * inf) differ
 *   between processors.  Which words are NaN, and every bit of every other word, is as the expressions above say.
 *
 * hj_follow_specular:  rays (n x 8) and hits (n x 4) are hj_trace_rays' ray layout and hit records; out_rays (n x 8) gets per record
 *     the continued ray in the same layout, and where the chain ends the empty ray: origin and direction 0, tMin = +inf, tMax = -inf -
 *     hj_trace_rays answers it with a miss.  hj_follow_specular and hj_trace_rays alternated by the caller give exactly the chain of
 *     the frame calls below.
 *   HJ_FOLLOW_DEVICE_ARRAYS: the three arrays are device pointers on the context's GPU, 16-byte aligned, used in place.  Without it
 *     they are host arrays, staged in chunks of HJ_TRACE_CHUNK records.  Runs on the context's stream and returns when the results
 *     are complete.  n == 0: HJ_OK, nothing touched.
 *   HJ_ERR_INVALID, before the device is touched, in this order: a null array (n > 0); unknown flag bits; n above 2^31 - 1; with
 *     device arrays, a misaligned array.  A refused call writes nothing.  Then hj_trace_rays' gate.
 *
 * hj_render_aovs_followed:  hj_render_aovs with one more argument, max_follow in 0 ... HJ_AOV_MAX_FOLLOW.  Same image layout, same
 *     block order, same flags.  A sample's chain starts with its camera ray, exactly as there.  While the last hit is a mirror or a
 *     dielectric and fewer than max_follow continuations have been taken, the chain continues by the rule above and is walked again -
 *     the same closest-hit walk.  The sample's record is the record of the chain's LAST hit: albedo and emission of the material at
 *     that hit, its shading normal, 1 for the hit; the depth word [7] is the float32 sum of the chain's t values in chain order,
 *     (t0 + t1) + t2 ... - the point at that depth along the camera ray is where a planar mirror's virtual image lies.
 *   A continuation that hits nothing leaves the record of the surface it left: albedo 1, that surface's normal, the sum so far, hit
 *     1 - so coverage, word 11, is exactly hj_render_aovs'.  A chain cut off by max_follow ends on its last specular hit the same way.
 *     A camera ray that misses gives the miss record.  max_follow == 0 is hj_render_aovs bit for bit, through the same launches.
 *   A record depends on the blocks, the scene, the camera and max_follow alone: not on HJ_TRACE_CHUNK or the lane that carried a chain.
 *   The context holds 36 bytes more per sample slot of one walk launch (HJ_TRACE_CHUNK): never a frame's worth.
 *   HJ_ERR_INVALID, before the device is touched: hj_render_aovs' refusals in their order, then max_follow above HJ_AOV_MAX_FOLLOW.
 *     Then hj_trace_rays' gate.
 * hj_render_aovs_frame_followed:  hj_render_aovs_frame with max_follow.  hj_render_aovs' refusals, then max_follow above
 *     HJ_AOV_MAX_FOLLOW, then the bad pass range; then the gate.
 * Not here: glass extinction does not tint the followed albedo (a dielectric's albedo stays 1 along the chain); a glossy lobe - the
 *   project has no such material; hj_render_motion still stops at the first hit: hj_render_motion_followed (ABI 0.31) follows these
 *   chains; a multi-GPU split. */
#define HJ_AOV_MAX_FOLLOW 8
#define HJ_FOLLOW_DEVICE_ARRAYS 1u
int hj_follow_specular(hj_context* ctx, const float* rays /* n x 8, hj_trace_rays' layout */, const float* hits /* n x 4, hj_trace_rays' records */,
                       size_t n, uint32_t flags, float* out_rays /* n x 8 */);
int hj_render_aovs_followed(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height,
                            uint32_t max_follow, uint32_t flags, float* aov /* height x width x 12 */);
int hj_render_aovs_frame_followed(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin,
                                  uint32_t pass_end, uint32_t max_follow, uint32_t flags, float* aov /* height x width x 12 */);

/* Probe-lit frames (ABI 0.32): the frame a probe volume is for.  The samples are exactly hj_render_aovs_followed's - the same blocks,
 * seeds and sample offsets, the same chains through at most max_follow specular surfaces - and each sample's last diffuse hit is lit
 * from the volume by the look-up the caller selects: noise-free diffuse lighting at the cost of a first-hit walk, with mirrors and
 * glass showing the lit scene.  No counterpart in the reference; tests/probe_lit_ref.py restates the contract in numpy.
 *
 * hj_probe_lighting:  desc is the volume's grid (hj_probe_desc, as the look-ups take it); its flags - with vis, vis->flags, which must
 *     agree - say whether probes, atlas and placement are host arrays or device pointers, as in the look-up selected:
 *       vis == NULL                      hj_sample_probes: the trilinear and validity weights alone; atlas and placement are not read
 *       vis != NULL, placement == NULL   hj_sample_probes_visible, with vis' normal_bias and its two switches
 *       vis != NULL, placement != NULL   hj_sample_probes_visible_placed
 *     Host arrays are staged once a call.
 * hj_render_probe_lit:  every sample's chain is hj_render_aovs_followed's.  Its radiance L, float32:
 *     - the chain's last hit is a mirror or a dielectric (the cap, max_follow, cut it there; max_follow == 0: the first hit is one):
 *       L = that surface's emission, which a material record has as 0.  No diffuse term.
 *     - any other hit: with (albedo, n, Le) the words of hj_render_aovs' record at the last hit and p the populated hit point the
 *       record is built from (fma(t, d, o) over the chain's last segment), E = words 0..2 of the selected look-up at the 8-word point
 *       (p, n, 0, 0), bit for bit what that call writes to `out`, and
 *           L[c] = Le[c] + (albedo[c] * E[c]) * 0.318309886f
 *       one rounding each, no contraction, in that order.  The constant is the shade stage's own 1 / pi (1.0f / 3.14159274f), whose
 *       bits are the literal's.
 *     - nothing was hit, from the camera or after leaving a specular surface, and hj_scene_upload_env is in effect: L = the
 *       environment's radiance along the last segment's direction, as hj_debug_env_lookup gives it for that direction.
 *     - nothing was hit and there is no environment: L = 0.
 *   image: height x width x HJ_PROBE_LIT_WORDS floats, OVERWRITTEN: words 0..2 of pixel (origin + l) are the float32 sums of L over its
 *     samples, block by block in the order of the list, starting from +0; word 3 is the count of its samples, every one of them, so
 *     rgb / count is the mean radiance.  A pixel no sample covers is four zeros.  A sample depends on the blocks, the scene, the
 *     camera, max_follow and the volume alone: not on HJ_TRACE_CHUNK or the lane that carried a chain.
 *   What E holds is what the volume was baked from: hj_bake_probes' gather counts a first segment that ends on an emitter (or leaves
 *     into the environment) with its radiance, so DIRECT light is in E beside the indirect, band-limited to nine SH coefficients a
 *     probe and interpolated between probes - soft where a traced shadow is sharp.  An emitter seen directly adds its Le here.
 *   HJ_AOV_DEVICE_ARRAY: image is a device pointer on the context's GPU, 16-byte aligned, written in place.
 *   No framebuffer is needed, and the framebuffer and the batch slots are left alone.  The context holds 64 bytes more per sample slot
 *     of one walk launch (HJ_TRACE_CHUNK) - the look-up point, the look-up's record, a side record (Le, kind) - beside
 *     hj_render_aovs_followed's, and the staging of host-side volume arrays.
 *   HJ_ERR_INVALID, before the device is touched, in this order: hj_render_aovs' refusals (the image in aov's place); max_follow above
 *     HJ_AOV_MAX_FOLLOW; a null lighting; a placement without vis; then the refusals of the look-up selected, in that call's order, the
 *     points and `out` - this call's own - aside: a null desc, vis, placement, probes or atlas (probes and a read atlas: with
 *     num_blocks > 0), the descs' refusals, misaligned device arrays, a non-finite offset in a host-side placement.  A refused call
 *     writes nothing.  Then hj_trace_rays' gate.  num_blocks == 0: HJ_OK behind the gate, an all-zero image.
 * hj_render_probe_lit_frame:  hj_render_probe_lit over exactly the block list hj_render_frame generates for world == 1 with the same
 *     spp, master_seed and pass range.  The bad pass range (pass_begin > pass_end or pass_end > spp) is refused behind max_follow, before
 *     the lighting.  An empty pass range: HJ_OK, an all-zero image.
 * Not here: a glossy lobe - the project has no such material; glass extinction along the chain; lighting from a baked light map; a
 *   multi-GPU split; a flag of the command-line tool; separately traced direct shadows - direct light is as soft as the volume has it.
 *   (For those: hj_render_direct_lit, below, with a volume baked HJ_PROBES_INDIRECT_ONLY.) */
#define HJ_PROBE_LIT_WORDS 4
typedef struct hj_probe_lighting {
  const hj_probe_desc*     desc;       /* the volume's grid; its flags say host or device arrays for probes / atlas / placement */
  const hj_probe_vis_desc* vis;        /* NULL: hj_sample_probes' weights alone                                                   */
  const float*             probes;     /* n x 28                                                                                   */
  const float*             atlas;      /* with vis, as hj_sample_probes_visible takes it                                           */
  const float*             placement;  /* NULL, or n x 4 as hj_sample_probes_visible_placed takes it (needs vis)                   */
} hj_probe_lighting;
int hj_render_probe_lit(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height,
                        uint32_t max_follow, uint32_t flags, const hj_probe_lighting* lighting, float* image /* height x width x 4 */);
int hj_render_probe_lit_frame(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin,
                              uint32_t pass_end, uint32_t max_follow, uint32_t flags, const hj_probe_lighting* lighting,
                              float* image /* height x width x 4 */);

/* Direct-lit frames (ABI 0.33): hj_render_probe_lit with one traced next-event sample at each chain's last diffuse hit - sharp direct
 * shadows beside the volume's indirect light, at the cost of one extra any-hit round.  Arguments, samples, chains, blocks, runs and the
 * block-order float32 sums are exactly hj_render_probe_lit's; lighting may be NULL, which means direct light alone.  No counterpart in
 * the reference; tests/direct_lit_ref.py restates the contract in numpy over the oracle's shade step.
 *
 * hj_render_direct_lit:  per sample, with Lp the L hj_render_probe_lit defines (lighting == NULL: E is absent and Lp = Le for a hit, the
 *     environment or 0 for a miss):
 *     - the direct term applies when the chain's last hit carries one of the three diffuse tags (HJ_MAT_DIFFUSE, HJ_MAT_DIFFUSECBOARD,
 *       HJ_MAT_DIFFUSE_TEXTURED).  Emitters, mirrors and glass (the cap cut the chain there) and misses get none.
 *     - the sample: rng = seedRng(seed) of the sample's own seed (block.seed + lx + ly * dimension.x: the state the camera ray leaves;
 *       a chain draws nothing, so a followed sample uses the same state); imp, sdir, stmax = the shade stage's next-event sample of
 *       the emitters at p from rng (with an uploaded environment its environment form), (p, n, albedo) being the words of Lp's record.
 *     - the term exists iff length(imp) > eps and dot(sdir, n) > 0, the shade stage's condition, and then
 *           D = ((albedo * dot(n, sdir)) * 0.318309886f) * imp
 *       in the shade stage's operation order with throughput 1, one rounding each, no contraction.
 *     - D counts iff the shade stage's shadow ray finds nothing: from p along sdir with tMin = 2 eps and tMax = stmax (+inf for an
 *       environment sample), any-hit, walked on the uploaded tree.
 *     - L = Lp + D, one rounding a channel, when D counts; otherwise L = Lp and no addition is taken.
 *   Corollary: with max_follow == 0 and lighting == NULL or an all-zero volume, a sample's L is bit for bit the radiance hj_trace_paths
 *     returns for that camera ray with spp = 1, the sample's seed and max_bounces = 1 (the shade stage takes the first hit's next-event
 *     sample before its bounce limit ends the path).
 *   With a volume baked HJ_PROBES_INDIRECT_ONLY the frame has direct light once; with a plain volume it has it twice (E holds it
 *     already).  The call does not and cannot check this.
 *   image, HJ_AOV_DEVICE_ARRAY, the independence of HJ_TRACE_CHUNK: as hj_render_probe_lit.  The context holds 48 bytes more per sample
 *     slot of one walk launch - the shadow ray and the pending D - and the list of the slots that want a ray (the chain rounds' own).
 *   HJ_ERR_INVALID: hj_render_probe_lit's refusals in its order under this call's name, but a null lighting is accepted, and nothing
 *     of a volume is then checked or staged.  A refused call writes nothing.  Then hj_trace_rays' gate.  num_blocks == 0: HJ_OK
 *     behind the gate, an all-zero image.
 * hj_render_direct_lit_frame:  hj_render_direct_lit over hj_render_probe_lit_frame's block list; the bad pass range as there.
 * Not here: more than one light sample a hit, stratified lights; the light-shaft grid's proven-free shortcut (every wanted ray is
 *   traced; the image would be the same bits either way); glass extinction along the chain; a glossy lobe; light-map indirect; a
 *   multi-GPU split; a flag of the command-line tool. */
int hj_render_direct_lit(hj_context* ctx, const hj_image_block* blocks, size_t num_blocks, uint32_t width, uint32_t height,
                         uint32_t max_follow, uint32_t flags, const hj_probe_lighting* lighting /* may be NULL */,
                         float* image /* height x width x 4 */);
int hj_render_direct_lit_frame(hj_context* ctx, uint32_t width, uint32_t height, uint32_t spp, uint64_t master_seed, uint32_t pass_begin,
                               uint32_t pass_end, uint32_t max_follow, uint32_t flags, const hj_probe_lighting* lighting /* may be NULL */,
                               float* image /* height x width x 4 */);

/* ------------------------------------------- frame denoiser */

/* hj_denoise_frame (ABI 0.27): the spatial filter of SVGF (Schied et al. 2017: its variance-guided a-trous stage) over one frame on
 * the device, guided by the frame's AOVs - the first consumer of hj_render_aovs.  It filters albedo-demodulated light, so textures
 * and the checkerboard stay sharp; a 5 x 5 B3-spline kernel whose taps move apart by powers of two, with edge stops on normal,
 * depth (relative to the local depth slope), albedo and luminance, the last scaled by a per-pixel variance that is itself
 * filtered.  No counterpart in the reference; tests/denoise_ref.py restates the contract in numpy.
 *   beauty: height x width x 4 floats in the framebuffer's format, (sum w * rgb, sum w), row y = 0 first.  NULL: the context's
 *     bound framebuffer is read on the device; it must be width x height (HJ_ERR_INVALID behind the gate otherwise; HJ_ERR_STATE
 *     when the context has none).  The framebuffer is read, never written.
 *   aov: height x width x HJ_AOV_WORDS floats, as hj_render_aovs writes it.      out: height x width x 4 floats; never aliases an input.
 *   Every operation is float32 with one rounding and no contraction: no fused multiply-add outside hj_exp; / and sqrtf are IEEE.
 *       sq(v) = (v.x * v.x + v.y * v.y) + v.z * v.z        Y(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 *       k = {0.375f, 0.25f, 0.0625f}
 *   Computed on the host, once: inn = sigma_normal > 0 ? 1.0f / (sigma_normal * sigma_normal) : 0.0f; ia the same of sigma_albedo;
 *   sz = sigma_depth and sl = sigma_luminance, where 0 switches the term off.
 *   PREPARE, per pixel, with S = aov[3], Hc = aov[11], bw = beauty[3]:  a pixel is LIT when aov[8], aov[9] or aov[10] is above 0 -
 *     a sample of it saw an emitter directly.  The pixel is GUIDED when Hc > 0 and bw > 0 and no in-image pixel of the 5 x 5
 *     window around it, itself included, is lit.  (The framebuffer holds light spread by the reconstruction filter, radius 2: a
 *     directly seen emitter's radiance reaches the pixels within two of it, while the AOVs are per pixel and know nothing of
 *     that.  Those pixels, and the emitter's own - noise-free but for their edges - are passed through, or the filter would pull
 *     the halo down to its surroundings' level and raise the frame's error instead of lowering it.)
 *     c = beauty.rgb / bw per channel, or +0 when bw is not above 0.
 *     A_ch = fmaxf(aov[ch] / S, 0.015625f) for ch = 0, 1, 2 - the floor keeps black surfaces (albedo 0) finite: such pixels are
 *       filtered undemodulated up to a constant.          I = c / A per channel.
 *     n = aov[4..6] / Hc, not renormalised.          z = aov[7] / Hc.
 *     A pixel that is not guided has the output (c, 0); it is copied through every iteration and is never a tap.
 *   SLOPE AND INITIAL VARIANCE, per guided pixel at (x, y):
 *     gz.x: of the forward difference z[x + 1] - z and the backward difference z - z[x - 1] the one with the smaller magnitude;
 *       only differences whose neighbour is in the image and guided count; a tie takes the forward one; none: +0.  (The smaller
 *       one keeps a depth edge from inflating its own slope.)          gz.y: the same along y.
 *     V: over the guided in-image pixels q of the 5 x 5 window at step 1 (dy = -2 ... 2 outer, dx = -2 ... 2 inner, the pixel
 *       itself included), from m1 = m2 = cnt = +0:  m1 = m1 + Y(I_q);  m2 = m2 + Y(I_q) * Y(I_q);  cnt = cnt + 1.0f.  Then
 *       mu = m1 / cnt and V = fmaxf(m2 / cnt - mu * mu, 0.0f).
 *   ITERATION i = 0 ... iterations - 1, step s = 1 << i, reads (I, V) and writes (I', V'), per guided pixel p = (x, y):
 *     vbar: over the guided in-image pixels q of the 3 x 3 window at step 1 WHATEVER s is (dy = -1 ... 1 outer, dx = -1 ... 1
 *       inner), with g = {0.25f, 0.125f, 0.0625f}[|dx| + |dy|], from vsum = gsum = +0:  vsum = vsum + V_q * g;  gsum = gsum + g.
 *       vbar = vsum / gsum.          sd = sqrtf(vbar).
 *     sum = (+0, +0, +0), vs = +0, ws = +0, then for dy = -2 ... 2 (outer), dx = -2 ... 2 (inner):
 *       0. the tap is q = (x + dx * s, y + dy * s); it is skipped when it lies outside the image or is not guided;
 *       1. h = k[|dx|] * k[|dy|] (the products are exact);
 *       2. en = sq(n_q - n) * inn;
 *       3. ez = fabsf(z_q - z) / (sz * fabsf(gz.x * (float)(dx * s) + gz.y * (float)(dy * s)) + 1e-6f), or +0 when sz == 0;
 *       4. el = fabsf(Y(I_q) - Y(I)) / (sl * sd + 1e-6f), or +0 when sl == 0;
 *       5. ea = sq(A_q - A) * ia;
 *       6. w = h * hj_exp(-(((en + ez) + el) + ea)) - the numeric contract's exp (kernels/hj_num.h; HJ_NUM_EXP of hj_debug_num);
 *       7. sum.r = sum.r + I_q.r * w, likewise g and b;  vs = vs + V_q * (w * w);  ws = ws + w.
 *     I' = sum / ws, one division per channel;  V' = vs / (ws * ws).  For finite data the centre tap alone gives ws >= 0.140625.
 *   FINISH: for a guided pixel out.rgb = I * A, one multiply per channel, and out.a = V.
 *   iterations == 0: the prepare stage still runs; the output is the demodulate / remodulate round trip with the initial variance
 *   in word 3.  The result depends on (width, height, beauty, aov, opts) alone: not on the kernel form (HJ_DENOISE_LDS_STEP), the
 *   launch shape or any tuning switch.  Agreement bit for bit with this text is claimed for finite inputs; non-finite values
 *   just propagate.
 *   HJ_DENOISE_DEVICE_ARRAYS (opts->flags): beauty (when not NULL), aov and out are device pointers on the context's GPU, 16-byte
 *     aligned, used in place on the context's stream; the call returns after one synchronisation, and the inputs are left as they
 *     were.  Without the flag they are host arrays, staged through buffers the context keeps.
 * The context keeps 48 bytes per pixel of guide data and two working images, grown on demand, freed with the context.
 * HJ_ERR_INVALID, before the device is touched, in this order, each with its text in hj_last_error behind "hj_denoise_frame:": a
 *   null opts, aov or out; unknown flag bits; iterations above 8; a negative or non-finite sigma; a zero width or height or one
 *   above 16384; a misaligned device array.  A refused call writes nothing.  Then hj_trace_rays' gate - a null context
 *   (HJ_ERR_DEVICE in a process without a HIP device, HJ_ERR_INVALID otherwise); HJ_ERR_STATE for an asynchronous frame in flight or
 *   undrained frames - except that no scene is needed: this call traces nothing.
 * The defaults of the Python wrapper and the command line (5 iterations; sigmas 0.5 normal, 1 depth, 4 luminance, 0.1 albedo) are
 *   SVGF's starting points where it has them (depth, luminance) and guesses elsewhere: they are not tuned.
 * Not here: a multi-GPU split; tuned defaults.  (Temporal accumulation and reprojection: hj_denoise_frame_temporal below.) */
#define HJ_DENOISE_DEVICE_ARRAYS 1u
#define HJ_DENOISE_MAX_ITERATIONS 8u
typedef struct hj_denoise_opts {
  uint32_t iterations;       /* 0 ... 8; iteration i uses the step s = 1 << i */
  float    sigma_normal;     /* on |n_q - n|; 0 = stop off */
  float    sigma_depth;      /* in units of the local depth slope; 0 = off */
  float    sigma_luminance;  /* in standard deviations of the demodulated luminance; 0 = off */
  float    sigma_albedo;     /* on |A_q - A|; 0 = off */
  uint32_t flags;            /* HJ_DENOISE_DEVICE_ARRAYS */
} hj_denoise_opts;
int hj_denoise_frame(hj_context* ctx, uint32_t width, uint32_t height,
                     const float* beauty /* H x W x 4; NULL = the context's framebuffer */,
                     const float* aov    /* H x W x HJ_AOV_WORDS, as hj_render_aovs writes it */,
                     const hj_denoise_opts* opts, float* out /* H x W x 4 */);

/* hj_denoise_frame_temporal (ABI 0.28): the temporal half of SVGF in front of hj_denoise_frame's filter - the last frame's
 * accumulated light and luminance moments are reprojected into this frame through the two cameras, tested against this frame's depth
 * and normal, and blended with the new sample; the filter then runs over the accumulated light, and a pixel whose history is
 * HJ_TEMPORAL_VARIANCE_FRAMES long is given its temporal variance instead of the 5 x 5 spatial estimate.  No counterpart in the
 * reference; tests/temporal_ref.py restates the contract in numpy.
 *   beauty, aov, opts and out mean exactly what they mean for hj_denoise_frame, beauty == NULL included; HJ_DENOISE_DEVICE_ARRAYS in
 *     opts->flags covers all five arrays.  The cameras come in the options, not from a scene: as with hj_denoise_frame, no scene is
 *     needed and the call traces nothing.  The caller holds the history, as it holds a probe volume's values across
 *     hj_update_probes, and swaps the two history arrays between frames.
 *   A history record, HJ_TEMPORAL_WORDS floats per pixel: [0..2] the accumulated demodulated light I; [3] the history length N as a
 *     float; [4] m1 and [5] m2, the moments of Y(I); [6] z; [7] the valid word (1u as bits, or 0); [8..10] n; [11] 0.  A pixel
 *     that is not guided writes twelve zeros.
 *   Every operation is float32 with one rounding and no contraction, except inside the camera arithmetic named below, which is the
 *   shader's: its dot3 and cross3 are the numeric contract's (kernels/hj_num.h: fmaf inside; HJ_NUM_DOT3, HJ_NUM_CROSS3 and
 *   HJ_NUM_NORMALIZE3 of hj_debug_num).  sq and Y are hj_denoise_frame's.
 *       rotate(v, q): with qv = q.xyz, qw = q.w:  tw = qw * 0.0f - dot3(qv, v);  c1 = cross3(qv, v);
 *         t = (c1 + qv * 0.0f) + v * qw per channel;  c2 = cross3(t, -qv);  the result is (c2 + t * qw) + (-qv) * tw per channel
 *         (quaternionRotate, shader/quaternion.glsl, in camera_ray's operation order).        conj(q) = (-q.xyz, q.w).
 *       tan(cam) = (float)tan((double)(0.5f * cam.fov) * (3.14159265358979323846 / 180.0)), computed on the host as the upload computes it.
 *   1. PREPARE is hj_denoise_frame's, unchanged: guided or not, c, A, I_cur = I, n and z.
 *   2. REPROJECT, per guided pixel (x, y), when history_in is not NULL, with W = (float)width, H = (float)height:
 *     d is camera_ray's arithmetic with px = (float)x + 0.5f, py = (float)y + 0.5f and topts->camera:  u = px - 0.5f * W,
 *       v = py - 0.5f * H;  u = (u * tan(camera)) / (0.5f * W), v = (v * tan(camera)) / (0.5f * W);
 *       d = normalize3(rotate((u, -v, -1.0f), camera.rotation)).
 *     P = position + z * d, one multiply and one add per channel.          v = P - prev.position.
 *     c = rotate(v, conj(prev.rotation)).          There is no history unless c.z < 0.
 *     k = (0.5f * W) / tan(prev).     sx = (c.x / -c.z) * k + 0.5f * W.     sy = (-c.y / -c.z) * k + 0.5f * H.
 *     fx = sx - 0.5f, ix = floorf(fx), tx = fx - ix; the same along y.          zp = sqrtf(sq(v)).
 *     The four taps (ix + a, iy + b), a, b = 0, 1, are taken in the order b outer, a inner, from sum = +0 and ws = +0.  A tap has the
 *       bilinear weight w = wx * wy, wx = 1.0f - tx for a = 0 and tx for a = 1, wy likewise of ty and b.  A tap counts when it is in
 *       the image, its valid word is not 0, fabsf(z_h - zp) <= depth_tolerance * zp, and
 *       (n_h.x * n.x + n_h.y * n.y) + n_h.z * n.z >= normal_cos.  For a tap that counts: sum = sum + value_h * w for each of
 *       I.r, I.g, I.b, m1, m2 and N;  ws = ws + w.
 *     There is no history when no tap counts or ws is not above 0.  Otherwise I_prev, m1_prev, m2_prev and N_prev are sum / ws,
 *       one division each.
 *   3. ACCUMULATE:  without history I = I_cur, m1 = Y(I_cur), m2 = m1 * m1, N = 1.  With history
 *       N = fminf(N_prev + 1.0f, (float)max_history);  a = fmaxf(alpha, 1.0f / N);  I = I_prev * (1.0f - a) + I_cur * a per channel;
 *       am = fmaxf(alpha_moments, 1.0f / N);  m1 = m1_prev * (1.0f - am) + Y(I_cur) * am;  m2 = m2_prev * (1.0f - am) + (Y(I_cur) * Y(I_cur)) * am.
 *   4. VARIANCE:  the slope gz is hj_denoise_frame's.  V is its 5 x 5 spatial estimate over the accumulated I when
 *       N < HJ_TEMPORAL_VARIANCE_FRAMES; otherwise V = fmaxf(m2 - m1 * m1, 0.0f).
 *   5. ITERATIONS and FINISH are hj_denoise_frame's, over (I, V).
 *   6. HISTORY OUT:  a guided pixel writes (I, N), (m1, m2, z, valid) and (n, 0).  With HJ_TEMPORAL_FEEDBACK and iterations >= 1, I in
 *       the history is the I' of the first iteration (step 1) - SVGF's feedback; without the flag it is the accumulated I of step 3.
 *   So history_in == NULL gives an out that is hj_denoise_frame's bit for bit, and so does a history whose valid words are all 0 or
 *   a prev_camera that looks the other way - in either kernel form.  Agreement bit for bit with this text is claimed for finite
 *   inputs; non-finite values just propagate.  A moved shape is met by the depth and normal tests alone, which reset its history
 *   (hj_denoise_frame_temporal_motion follows it).
 * The context keeps, beside hj_denoise_frame's buffers, the staging of the two histories when they are host arrays.
 * HJ_ERR_INVALID, before the device is touched, in this order, each with its text in hj_last_error behind
 *   "hj_denoise_frame_temporal:": hj_denoise_frame's own list up to the image size, with topts and history_out joining the null
 *   check (opts, topts, aov, history_out, out); unknown topts->flags bits; alpha or alpha_moments outside [0, 1] or NaN;
 *   depth_tolerance negative or non-finite; normal_cos outside [-1, 1] or NaN; max_history 0 or above 65535; a camera field that is
 *   not finite, or a fov outside (0, 180); history_out aliasing any input or out; a misaligned device array.  A refused call
 *   writes nothing.  Then hj_denoise_frame's gate.
 * The defaults of the Python wrapper: alpha 0.2 and alpha_moments 0.2 are SVGF's; depth_tolerance 0.1, normal_cos 0.9 and
 *   max_history 64 are guesses: they are not tuned.
 * Not here: motion vectors for moved shapes: hj_render_motion and hj_denoise_frame_temporal_motion below; SVGF's 3 x 3 fallback search
 *   when the bilinear taps fail; history for pixels that are not guided (lit or missed); a flag of the command line; a multi-GPU
 *   split; tuned defaults. */
#define HJ_TEMPORAL_WORDS 12
#define HJ_TEMPORAL_FEEDBACK 1u
#define HJ_TEMPORAL_VARIANCE_FRAMES 4u
typedef struct hj_temporal_opts {
  hj_camera camera;          /* the camera (beauty, aov) were rendered with */
  hj_camera prev_camera;     /* the camera of the frame that wrote history_in */
  float     alpha;           /* floor of the new colour's blend weight, 0 ... 1 */
  float     alpha_moments;   /* the same for the two luminance moments */
  float     depth_tolerance; /* relative: |z_hist - zp| <= depth_tolerance * zp; finite, >= 0 */
  float     normal_cos;      /* a tap needs dot(n_hist, n) >= normal_cos; -1 ... 1 */
  uint32_t  max_history;     /* 1 ... 65535: cap of the stored history length */
  uint32_t  flags;           /* HJ_TEMPORAL_FEEDBACK */
} hj_temporal_opts;
int hj_denoise_frame_temporal(hj_context* ctx, uint32_t width, uint32_t height, const float* beauty, const float* aov,
                              const hj_denoise_opts* opts, const hj_temporal_opts* topts,
                              const float* history_in  /* H x W x 12, or NULL: no history */,
                              float* history_out       /* H x W x 12, never aliases an input */,
                              float* out               /* H x W x 4 */);

/* hj_render_motion (ABI 0.29): per-pixel motion for the temporal denoiser - for every pixel (x, y), where the surface point that the
 * pixel's centre ray sees in the CURRENT frame was in the PREVIOUS frame: a position in the previous image and a distance from the
 * previous camera, the (sx, sy, zp) of hj_denoise_frame_temporal's step 2 with the point carried back onto the previous shape.  No
 * counterpart in the reference; tests/motion_ref.py restates the contract in numpy.
 *   The current frame is the scene as uploaded - after hj_scene_update_shapes the updated shapes and camera.  prev says how the scene
 *     stood in the previous frame, in the form hj_scene_update_shapes reads: prev->camera is the previous camera; prev->spheres,
 *     prev->quads and prev->vertices carry the same counts as the uploaded scene.  bvh, triangles, materials, emitters and the
 *     material records are not read: the index triples are the uploaded ones.  A shape array that is NULL with its count equal to
 *     the uploaded count means that kind did not move: the uploaded array stands in for it.  The ordinary frame loop: move the
 *     shapes, hj_scene_update_shapes, hj_render_motion against the old arrays.
 *   motion: height x width records of HJ_MOTION_WORDS floats, pixel (x, y) at record y * width + x:  (sx, sy, zp, id as bits), or
 *     (0, 0, 0, HJ_MOTION_NONE) for a pixel without a previous position.
 *   Every operation is float32 with one rounding and no contraction, except inside rotate, normalize3, dot3, cross3 (the numeric
 *   contract's, as for hj_denoise_frame_temporal) and the hit point.  rotate, conj, tan and sq are hj_denoise_frame_temporal's;
 *   W = (float)width, H = (float)height.
 *   RAY.  d is step 2's d with px = (float)x + 0.5f, py = (float)y + 0.5f, the uploaded scene's camera and its tan as the upload
 *     computes it.  The ray has the origin o = camera.position, tMin = eps (1e-4f) and tMax = +inf, and goes through the uploaded
 *     tree by the path kernel's walk, as a frame's primary rays and hj_trace_rays' do: the result is hj_trace_rays' (id, t, u, v).
 *   MISS.  A miss is an id outside [0, shapes): the record is (0, 0, 0, HJ_MOTION_NONE).
 *   PREVIOUS POINT Pp, per channel:
 *     sphere id:   P = fma(t, d, o), the shade stage's hit point.  n = (P - c) * (1.0f / r) with (c, r) the uploaded sphere: one
 *                  reciprocal, then one multiply per channel (the numeric contract's vector / scalar, as the shade stage's sphere
 *                  normal).  Pp = c' + n * r' with (c', r') the previous sphere.
 *     quad:        Pp = (o' + e1' * u) + e2' * v with (o', e1', e2') the previous quad.
 *     triangle:    l0 = (1.0f - u) - v.  Pp = (a' * l0 + b' * u) + c' * v with a', b', c' the previous positions of the uploaded
 *                  index triple.
 *   PROJECTION, step 2's words with prev->camera:  vv = Pp - prev.position.  c = rotate(vv, conj(prev.rotation)).  If c.z < 0 is
 *     false the record is (0, 0, 0, HJ_MOTION_NONE).  Otherwise k = (0.5f * W) / tan(prev);  sx = (c.x / -c.z) * k + 0.5f * W;
 *     sy = (-c.y / -c.z) * k + 0.5f * H;  zp = sqrtf(sq(vv)).  The record is (sx, sy, zp, id as bits).
 *   A record depends on the uploaded scene, prev and (width, height) alone: not on the lane, the workgroup count, the grouping of
 *   pixels into waves or any tuning switch.  Agreement bit for bit with this text is claimed for finite inputs.
 *   HJ_MOTION_DEVICE_SHAPES: prev->spheres / quads / vertices are device pointers (as HJ_UPDATE_DEVICE_ARRAYS), used in place on the
 *     context's stream.  HJ_MOTION_DEVICE_OUT: motion is a device pointer, 16-byte aligned, written in place.
 * The context keeps the staging of previous shape arrays that come from the host - 48 / 16 / 32 bytes per quad / sphere / vertex -
 *   and 16 bytes a pixel when motion is a host array.  No second width x height buffer exists: the walk writes each pixel's raw hit
 *   into its record and the resolve overwrites it in place.
 * HJ_ERR_INVALID, before the device is touched, in this order, each with its text in hj_last_error behind "hj_render_motion:":
 *   null prev or motion; unknown flag bits; a zero width or height, or one above 16384; a prev->camera field that is not finite, or
 *   a fov outside (0, 180); a misaligned device array.  A refused call writes nothing.  Then hj_trace_rays' gate: HJ_ERR_STATE without
 *   a scene, with a frame in flight, or with undrained frames.  Behind the gate, in this order: counts that differ from the uploaded
 *   scene's (HJ_ERR_INVALID); with host arrays, a previous coordinate or radius that is not finite (HJ_ERR_INVALID) - device arrays
 *   are the caller's word, as for hj_scene_update_shapes.
 * Not here: rotation of a sphere about its own centre, which a record of centre and radius cannot express; what a mirror or glass
 *   shows (hj_render_motion_followed below follows it); moving lights' shadows on static surfaces; a change of topology or counts; a multi-GPU split; a CLI flag. */
#define HJ_MOTION_WORDS 4
#define HJ_MOTION_NONE 0xFFFFFFFFu
#define HJ_MOTION_DEVICE_SHAPES 1u   /* prev->spheres / quads / vertices are device pointers (as HJ_UPDATE_DEVICE_ARRAYS) */
#define HJ_MOTION_DEVICE_OUT    2u   /* motion is a device pointer, 16-byte aligned, written in place */
int hj_render_motion(hj_context* ctx, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t flags,
                     float* motion /* height x width x 4 */);

/* hj_render_motion_followed (ABI 0.31): hj_render_motion through mirrors and glass - the motion image that composes with the followed
 * AOVs' guides.  A followed guide's depth on a specular pixel is the depth of what the surface SHOWS (the sum of the chain's t), and
 * hj_denoise_frame_temporal_motion tests the history's depth against the record's zp: hj_render_motion's zp is the distance to the
 * mirror itself, so with followed guides every tap on a mirror fails and the pixel restarts every frame.  This call follows the chain
 * the followed AOVs follow, for the pixel's centre ray, and gives the previous position of the VIRTUAL point the guide describes.
 * No counterpart in the reference; tests/motion_follow_ref.py restates the contract in numpy.
 *   Arguments, flags, the record layout, the staging and the device forms are hj_render_motion's, with max_follow in 0 ...
 *   HJ_AOV_MAX_FOLLOW in front of flags.  Every operation is float32 with one rounding and no contraction, except where hj_render_motion
 *   excepts it, inside the specular continuation (Followed AOVs above: its own fixed expressions) and the hit points' fma.
 *   THE CHAIN starts as hj_render_motion's RAY and is continued at each hit by the specular continuation of hj_follow_specular (a
 *     mirror reflects; a dielectric reflects when k <= 0 or fr >= 0.5f, else refracts): origin p, direction wo, tMin = eps, tMax =
 *     +inf.  It ends after max_follow continuations, at a hit that is neither mirror nor dielectric, or at a continuation that hits
 *     nothing: hj_render_aovs_followed's chain for a sample through the pixel's centre.
 *   NO CONTINUATION TAKEN - max_follow == 0, a first hit that is not specular, a miss: the record is hj_render_motion's, bit for bit,
 *     by its own arithmetic.  max_follow == 0 is hj_render_motion through the same two launches and nothing else.
 *   AT LEAST ONE CONTINUATION TAKEN, and a last hit (id, t, u, v) on the segment (o, d):
 *     D = the float32 sum of the chain's t values in chain order, (t0 + t1) + t2 ...: the followed AOVs' depth word.
 *     d0 = the RAY's d.  Pv = camera.position + D * d0 per channel (one multiply, one add): the virtual point, where step 2 of
 *       hj_denoise_frame_temporal would put a guide of depth D.
 *     X_now and X_prev: the hit point re-expressed on the uploaded and on the previous shape by ONE expression, so that an unmoved
 *       shape gives X_prev - X_now == 0 exactly.  sphere: P = fma(t, d, o); n = (P - c) * (1.0f / r) with (c, r) the uploaded sphere;
 *       X = c* + n * r* with (c*, r*) the uploaded, then the previous sphere.  quad: X = (o* + e1* * u) + e2* * v.  triangle:
 *       l0 = (1.0f - u) - v; X = (a* * l0 + b* * u) + c* * v with the uploaded index triple.
 *     delta = X_prev - X_now.
 *     M = the product of the Householder matrices of the chain's REFLECT events in chain order, M_k = M_(k-1) H_k, starting as the
 *       identity; a refraction leaves M as it is.  A reflect event with shading normal n (the populated normal, not turned towards
 *       the ray) takes M to M - 2 (M n) n^T in this order: w_i = (M_i0 * n.x + M_i1 * n.y) + M_i2 * n.z;  w2_i = 2.0f * w_i;
 *       M_ij = M_ij - w2_i * n_j.
 *     Pv_prev_i = Pv_i + ((M_i0 * delta.x + M_i1 * delta.y) + M_i2 * delta.z).
 *     The record is hj_render_motion's PROJECTION of Pv_prev in Pp's place: (sx, sy, zp = |Pv_prev - prev.position|, id as bits), or
 *       (0, 0, 0, HJ_MOTION_NONE) where c.z < 0 is false.
 *   A CHAIN WHOSE LAST CONTINUATION HITS NOTHING: D = the sum so far and Pv_prev = Pv itself (no delta is added); the record is
 *     its PROJECTION with word 3 = HJ_MOTION_LEFT - the followed guide keeps the record of the surface that was left at that depth.
 *     HJ_MOTION_LEFT is not HJ_MOTION_NONE: hj_denoise_frame_temporal_motion reads the record as a position.
 *   A record depends on the uploaded scene, prev, (width, height) and max_follow alone, as hj_render_motion's.
 * The context keeps, beside hj_render_motion's staging, 84 bytes a pixel of the whole image while max_follow > 0: the chain state
 *   (32), M (48), the list of live pixels (4), and a count per 256 pixels.  An image that does not fit is HJ_ERR_NOMEM; the image is
 *   not banded.  The stream is synchronised once a round, for the count of live chains.
 * HJ_ERR_INVALID, before the device is touched: hj_render_motion's refusals in their order with their texts behind
 *   "hj_render_motion_followed:", then max_follow above HJ_AOV_MAX_FOLLOW.  Then hj_trace_rays' gate, and behind it hj_render_motion's
 *   two checks.
 * Not here: on a planar static mirror the record is exact (tests/test_motion_follow_host.py judges it in float64); a curved mirror
 *   is treated by its tangent plane at the hit; a refraction carries the displacement through unchanged; a specular surface that
 *   itself moved is not accounted for; an environment seen after a mirror is treated as static; the chain is the centre ray's, not a
 *   mean over a pixel's samples; what hj_render_motion leaves out. */
#define HJ_MOTION_LEFT 0xFFFFFFFEu
int hj_render_motion_followed(hj_context* ctx, const hj_scene_desc* prev, uint32_t width, uint32_t height, uint32_t max_follow,
                              uint32_t flags, float* motion /* height x width x 4 */);

/* hj_denoise_frame_temporal_motion (ABI 0.29): hj_denoise_frame_temporal reprojecting through a motion image.
 *   motion == NULL: the call is hj_denoise_frame_temporal, bit for bit (one host routine).
 *   Otherwise step 2 (REPROJECT) changes for a guided pixel: if word 3 of the pixel's motion record is HJ_MOTION_NONE there is no
 *     history; otherwise sx, sy and zp are words 0, 1 and 2 of the record, and everything from fx = sx - 0.5f on is step 2
 *     unchanged - the window test, the four taps, their order, and the depth and normal tests against zp and the pixel's own n.
 *     The two cameras of topts are still validated but not used.
 *   HJ_DENOISE_DEVICE_ARRAYS covers motion too; motion joins the alias check against history_out and the alignment check.  The
 *   context keeps the staging of a host-side motion image, 16 bytes a pixel.  Every refusal is hj_denoise_frame_temporal's, behind
 *   "hj_denoise_frame_temporal_motion:".
 *   So a motion image holding the static projection's own (sx, sy, zp) - and HJ_MOTION_NONE where c.z < 0 is false - gives
 *   hj_denoise_frame_temporal's results bit for bit, and an image of HJ_MOTION_NONE alone gives hj_denoise_frame's out.
 * Not here: what hj_render_motion does not follow (its list). */
int hj_denoise_frame_temporal_motion(hj_context* ctx, uint32_t width, uint32_t height, const float* beauty, const float* aov,
                                     const hj_denoise_opts* opts, const hj_temporal_opts* topts,
                                     const float* motion /* H x W x HJ_MOTION_WORDS, or NULL */,
                                     const float* history_in, float* history_out, float* out);

/* The deterministic replacement of `rand::random()` in the block generator.
 * Pure functions (no context); the same definitions are used by the host
 * library's ImageBlockGenerator and restated by the oracle. */
uint32_t hj_block_seed(uint64_t master_seed, uint32_t pass, uint32_t block_in_pass);
void hj_pass_offset(uint64_t master_seed, uint32_t offset_index, float out_xy[2]);
/* Rank that renders block j (raster index inside a pass) of pass `pass` of a width x height frame:
 * (column + row + pass) mod world.  With HJ_RENDER_STATIC_DEAL hj_render_frame uses pass = 0 for every pass. */
uint32_t hj_block_owner(uint32_t width, uint32_t height, uint32_t pass, uint32_t block_in_pass, uint32_t world);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HIJIKI_HIP_H */
