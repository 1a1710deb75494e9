"""ctypes loader for the CPU oracle (oracle/hj_oracle.c).

TEST INFRASTRUCTURE ONLY — imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg; never by the product package.
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libhj_oracle.so")
_LIB = None


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("paths", "closest_calls", "shadow_calls", "nodes", "tri_tests",
                                           "sphere_tests", "quad_tests", "hits", "nee_evals", "shadow_nodes",
                                           "shadow_tri_tests", "shadow_sphere_tests", "shadow_quad_tests",
                                           "shadow_hits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def build():
    subprocess.check_call(["make", "-s", "oracle"], cwd=os.path.dirname(_HERE))


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            build()
        from hijiki_amd import abi
        L = C.CDLL(LIB_PATH)
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        L.hjo_render_blocks.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.ImageBlock), C.c_size_t,
                                        C.POINTER(abi.RenderOpts), C.c_uint32, C.c_uint32, fp, C.c_int,
                                        C.POINTER(Counters), C.POINTER(C.c_double)]
        L.hjo_block_seed.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.hjo_block_seed.restype = C.c_uint32
        L.hjo_pass_offset.argtypes = [C.c_uint64, C.c_uint32, fp]
        L.hjo_pass_offset.restype = None
        L.hjo_make_blocks.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.POINTER(abi.ImageBlock), C.c_size_t]
        L.hjo_make_blocks.restype = C.c_size_t
        L.hjo_rng_seed.argtypes = [C.c_uint32]
        L.hjo_rng_seed.restype = C.c_uint32
        L.hjo_rng_next.argtypes = [u32p]
        L.hjo_rng_next.restype = C.c_uint32
        L.hjo_rng_float.argtypes = [u32p]
        L.hjo_rng_float.restype = C.c_float
        L.hjo_exp.argtypes = [C.c_float]
        L.hjo_exp.restype = C.c_float
        L.hjo_sincos2pi.argtypes = [C.c_float, fp]
        L.hjo_sincos2pi.restype = None
        L.hjo_atan2.argtypes = [C.c_float, C.c_float]
        L.hjo_atan2.restype = C.c_float
        L.hjo_asin.argtypes = [C.c_float]
        L.hjo_asin.restype = C.c_float
        for name in ("hjo_cos_hemisphere", "hjo_barycentric", "hjo_uniform_sphere"):
            getattr(L, name).argtypes = [u32p, fp]
            getattr(L, name).restype = None
        L.hjo_intersect.argtypes = [C.POINTER(abi.SceneDesc), C.c_int, fp, C.c_size_t, fp, fp]
        L.hjo_camera_rays.argtypes = [C.POINTER(abi.Camera), C.c_uint32, C.c_uint32, fp, C.c_size_t, fp]
        L.hjo_camera_rays.restype = None
        L.hjo_integrate_block.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.ImageBlock),
                                          C.POINTER(abi.RenderOpts), fp, C.POINTER(Counters)]
        L.hjo_reconstruct_block.argtypes = [C.POINTER(abi.ImageBlock), C.POINTER(abi.RenderOpts), fp, fp, C.c_uint32,
                                            C.c_uint32]
        L.hjo_recon_gauss.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.hjo_recon_gauss.restype = C.c_float
        L.hjo_dielectric_probe.argtypes = [C.c_float, fp, fp, u32p, fp]
        L.hjo_dielectric_probe.restype = None
        L.hjo_shade_probe.argtypes = [C.POINTER(abi.SceneDesc), fp, u32p, C.c_size_t, fp]
        L.hjo_set_directional_bvh.argtypes = [C.c_int, C.c_void_p]
        L.hjo_set_directional_bvh.restype = None
        L.hjo_set_textures.argtypes = [C.POINTER(abi.TextureSet)]
        L.hjo_set_textures.restype = None
        L.hjo_texture_lookup.argtypes = [C.POINTER(abi.TextureSet), C.c_uint32, fp, C.c_size_t, fp]
        L.hjo_set_environment.argtypes = [C.POINTER(abi.Environment), fp, C.c_size_t]
        L.hjo_set_environment.restype = None
        L.hjo_env_lookup.argtypes = [fp, C.c_size_t, fp]
        L.hjo_env_sample.argtypes = [u32p, C.c_size_t, fp]
        L.hjo_num_batch.argtypes = [C.c_uint32, u32p, C.c_size_t, u32p]
        L.hjo_shade_step.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RenderOpts), u32p, C.c_size_t, u32p]
        L.hjo_sizeof_counters.restype = C.c_size_t
        assert L.hjo_sizeof_counters() == C.sizeof(Counters)
        _LIB = L
    return _LIB


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@contextlib.contextmanager
def textures(compiled, texture_set=None):
    """The image textures of `compiled` (its texture_set, as device.Renderer.upload_scene takes them) - or `texture_set`, an
    abi.TextureSet that overrides them - for the oracle calls inside the block (hjo_set_textures); none after it."""
    t = texture_set
    if t is None and hasattr(compiled, "texture_set"):
        t = compiled.texture_set
        t = t if t.num_textures else None
    L = lib()
    L.hjo_set_textures(C.byref(t) if t is not None else None)
    try:
        yield
    finally:
        L.hjo_set_textures(None)


def env_table(texture_set, env):
    """The alias table hjo_set_environment takes, from hj_debug_env_distribution (host code, no GPU): (W * H, 4) float32 records
    (threshold, alias cell as uint32 bits, pdf of the cell, pdf of the alias cell).  None when the distribution is refused - the
    oracle then refuses the environment itself."""
    from hijiki_amd import abi, device
    try:
        d = device.env_distribution(texture_set, env)
    except (abi.HijikiError, IndexError, ValueError):
        return None
    alias = d["alias"].ravel()
    pdf = d["pdf"].ravel()
    rec = np.zeros((alias.size, 4), np.float32)
    rec[:, 0] = d["alias_prob"].ravel()
    rec[:, 1] = alias.view(np.float32)
    rec[:, 2] = pdf
    rec[:, 3] = pdf[alias]
    return rec


@contextlib.contextmanager
def environment(compiled, env=None, table=None):
    """The environment of `compiled` (its `environment`, as device.Renderer.upload_scene takes it) - or `env`, an abi.Environment
    that overrides it - and its sampling distribution (`table`, default env_table of the scene's texture set) for the oracle calls
    inside the block (hjo_set_environment); none after it.  Use inside `textures(...)`: the environment is one of its textures."""
    if env is None:
        env = getattr(compiled, "environment", None)
    L = lib()
    if env is not None and table is None:
        t = getattr(compiled, "texture_set", None)
        if t is not None and env.texture < t.num_textures:
            table = env_table(t, env)
    if table is not None:
        table = np.ascontiguousarray(table, np.float32).reshape(-1, 4)
    L.hjo_set_environment(C.byref(env) if env is not None else None, _fp(table) if table is not None else None,
                          len(table) if table is not None else 0)
    try:
        yield
    finally:
        L.hjo_set_environment(None, None, 0)


@contextlib.contextmanager
def scene_inputs(compiled, texture_set=None, env=None, table=None):
    """textures(...) and environment(...) of one compiled scene."""
    with textures(compiled, texture_set), environment(compiled, env, table):
        yield


def _status(name, rc):
    """A refusal as abi.HijikiError (a RuntimeError) carrying the status."""
    if rc != 0:
        from hijiki_amd import abi
        raise abi.HijikiError(rc, f"{name} failed")


def render_blocks(compiled, blocks, width, height, opts=None, nthreads=None, accum=None):
    """Render `blocks` (ctypes array of ImageBlock) in order, with the compiled scene's image textures and environment if it has
    any.  Returns (accum[H,W,4], counters dict, seconds)."""
    from hijiki_amd import abi
    L = lib()
    opts = opts or abi.RenderOpts.default()
    nthreads = nthreads or os.cpu_count() or 1
    if accum is None:
        accum = np.zeros((height, width, 4), np.float32)
    ctr, secs = Counters(), C.c_double(0)
    with scene_inputs(compiled):
        rc = L.hjo_render_blocks(C.byref(compiled.desc), blocks, len(blocks), C.byref(opts), width, height, _fp(accum),
                                 nthreads, C.byref(ctr), C.byref(secs))
    _status("hjo_render_blocks", rc)
    return accum, ctr.as_dict(), secs.value


def make_blocks(width, height, spp, master_seed, pass_begin=0, pass_end=None, block_size=128):
    from hijiki_amd import abi
    L = lib()
    pass_end = spp if pass_end is None else pass_end
    n = L.hjo_make_blocks(width, height, block_size, master_seed, pass_begin, pass_end, None, 0)
    arr = (abi.ImageBlock * n)()
    L.hjo_make_blocks(width, height, block_size, master_seed, pass_begin, pass_end, arr, n)
    return arr


def resolve(accum):
    """rgb / w (src/main.rs:1399)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return accum[..., :3] / accum[..., 3:4]


def intersect(compiled, rays, use_bvh=True, full=False):
    """rays (n,8) f32 -> ids (n,) int32, t,u,v (n,) [, full (n,16)]."""
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    hits = np.zeros((n, 4), np.float32)
    fullbuf = np.zeros((n, 16), np.float32) if full else None
    lib().hjo_intersect(C.byref(compiled.desc), int(use_bvh), _fp(rays), n, _fp(hits),
                        _fp(fullbuf) if full else None)
    ids = hits[:, 0].copy().view(np.int32)
    return (ids, hits[:, 1], hits[:, 2], hits[:, 3]) + ((fullbuf,) if full else ())


def shade_probe(compiled, rays, rng_states):
    """One shading step per ray (hjo_shade_probe): returns the (n, 20) float32 record array, ids (int32), RNG after (uint32)."""
    rays = np.ascontiguousarray(rays, np.float32)
    rng = np.ascontiguousarray(rng_states, np.uint32)
    out = np.zeros((len(rays), 20), np.float32)
    with scene_inputs(compiled):
        _status("hjo_shade_probe", lib().hjo_shade_probe(C.byref(compiled.desc), _fp(rays), rng.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                         len(rays), _fp(out)))
    return out, out[:, 0].copy().view(np.int32), out[:, 15].copy().view(np.uint32)


def num_batch(op, words):
    """hjo_num_batch, the twin of hj_debug_num (device.Renderer.num_probe: same arguments, same (n, 4) uint32 result) over the
    oracle's own primitives."""
    from hijiki_amd import abi
    w = np.asarray(words, np.uint32)
    w = w.reshape(len(w), -1)
    rec = np.zeros((len(w), abi.NUM_IN_WORDS), np.uint32)
    rec[:, :w.shape[1]] = w
    out = np.zeros((len(w), abi.NUM_OUT_WORDS), np.uint32)
    up = C.POINTER(C.c_uint32)
    _status("hjo_num_batch", lib().hjo_num_batch(abi.NUM_OPS.index(op) if isinstance(op, str) else int(op), rec.ctypes.data_as(up),
                                                 len(rec), out.ctypes.data_as(up)))
    return out


def shade_step(compiled, records, opts=None):
    """hjo_shade_step, the twin of hj_debug_shade_step (device.Renderer.shade_step: same (n, 18) uint32 records, same (n, 33) uint32
    result) over the step function integrate_ray itself calls.  Next-event samples always come back as shadow records: the oracle
    has no light-shaft grid."""
    from hijiki_amd import abi
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, abi.STEP_IN_WORDS)
    out = np.zeros((len(rec), abi.STEP_OUT_WORDS), np.uint32)
    opts = opts or abi.RenderOpts.default()
    up = C.POINTER(C.c_uint32)
    with scene_inputs(compiled):
        _status("hjo_shade_step", lib().hjo_shade_step(C.byref(compiled.desc), C.byref(opts), rec.ctypes.data_as(up), len(rec),
                                                       out.ctypes.data_as(up)))
    return out


def texture_lookup(texture_set, texture, uv):
    """hjo_texture_lookup: the colour texture `texture` of `texture_set` (abi.TextureSet) gives a HJ_MAT_DIFFUSE_TEXTURED hit at
    (n, 2) float32 uv -> (n, 3) float32."""
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((len(uv), 3), np.float32)
    _status("hjo_texture_lookup", lib().hjo_texture_lookup(C.byref(texture_set), int(texture), _fp(uv), len(uv), _fp(out)))
    return out


def env_lookup(compiled, dirs, env=None, table=None):
    """hjo_env_lookup: the radiance the environment of `compiled` sends along (n, 3) directions -> (n, 3) float32."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = np.zeros((len(d), 3), np.float32)
    with scene_inputs(compiled, env=env, table=table):
        _status("hjo_env_lookup", lib().hjo_env_lookup(_fp(d), len(d), _fp(out)))
    return out


def env_sample(compiled, rng_states, env=None, table=None):
    """hjo_env_sample: n uint32 RNG states -> (n, 8) float32: direction xyz, pdf, texel index, Le / pdf rgb (the layout of
    hj_debug_env_sample)."""
    s = np.ascontiguousarray(rng_states, np.uint32).reshape(-1)
    out = np.zeros((len(s), 8), np.float32)
    with scene_inputs(compiled, env=env, table=table):
        _status("hjo_env_sample", lib().hjo_env_sample(s.ctypes.data_as(C.POINTER(C.c_uint32)), len(s), _fp(out)))
    return out


def camera_rays(camera, width, height, pix_xy):
    pix_xy = np.ascontiguousarray(pix_xy, np.float32).reshape(-1, 2)
    out = np.zeros((len(pix_xy), 6), np.float32)
    lib().hjo_camera_rays(C.byref(camera), width, height, _fp(pix_xy), len(pix_xy), _fp(out))
    return out


def integrate_block(compiled, block, opts=None):
    """Per-path samples of one block: (dim_y, dim_x, 8) = (rgb, w, normal, depth); counters."""
    from hijiki_amd import abi
    opts = opts or abi.RenderOpts.default()
    out = np.zeros((block.dimension[1], block.dimension[0], 8), np.float32)
    ctr = Counters()
    with scene_inputs(compiled):
        _status("hjo_integrate_block", lib().hjo_integrate_block(C.byref(compiled.desc), C.byref(block), C.byref(opts), _fp(out),
                                                                 C.byref(ctr)))
    return out, ctr.as_dict()


def logged_rays(compiled, blocks, opts=None):
    """Every ray the oracle traces for `blocks` (hjo_set_ray_log around hjo_integrate_block, single-threaded): (n, 11) float32 =
    o, d, tMin, tMax, kind (0 closest-hit, 1 shadow), id of the shape hit or -1, index of the emitter a shadow ray aims at (8: the
    environment; else -1).  Directions are whatever the reference's
    arithmetic made them - not always unit vectors."""
    import tempfile
    L = lib()
    L.hjo_set_ray_log.argtypes = [C.c_char_p]
    L.hjo_set_ray_log.restype = None
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rays.bin")
        L.hjo_set_ray_log(path.encode())
        try:
            for b in blocks:
                integrate_block(compiled, b, opts)
        finally:
            L.hjo_set_ray_log(None)
        return np.fromfile(path, np.float32).reshape(-1, 11)


def reconstruct_block(block, samples, accum, opts=None):
    from hijiki_amd import abi
    opts = opts or abi.RenderOpts.default()
    samples = np.ascontiguousarray(samples, np.float32)
    h, w = accum.shape[:2]
    lib().hjo_reconstruct_block(C.byref(block), C.byref(opts), _fp(samples), _fp(accum), w, h)
    return accum
