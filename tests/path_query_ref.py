"""The reference of hj_trace_paths, from the oracle alone, and the ray sets its tests share.

compose() is the loop of test_shade_step_gpu.chain - oracle.shade_step for a bounce, oracle.intersect for the rays between the steps
and for the shadow rays - with the caller's rays and seeds as the first records instead of a block's camera rays.
test_path_query_host.py proves that on a block's camera rays and seeds it equals hjo_integrate_block word for word."""
import functools

import numpy as np

import env_scenes
import scenes
import texture_scenes
from hijiki_amd import abi, host
from test_num_gpu import words
from test_shade_step_gpu import IN, KEPS, records

U, F = np.uint32, np.float32
END_MISS, END_EMISSIVE, END_ROULETTE, END_CAP, END_OTHER = range(5)


def rng_states(seeds):
    """rng_seed of (n,) uint32 seeds, by the oracle's own hash"""
    from oracle import hj_oracle as oracle
    return oracle.num_batch("rng_seed", np.asarray(seeds, U).reshape(-1, 1))[:, 0].copy()


def compose(cs, rays, spp=1, opts=None, detail=False):
    """rays (n, 8): origin, direction, seed bits, reserved.  The scene's textures and environment are the compiled scene's (the
    oracle's shade_step installs them).  -> (samples (n, 8) float32 in hj_debug_samples' layout: the float32 sum over k = 0, 1, ... of
    sample k's radiance starting from +0, (float)spp, first-hit normal and t; counts: closest_rays, hits, shadow_rays,
    unoccluded_shadow_rays, paths) [, detail: per sample k (list) how the path ended (END_*) and the first hit's shape id]."""
    from oracle import hj_oracle as oracle
    o = opts if opts is not None else abi.RenderOpts.default()
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n = len(rays)
    ns, nq, nt = int(cs.desc.num_spheres), int(cs.desc.num_quads), int(cs.desc.num_triangles)
    tags = cs.materials >> abi.MATERIAL_TAG_SHIFT if ns + nq + nt else np.zeros(0, U)
    seeds = rays[:, 6].copy().view(U)
    counts = dict(closest_rays=0, hits=0, shadow_rays=0, unoccluded_shadow_rays=0, paths=n * spp)
    rgb = np.zeros((n, 3), F)
    nd = np.zeros((n, 4), F)
    ends, first_ids = [], []
    for k in range(spp):
        rec = records(rays[:, 0:3], rays[:, 3:6], 0.0, np.zeros(n, np.int32), 0.0, 0.0, rng=rng_states(seeds + U(k)), bounce=0, discrete=1)
        tmin = np.full(n, KEPS, F)
        total = np.zeros((n, 3), F)
        nd_k = np.zeros((n, 4), F)
        end = np.full(n, END_OTHER, np.int8)
        first_id = np.full(n, -1, np.int32)
        live = np.arange(n)
        while len(live):
            r8 = np.concatenate([rec[:, 0:6].view(F), tmin[:, None], np.full((len(rec), 1), np.inf, F)], 1)
            ids, t, u, v = oracle.intersect(cs, r8)
            counts["closest_rays"] += len(rec)
            counts["hits"] += int((ids >= 0).sum())
            rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9] = words(t), ids.view(U), words(u), words(v)
            out = oracle.shade_step(cs, rec, o)
            total[live] = total[live] + out[:, 26:29].view(F)                             # (+0 where the step added nothing)
            bounce = rec[:, 17] >> 1
            first = bounce == 0
            nd_k[live[first]] = out[first, 29:33].view(F)
            first_id[live[first]] = ids[first]
            sh = out[:, 15] == 1
            if sh.any():
                srays = np.concatenate([out[sh, 16:22].view(F), np.full((int(sh.sum()), 1), F(2) * KEPS, F), out[sh, 22:23].view(F)], 1)
                occ = oracle.intersect(cs, srays)[0] >= 0
                counts["shadow_rays"] += int(sh.sum())
                counts["unoccluded_shadow_rays"] += int((~occ).sum())
                idx = live[sh][~occ]
                total[idx] = total[idx] + out[sh][~occ][:, 23:26].view(F)
            go = out[:, 0] == 1
            tag = np.where(ids >= 0, tags[np.maximum(ids, 0)], 99)
            why = np.where(ids < 0, END_MISS, np.where(tag == abi.MAT_EMISSIVE, END_EMISSIVE,
                           np.where(bounce + 1 >= o.max_bounces, END_CAP, np.where(bounce >= o.rr_start, END_ROULETTE, END_OTHER))))
            end[live[~go]] = why[~go]
            nxt = np.zeros((int(go.sum()), IN), U)
            nxt[:, 0:3], nxt[:, 3:6], nxt[:, 10:13], nxt[:, 13:16] = out[go, 1:4], out[go, 4:7], out[go, 7:10], out[go, 12:15]
            nxt[:, 16], nxt[:, 17] = out[go, 11], out[go, 10]
            rec, live, tmin = nxt, live[go], np.full(int(go.sum()), F(2) * KEPS, F)
        rgb = rgb + total                                                                 # float32, in the order of k, from +0
        if k == 0:
            nd = nd_k
        ends.append(end)
        first_ids.append(first_id)
    samples = np.concatenate([rgb, np.full((n, 1), F(spp), F), nd], 1)
    return (samples, counts, dict(end=ends, first_id=first_ids)) if detail else (samples, counts)


# ------------------------------------------------------------------------------------------------------------------ ray sets

def _textured():
    return texture_scenes.textured_cbox(seed=2, filt=abi.TEX_BILINEAR)[0].compile()


SCENES = {"cbox": lambda: host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile(), "rich": lambda: scenes.rich_scene(7),
          "env": lambda: env_scenes.mixed_scene(tinted=True), "textured": _textured}
N_RAYS = 3001
# the generator's seed per scene: the first of 1, 2, ... at which the set holds what test_path_query_host.py asserts of it
GEN_SEED = {"cbox": 1, "rich": 1, "env": 1, "textured": 1}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def domain(cs):
    """the origin domain: the root box joined with the camera"""
    b = cs.bvh_f32
    cam = np.array(cs.desc.camera.position[:3], F)
    return np.minimum(b[0, 0:3], cam), np.maximum(b[0, 4:7], cam)


def shape_points(cs, ids, rng):
    """a point of each shape of `ids`: inside a sphere's silhouette disc, inside a quad or triangle"""
    ns, nq = len(cs.spheres), len(cs.quads)
    out = np.zeros((len(ids), 3))
    for j, i in enumerate(ids):
        if i < ns:
            out[j] = cs.spheres[i, 0:3] + rng.uniform(-0.5, 0.5, 3) * cs.spheres[i, 3]
        elif i < ns + nq:
            q = cs.quads[i - ns]
            out[j] = q[0:3] + rng.uniform(0.05, 0.95) * q[4:7] + rng.uniform(0.05, 0.95) * q[8:11]
        else:
            a, b, c = cs.vertices[cs.triangles[i - ns - nq], 0:3].astype(np.float64)
            w = rng.dirichlet([1, 1, 1])
            out[j] = w[0] * a + w[1] * b + w[2] * c
    return out


@functools.lru_cache(maxsize=None)
def ray_set(name):
    """N_RAYS rays of scene `name`, every origin inside the domain:
      [0, 2601)     origins uniform in the domain; every second direction uniform on the sphere, the others aimed at a point of a
                    shape drawn by material tag (so that every tag the scene has gets first hits, small shapes too)
      [2601, 2801)  origins ON surfaces: hit points of the first 200 rays that hit, directions uniform
      [2801, 3001)  rays that leave the scene: from a point of the root box's faces, outwards
    unit directions, except rays [300, 600): lengths in [0.5, 2]; seeds random uint32, rays 0, 1, 2: 0, 0xFFFFFFFE, 0xFFFFFFFF."""
    from oracle import hj_oracle as oracle
    cs = scene(name)
    rng = np.random.default_rng([GEN_SEED[name], list(SCENES).index(name)])
    lo, hi = domain(cs)
    n_in, n_surf, n_out = N_RAYS - 400, 200, 200
    o = rng.uniform(lo, hi, (n_in, 3))
    d = rng.normal(size=(n_in, 3))
    tags = cs.materials >> abi.MATERIAL_TAG_SHIFT
    present = sorted(set(tags.tolist()))
    aimed = np.arange(1, n_in, 2)
    pick = np.array([rng.choice(np.flatnonzero(tags == present[j % len(present)])) for j in range(len(aimed))])
    d[aimed] = shape_points(cs, pick, rng) - o[aimed]
    rays = np.zeros((N_RAYS, 8), F)
    rays[:n_in, 0:3], rays[:n_in, 3:6] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    probe = rays[:n_in].copy()
    probe[:, 6], probe[:, 7] = KEPS, np.inf
    ids, t, _, _ = oracle.intersect(cs, probe)
    hit = np.flatnonzero((ids >= 0) & np.isfinite(t))[:n_surf]
    assert len(hit) == n_surf
    p = (probe[hit, 0:3] + t[hit, None] * probe[hit, 3:6]).astype(F)
    rays[n_in:n_in + n_surf, 0:3] = np.clip(p, lo, hi)
    ds = rng.normal(size=(n_surf, 3))
    rays[n_in:n_in + n_surf, 3:6] = ds / np.linalg.norm(ds, axis=1, keepdims=True)
    blo, bhi = cs.bvh_f32[0, 0:3], cs.bvh_f32[0, 4:7]
    po = rng.uniform(blo, bhi, (n_out, 3))
    do = rng.normal(size=(n_out, 3))
    axis, side = rng.integers(0, 3, n_out), rng.integers(0, 2, n_out)
    rows = np.arange(n_out)
    po[rows, axis] = np.where(side == 1, bhi[axis], blo[axis])
    do[rows, axis] = np.where(side == 1, 1.0, -1.0) * (1.0 + np.abs(do[rows, axis]))
    rays[n_in + n_surf:, 0:3], rays[n_in + n_surf:, 3:6] = po, do / np.linalg.norm(do, axis=1, keepdims=True)
    rays[300:600, 3:6] *= rng.uniform(0.5, 2.0, (300, 1)).astype(F)
    seeds = rng.integers(0, 1 << 32, N_RAYS, dtype=np.uint64).astype(U)
    seeds[0:3] = [0, 0xFFFFFFFE, 0xFFFFFFFF]
    rays.view(U)[:, 6] = seeds
    assert ((rays[:, 0:3] >= lo) & (rays[:, 0:3] <= hi)).all()
    rays.setflags(write=False)
    return rays


def options(max_bounces=40, grid=True):
    o = abi.RenderOpts.default()
    o.max_bounces = max_bounces
    if not grid:
        o.flags |= abi.RENDER_NO_LIGHT_GRID
    return o


@functools.lru_cache(maxsize=None)
def expected(name, max_bounces=40):
    """compose() of the scene's ray set with its detail: computed once, never written to"""
    samples, counts, detail = compose(scene(name), ray_set(name), 1, options(max_bounces), detail=True)
    samples.setflags(write=False)
    return samples, counts, detail


def camera_block():
    """the 32 x 32 block of the premise test"""
    block = abi.ImageBlock()
    block.dimension[:] = (32, 32)
    block.original_dimension[:] = (32, 32)
    block.origin[:] = (0, 0)
    block.sample_offset[:] = (0.25, 0.75)
    block.seed = 4242
    return block


def camera_rays(cs, block):
    """the block's camera rays (oracle.camera_rays) with seed = block.seed + lx + ly * dimension.x, row by row"""
    from oracle import hj_oracle as oracle
    W, H = int(block.dimension[0]), int(block.dimension[1])
    ly, lx = np.mgrid[0:H, 0:W]
    px = np.stack([lx.ravel() + block.origin[0] + block.sample_offset[0], ly.ravel() + block.origin[1] + block.sample_offset[1]], 1).astype(F)
    cam = oracle.camera_rays(cs.desc.camera, int(block.original_dimension[0]), int(block.original_dimension[1]), px)
    rays = np.zeros((W * H, 8), F)
    rays[:, 0:6] = cam[:, 0:6]
    rays.view(U)[:, 6] = ((block.seed + lx.ravel() + ly.ravel() * W) & 0xFFFFFFFF).astype(U)
    return rays
