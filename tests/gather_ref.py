"""The reference of hj_trace_irradiance, from the oracle alone, and the point sets its tests share.

directions(): rng_seed, rand_cos_hemisphere / rand_uniform_sphere, cross3 and normalize3 are oracle.num_batch's; the products and sums
of the frame are plain numpy float32 in the header's order.  trace() is the loop of path_query_ref.compose, generalised to take
initial RNG STATES (not seeds) and to return every path's radiance and first-hit record; test_gather_host.py proves that with the
states rng_seed(seeds + k) and the caller's directions it equals compose word for word.  gather() adds the sums, the hit count, the
minimum and the SH sums in numpy float32, in the stated order."""
import functools

import numpy as np

import path_query_ref as R
from hijiki_amd import abi
from test_num_gpu import words
from test_shade_step_gpu import IN, KEPS, records

U, F = np.uint32, np.float32
COUNTS = ("paths", "closest_rays", "shadow_rays", "hits", "unoccluded_shadow_rays")
# the header's five constants: 1 / (2 sqrt(pi)), sqrt(3 / (4 pi)), sqrt(15 / (4 pi)), sqrt(5 / (16 pi)), sqrt(15 / (16 pi)) in float32
C0, C1, C2, C3, C4 = (F(float.fromhex(h)) for h in ("0x1.20dd76p-2", "0x1.f45438p-2", "0x1.17b142p+0", "0x1.42f602p-2", "0x1.17b142p-1"))


def _num(op, w):
    from oracle import hj_oracle as oracle
    return oracle.num_batch(op, np.ascontiguousarray(w, U))


def _vec(op, p, q=None):
    w = words(p) if q is None else np.concatenate([words(p), words(q)], 1)
    return _num(op, w)[:, 0:3].copy().view(F)


def directions(points, spp, sphere):
    """points (n, 8) -> (d (n, spp, 3) float32: the direction of sample k of point i as the header defines it; states (n, spp)
    uint32: the RNG state behind its two draws)"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 8)
    n = len(pts)
    seeds = pts[:, 6].copy().view(U)
    d, states = np.zeros((n, spp, 3), F), np.zeros((n, spp), U)
    if not sphere:
        nm = pts[:, 3:6]
        bt = np.where((np.abs(nm[:, 0]) > np.abs(nm[:, 1]))[:, None], F([0, 1, 0]), F([1, 0, 0])).astype(F)
        t = _vec("normalize3", _vec("cross3", nm, bt))
        b = _vec("cross3", nm, t)
    for k in range(spp):
        s = _num("rng_seed", (seeds + U(k)).reshape(-1, 1))[:, 0]
        out = _num("rand_uniform_sphere" if sphere else "rand_cos_hemisphere", s.reshape(-1, 1))
        l = out[:, 0:3].copy().view(F)
        states[:, k] = out[:, 3]
        d[:, k] = l if sphere else (t * l[:, 0:1] + b * l[:, 1:2]) + nm * l[:, 2:3]
    return d, states


def trace(cs, origins, dirs, states, opts=None):
    """One path per row: from origins (m, 3) along dirs (m, 3) with the RNG state states (m,), started as a sample of hj_trace_paths
    is (throughput 1, extinction 0, wasDiscrete, bounce 0, first tMin = eps).  -> (radiance (m, 3) float32, first (m, 4): the first
    hit's normal and t, zeros for a miss; counts: closest_rays, hits, shadow_rays, unoccluded_shadow_rays)."""
    from oracle import hj_oracle as oracle
    o = opts if opts is not None else abi.RenderOpts.default()
    n = len(origins)
    counts = dict(closest_rays=0, hits=0, shadow_rays=0, unoccluded_shadow_rays=0)
    rec = records(origins, dirs, 0.0, np.zeros(n, np.int32), 0.0, 0.0, rng=np.asarray(states, U), bounce=0, discrete=1)
    tmin = np.full(n, KEPS, F)
    total = np.zeros((n, 3), F)
    first_nd = np.zeros((n, 4), F)
    live = np.arange(n)
    while len(live):
        r8 = np.concatenate([rec[:, 0:6].view(F), tmin[:, None], np.full((len(rec), 1), np.inf, F)], 1)
        ids, t, u, v = oracle.intersect(cs, r8)
        counts["closest_rays"] += len(rec)
        counts["hits"] += int((ids >= 0).sum())
        rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9] = words(t), ids.view(U), words(u), words(v)
        out = oracle.shade_step(cs, rec, o)
        total[live] = total[live] + out[:, 26:29].view(F)                                 # (+0 where the step added nothing)
        first = (rec[:, 17] >> 1) == 0
        first_nd[live[first]] = out[first, 29:33].view(F)
        sh = out[:, 15] == 1
        if sh.any():
            srays = np.concatenate([out[sh, 16:22].view(F), np.full((int(sh.sum()), 1), F(2) * KEPS, F), out[sh, 22:23].view(F)], 1)
            occ = oracle.intersect(cs, srays)[0] >= 0
            counts["shadow_rays"] += int(sh.sum())
            counts["unoccluded_shadow_rays"] += int((~occ).sum())
            idx = live[sh][~occ]
            total[idx] = total[idx] + out[sh][~occ][:, 23:26].view(F)
        go = out[:, 0] == 1
        nxt = np.zeros((int(go.sum()), IN), U)
        nxt[:, 0:3], nxt[:, 3:6], nxt[:, 10:13], nxt[:, 13:16] = out[go, 1:4], out[go, 4:7], out[go, 7:10], out[go, 12:15]
        nxt[:, 16], nxt[:, 17] = out[go, 11], out[go, 10]
        rec, live, tmin = nxt, live[go], np.full(int(go.sum()), F(2) * KEPS, F)
    return total, first_nd, counts


def compose_from_states(cs, rays, spp=1, opts=None):
    """path_query_ref.compose through trace(): the premise's form - states rng_seed(seeds + k), the caller's directions"""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n = len(rays)
    seeds = rays[:, 6].copy().view(U)
    counts = dict(closest_rays=0, hits=0, shadow_rays=0, unoccluded_shadow_rays=0, paths=n * spp)
    rgb, nd = np.zeros((n, 3), F), np.zeros((n, 4), F)
    for k in range(spp):
        L, first, c = trace(cs, rays[:, 0:3], rays[:, 3:6], R.rng_states(seeds + U(k)), opts)
        rgb = rgb + L
        if k == 0:
            nd = first
        for key, val in c.items():
            counts[key] += val
    return np.concatenate([rgb, np.full((n, 1), F(spp), F), nd], 1), counts


def sh9(d):
    """d (n, 3) float32 -> (n, 9): the header's basis in its order and operation order, float32"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full(len(d), C0, F), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * ((F(3.0) * z) * z - F(1.0)),
                     C2 * (x * z), C4 * (x * x - y * y)], 1).astype(F)


def gather(cs, points, spp=1, sphere=False, sh=False, opts=None):
    """-> (out (n, 8) or (n, 36) float32 as hj_trace_irradiance defines it, counts as the statistics count)"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 8)
    n = len(pts)
    d, states = directions(pts, spp, sphere)
    L, first, counts = trace(cs, np.repeat(pts[:, 0:3], spp, axis=0), d.reshape(-1, 3), states.reshape(-1), opts)
    L, t = L.reshape(n, spp, 3), first[:, 3].reshape(n, spp)
    out = np.zeros((n, 36 if sh else 8), F)
    for k in range(spp):                                                                  # float32, in the order of k, from +0
        out[:, 0:3] = out[:, 0:3] + L[:, k]
        if sh:
            Y = sh9(d[:, k])
            for j in range(9):
                out[:, 8 + 3 * j:11 + 3 * j] = out[:, 8 + 3 * j:11 + 3 * j] + Y[:, j:j + 1] * L[:, k]
    hit = t > 0
    out[:, 3] = F(spp)
    out[:, 4] = hit.sum(1).astype(F)
    out[:, 5] = np.where(hit, t, np.inf).min(1)
    counts["paths"] = n * spp
    return out, counts


# ------------------------------------------------------------------------------------------------------------------ point sets

SCENES = ("cbox", "rich", "env")          # pair nodes on and off, the environment instantiations (path_query_ref.SCENES)
N_SURFACE, N_FREE, N_SCALED = 300, 200, 60
AXES = F([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
N_POINTS = N_SURFACE + N_FREE + N_SCALED + len(AXES)


@functools.lru_cache(maxsize=None)
def point_set(name):
    """N_POINTS points of scene `name`, every position inside path_query_ref.domain:
      [0, 300)    ON surfaces, with the populated normal (oracle.intersect(full=True)) turned towards the probing ray
      [300, 500)  free points, random unit normals
      [500, 560)  free points, normal lengths in [0.5, 2]
      [560, 566)  free points with the six axis normals: both sides of |n.x| > |n.y| and its tie (0, 0, +-1)
    seeds random uint32, points 0, 1, 2: 0, 0xFFFFFFFE, 0xFFFFFFFF."""
    from oracle import hj_oracle as oracle
    cs = R.scene(name)
    rng = np.random.default_rng([11, list(R.SCENES).index(name)])
    lo, hi = R.domain(cs)
    probe = R.ray_set(name)[:2601].copy()
    probe[:, 6], probe[:, 7] = KEPS, np.inf
    ids, t, _, _, full = oracle.intersect(cs, probe, full=True)
    hit = np.flatnonzero((ids >= 0) & np.isfinite(t) & np.isfinite(full[:, 0:6]).all(1) & (full[:, 3:6] != 0).any(1))[:N_SURFACE]
    assert len(hit) == N_SURFACE
    pts = np.zeros((N_POINTS, 8), F)
    nm = full[hit, 3:6]
    facing = (nm.astype(np.float64) * probe[hit, 3:6]).sum(1) > 0
    pts[:N_SURFACE, 0:3] = np.clip(full[hit, 0:3], lo, hi)
    pts[:N_SURFACE, 3:6] = np.where(facing[:, None], -nm, nm)
    rest = N_POINTS - N_SURFACE
    pts[N_SURFACE:, 0:3] = rng.uniform(lo, hi, (rest, 3))
    v = rng.normal(size=(rest, 3))
    pts[N_SURFACE:, 3:6] = v / np.linalg.norm(v, axis=1, keepdims=True)
    a = N_SURFACE + N_FREE
    pts[a:a + N_SCALED, 3:6] *= rng.uniform(0.5, 2.0, (N_SCALED, 1)).astype(F)
    pts[a + N_SCALED:, 3:6] = AXES
    seeds = rng.integers(0, 1 << 32, N_POINTS, dtype=np.uint64).astype(U)
    seeds[0:3] = [0, 0xFFFFFFFE, 0xFFFFFFFF]
    pts.view(U)[:, 6] = seeds
    assert ((pts[:, 0:3] >= lo) & (pts[:, 0:3] <= hi)).all() and np.isfinite(pts[:, 0:6]).all()
    pts.setflags(write=False)
    return pts


MODES = {"hemisphere-1": (1, False, False), "hemisphere-5": (5, False, False), "sphere-sh9-4": (4, True, True)}


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """gather() of the scene's point set in one of MODES (spp, sphere, sh9), max_bounces = 40: computed once, never written to"""
    spp, sphere, sh = MODES[mode]
    out, counts = gather(R.scene(name), point_set(name), spp, sphere, sh, R.options(40))
    out.setflags(write=False)
    return out, counts


@functools.lru_cache(maxsize=None)
def closed_form_scene():
    """env_scenes.analytic_sky_scene (an upward quad at y = 0, a small sphere far below, the camera at y = 1) under a constant
    environment of 0.5"""
    import env_scenes
    return env_scenes.analytic_sky_scene(np.full((4, 8, 4), 0.5, F))


def closed_form_points(n=130):
    """points above all geometry (0.25 <= y <= 1, inside the domain), facing up"""
    rng = np.random.default_rng(5)
    pts = np.zeros((n, 8), F)
    pts[:, 0:3] = rng.uniform((-4.0, 0.25, -4.0), (4.0, 1.0, 4.0), (n, 3))
    pts[:, 4] = 1.0
    pts.view(U)[:, 6] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return pts
