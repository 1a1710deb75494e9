"""hj_render_direct_lit and the indirect-only gather restated in numpy, float32 throughout, from what exists already:

  trace()            gather_ref.trace generalised by one argument, the `discrete` that test_shade_step_gpu.records takes: the flags word a
                     path starts with.  discrete=1 is gather_ref.trace (test_direct_lit_host.py proves it); gather_indirect() is
                     gather_ref.gather over trace(discrete=0).
  direct_terms()     oracle.shade_step on the record (last segment, last hit, T = 1, ext = 0, rng = rng_seed(seed), bounce 0, discrete 0):
                     word 15 says whether a shadow ray is wanted, words 16..22 are the ray, words 23..25 are D; the ray's range is what
                     gather_ref.trace gives shadow rays, (2 eps, word 22).  Occlusion comes from a trace the caller brings.
  render()           probe_lit_ref.chains, compose and accumulate with D added as include/hijiki_hip.h says: L = Lp + D where the term
                     exists and its shadow ray finds nothing, L = Lp with no addition otherwise."""
import numpy as np

import follow_ref as R
import gather_ref as G
import path_query_ref as P
import probe_lit_ref as PL
from hijiki_amd import abi
from test_num_gpu import words
from test_shade_step_gpu import IN, KEPS, records

U, F = np.uint32, np.float32
DIFFUSE_TAGS = (abi.MAT_DIFFUSE, abi.MAT_DIFFUSECBOARD, abi.MAT_DIFFUSE_TEXTURED)


# ------------------------------------------------------------------------------------------------------------- the indirect gather

def trace(cs, origins, dirs, states, opts=None, discrete=1):
    """gather_ref.trace with the first record's wasDiscrete as an argument: nothing else of the loop differs"""
    from oracle import hj_oracle as oracle
    o = opts if opts is not None else abi.RenderOpts.default()
    n = len(origins)
    counts = dict(closest_rays=0, hits=0, shadow_rays=0, unoccluded_shadow_rays=0)
    rec = records(origins, dirs, 0.0, np.zeros(n, np.int32), 0.0, 0.0, rng=np.asarray(states, U), bounce=0, discrete=discrete)
    tmin = np.full(n, KEPS, F)
    total = np.zeros((n, 3), F)
    first_nd = np.zeros((n, 4), F)
    first_id = np.full(n, -1, np.int32)
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
        nxt = np.zeros((int(go.sum()), IN), U)
        nxt[:, 0:3], nxt[:, 3:6], nxt[:, 10:13], nxt[:, 13:16] = out[go, 1:4], out[go, 4:7], out[go, 7:10], out[go, 12:15]
        nxt[:, 16], nxt[:, 17] = out[go, 11], out[go, 10]
        rec, live, tmin = nxt, live[go], np.full(int(go.sum()), F(2) * KEPS, F)
    return total, first_nd, counts, first_id


def gather(cs, points, spp=1, sphere=False, sh=False, opts=None, discrete=1, detail=False):
    """gather_ref.gather over trace(discrete=) -> (out, counts) [, per sample (n, spp): radiance, the first segment's shape id]"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 8)
    n = len(pts)
    d, states = G.directions(pts, spp, sphere)
    L, first, counts, first_id = trace(cs, np.repeat(pts[:, 0:3], spp, axis=0), d.reshape(-1, 3), states.reshape(-1), opts, discrete)
    L, t = L.reshape(n, spp, 3), first[:, 3].reshape(n, spp)
    out = np.zeros((n, 36 if sh else 8), F)
    for k in range(spp):                                                                  # float32, in the order of k, from +0
        out[:, 0:3] = out[:, 0:3] + L[:, k]
        if sh:
            Y = G.sh9(d[:, k])
            for j in range(9):
                out[:, 8 + 3 * j:11 + 3 * j] = out[:, 8 + 3 * j:11 + 3 * j] + Y[:, j:j + 1] * L[:, k]
    hit = t > 0
    out[:, 3] = F(spp)
    out[:, 4] = hit.sum(1).astype(F)
    out[:, 5] = np.where(hit, t, np.inf).min(1)
    counts["paths"] = n * spp
    return (out, counts, L, first_id.reshape(n, spp)) if detail else (out, counts)


def gather_indirect(cs, points, spp=1, sphere=False, sh=False, opts=None, detail=False):
    """hj_trace_irradiance with HJ_GATHER_INDIRECT: a path starts with wasDiscrete clear"""
    return gather(cs, points, spp, sphere, sh, opts, discrete=0, detail=detail)


# ------------------------------------------------------------------------------------------------------------------ the direct term

def camera_rays_and_seeds(cs, blocks):
    """probe_lit_ref.camera_rays and, beside them, every sample's own seed (block.seed + lx + ly * dimension.x)"""
    if not len(blocks):
        return np.zeros((0, 8), F), np.zeros(0, U)
    rays = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    seeds = rays[:, 6].copy().view(U)
    rays[:, 6], rays[:, 7] = P.KEPS, np.inf
    return rays, seeds


def last_segments(cs, rays, max_follow, trace_fn):
    """probe_lit_ref.chains' loop again, keeping each chain's last segment (origin, direction) and its hit record (n, 4)"""
    n = len(rays)
    hits, surf = trace_fn(rays)
    last_hits = np.array(hits, F)
    origin, direction = np.array(rays[:, 0:3], F), np.array(rays[:, 3:6], F)
    live, cur = np.arange(n), np.asarray(rays, F)
    for _ in range(max_follow):
        nxt, cls = R.continue_rays(cs, cur, hits, surf)
        go = cls != R.END
        if not go.any():
            break
        live, cur = live[go], nxt[go]
        hits, surf = trace_fn(cur)
        last_hits[live], origin[live], direction[live] = hits, cur[:, 0:3], cur[:, 3:6]
        hit = hits[:, 0].copy().view(np.int32) >= 0
        live, cur, hits, surf = live[hit], cur[hit], hits[hit], surf[hit]
    return origin, direction, last_hits


def step_opts():
    """shade_step's options for the direct term: every wanted shadow ray is a record (no light-shaft grid); the bounce limits decide
    nothing of words 15..25"""
    o = abi.RenderOpts.default()
    o.flags |= abi.RENDER_NO_LIGHT_GRID
    return o


def direct_terms(cs, origin, direction, hits, seeds):
    """-> (wants (n,) bool: the sample has a direct term and so a shadow ray; rays (n, 8): origin p, direction sdir, tMin = 2 eps,
    tMax = stmax; D (n, 3)).  A sample whose last hit carries none of the three diffuse tags has none."""
    from oracle import hj_oracle as oracle
    n = len(hits)
    ids = hits[:, 0].copy().view(np.int32)
    total = int(cs.desc.num_spheres) + int(cs.desc.num_quads) + int(cs.desc.num_triangles)
    inside = (ids >= 0) & (ids < total)
    tags = np.where(inside, cs.materials[np.clip(ids, 0, max(total - 1, 0))] >> abi.MATERIAL_TAG_SHIFT, 0xFF) if total else np.full(n, 0xFF, U)
    dif = inside & np.isin(tags, DIFFUSE_TAGS)
    wants, rays, D = np.zeros(n, bool), np.zeros((n, 8), F), np.zeros((n, 3), F)
    if dif.any():
        rec = records(origin[dif], direction[dif], hits[dif, 1], ids[dif], hits[dif, 2], hits[dif, 3], rng=P.rng_states(seeds[dif]), bounce=0, discrete=0)
        out = oracle.shade_step(cs, rec, step_opts())
        sh = out[:, 15] == 1
        at = np.flatnonzero(dif)[sh]
        wants[at] = True
        rays[at] = np.concatenate([out[sh, 16:22].view(F), np.full((int(sh.sum()), 1), F(2) * KEPS, F), out[sh, 22:23].view(F)], 1)
        D[at] = out[sh, 23:26].view(F)
    return wants, rays, D


def oracle_occluded(cs):
    """an occlusion test that needs no GPU: the oracle's closest hit over the shadow ray's range"""
    from oracle import hj_oracle as oracle
    return lambda rays: oracle.intersect(cs, np.ascontiguousarray(rays, F))[0] >= 0


def zero_look(pts):
    return np.zeros((len(pts), 4), F)


def render(cs, blocks, width, height, max_follow, trace_fn, occluded, look=None, env=None, detail=False):
    """hj_render_direct_lit -> (height, width, 4) [, dict(chains, Lp, L, wants, counts: D counts, D, rays)].  look=None: no lighting
    (Lp = Le at a hit: probe_lit_ref.compose under a look-up of zeros gives Le + (albedo * 0) * (1 / pi), which is Le's bits for the
    finite albedos and non-negative emissions every scene here has - asserted)."""
    rays, seeds = camera_rays_and_seeds(cs, blocks)
    ch = PL.chains(cs, rays, max_follow, trace_fn)
    Lp = PL.compose(ch, look if look is not None else zero_look, env)
    if look is None:
        dif = ch["kind"] == PL.DIFFUSE
        assert (Lp[dif].view(U) == ch["emission"][dif].view(U)).all()
    origin, direction, hits = last_segments(cs, rays, max_follow, trace_fn)
    assert (direction.view(U) == ch["direction"].view(U)).all()
    wants, srays, D = direct_terms(cs, origin, direction, hits, seeds)
    counts = wants.copy()
    if wants.any():
        counts[wants] = ~np.asarray(occluded(srays[wants]), bool)
    L = Lp.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        L[counts] = (Lp[counts] + D[counts]).astype(F)
    img = PL.accumulate(width, height, blocks, L)
    return (img, dict(chains=ch, Lp=Lp, L=L, wants=wants, counts=counts, D=D, rays=srays, seeds=seeds, camera=rays)) if detail else img
