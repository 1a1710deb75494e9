"""The reference of hj_trace_irradiance_adaptive and of hj_bake_lightmap_adaptive's scatter, from the oracle alone.

expected() takes every sample's radiance and first-hit t from gather_ref.directions + gather_ref.trace with seeds + k (the oracle's
walk and shade step), restates the running state of include/hijiki_hip.h in numpy float32, operation for operation, and applies
path_adaptive_ref.stops - the one numpy text of the stop rule.  Only the samples a point actually receives are traced, so the counts
are the counts of the samples taken."""
import functools

import numpy as np

import gather_ref as G
import lightmap_ref as LR
import path_query_ref as R
from path_adaptive_ref import aopts, stops  # noqa: F401  (aopts: re-exported for the tests)

U, F = np.uint32, np.float32
COUNTS = G.COUNTS
# 4 / +4 / 16 at rel_error 0.5, floor 0.01 (path_adaptive_ref's default): test_gather_adaptive_host.py proves that it spreads every
# scene's point set over all four sample counts
KW = aopts()


def expected(cs, points, a, opts, sphere=False):
    """-> dict: out (n, 8) float32, moments (n, 4) uint32 (the bits of S1, S2, the last sem2; n_i), n (n,) int64, counts (COUNTS),
    rounds (adaptive rounds run), lists (the length of every round's list of points)."""
    pts = np.ascontiguousarray(points, F).reshape(-1, 8)
    n = len(pts)
    seeds = pts.view(U)[:, 6].copy()
    rgb, S1, S2, sem2 = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    hits, t_min = np.zeros(n, np.int64), np.full(n, np.inf, F)
    n_i = np.zeros(n, np.int64)
    counts = dict.fromkeys(COUNTS, 0)
    active = np.arange(n)
    done, rounds, lists = 0, 0, []
    while len(active):
        c = a["spp_min"] if done == 0 else min(a["spp_step"], a["spp_max"] - done)
        lists.append(len(active))
        for k in range(done, done + c):
            sub = pts[active].copy()
            sub.view(U)[:, 6] = seeds[active] + U(k)                                       # (uint32 wrap-around)
            d, states = G.directions(sub, 1, sphere)
            L, first, cnt = G.trace(cs, sub[:, 0:3], d[:, 0], states[:, 0], opts)
            for key, val in cnt.items():
                counts[key] += val
            counts["paths"] += len(active)
            r, g, b = L[:, 0], L[:, 1], L[:, 2]
            rgb[active] = rgb[active] + L
            Y = (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b
            S1[active] = S1[active] + Y
            S2[active] = S2[active] + Y * Y
            t = first[:, 3]
            hit = t > 0
            hits[active] += hit
            t_min[active] = np.where(hit, np.fmin(t_min[active], t), t_min[active])
        done += c
        rounds += 1
        n_i[active] = done
        stop, s = stops(S1[active], S2[active], done, a)
        sem2[active] = s
        active = active[~stop]
    out = np.concatenate([rgb, n_i.astype(F)[:, None], hits.astype(F)[:, None], t_min[:, None], np.zeros((n, 2), F)], 1)
    moments = np.stack([S1.view(U), S2.view(U), sem2.view(U), n_i.astype(U)], 1)
    return dict(out=out, moments=moments, n=n_i, counts=counts, rounds=rounds, lists=lists)


@functools.lru_cache(maxsize=None)
def expected_for(name, spp_min=4, spp_step=4, spp_max=16, rel_error=0.5, floor=0.01, sphere=False, max_bounces=40):
    """expected() of scene `name`'s point set (gather_ref.point_set): computed once per setting, never written to"""
    e = expected(R.scene(name), G.point_set(name), aopts(spp_min, spp_step, spp_max, rel_error, floor), R.options(max_bounces), sphere)
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return e


def scatter(points, records, W, H):
    """lightmap_ref.scatter with the scale per texel - points (n, 8), records (n, 8: word 3 = (float)n_i) -> ((H, W, 4) float32 image,
    (H, W) uint32 sample map)"""
    img, smap = np.zeros((H * W, 4), F), np.zeros(H * W, U)
    t = np.ascontiguousarray(points, F).view(U)[:, 7]
    rec = np.asarray(records, F)
    scale = LR.PI / rec[:, 3]                                                              # (float32 / float32: correctly rounded)
    assert scale.dtype == F
    img[t, 0:3] = rec[:, 0:3] * scale[:, None]
    img[t, 3] = 1.0
    smap[t] = rec[:, 3].astype(U)
    return img.reshape(H, W, 4), smap.reshape(H, W)
