"""The reference of hj_trace_paths_adaptive, from the oracle alone.

expected() takes every sample's radiance from path_query_ref.compose (spp = 1, seeds + k: the oracle's integrator, proven so by
test_path_query_host.py), restates the running sums and the stop rule of include/hijiki_hip.h in numpy float32, operation for
operation, and sums a ray's first n_i samples in order.  Only the samples a ray actually receives are composed, so the counts are the
counts of the samples taken."""
import functools

import numpy as np

import path_query_ref as R

U, F = np.uint32, np.float32
COUNTS = ("paths", "closest_rays", "shadow_rays", "hits", "unoccluded_shadow_rays")


def aopts(spp_min=4, spp_step=4, spp_max=16, rel_error=0.5, floor=0.01):
    """the adaptive options as Renderer.trace_paths_adaptive's keyword arguments"""
    return dict(spp_min=spp_min, spp_step=spp_step, spp_max=spp_max, rel_error=rel_error, floor=floor)


def stops(S1, S2, m, a):
    """the stop rule for (n,) float32 sums after m samples -> (stop (n,) bool, sem2 (n,) float32)"""
    with np.errstate(all="ignore"):
        mean = S1 / F(m)
        var = np.fmax(F(0), S2 - S1 * mean) / F(m - 1)
        sem2 = var / F(m)
        thr = F(a["rel_error"]) * np.fmax(mean, F(a["floor"]))
        stop = (sem2 <= thr * thr) | (m == a["spp_max"])
    assert mean.dtype == var.dtype == sem2.dtype == thr.dtype == F
    return stop, sem2


def expected(cs, rays, a, opts, sample=None):
    """-> dict: samples (n, 8) float32, moments (n, 4) uint32 (the bits of S1, S2, the last sem2; n_i), n (n,) int64, counts (COUNTS),
    rounds (adaptive rounds run), lists (the length of every round's list of rays).  sample(active, k) -> (the spp = 1 records of
    sample k of the rays `active`, their counts): where a sample comes from - by default the oracle, compose() with seeds + k."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n = len(rays)
    seeds = rays.view(U)[:, 6].copy()

    def composed(active, k):
        sub = rays[active].copy()
        sub.view(U)[:, 6] = seeds[active] + U(k)                                           # (uint32 wrap-around)
        return R.compose(cs, sub, 1, opts)
    sample = sample or composed
    rgb, S1, S2, sem2 = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    nd = np.zeros((n, 4), F)
    n_i = np.zeros(n, np.int64)
    counts = dict.fromkeys(COUNTS, 0)
    active = np.arange(n)
    done, rounds, lists = 0, 0, []
    while len(active):
        c = a["spp_min"] if done == 0 else min(a["spp_step"], a["spp_max"] - done)
        lists.append(len(active))
        for k in range(done, done + c):
            smp, cnt = sample(active, k)
            for key in COUNTS:
                counts[key] += cnt[key]
            r, g, b = smp[:, 0], smp[:, 1], smp[:, 2]
            rgb[active] = rgb[active] + smp[:, 0:3]
            Y = (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b
            S1[active] = S1[active] + Y
            S2[active] = S2[active] + Y * Y
            if k == 0:
                nd = smp[:, 4:8].copy()
        done += c
        rounds += 1
        n_i[active] = done
        stop, s = stops(S1[active], S2[active], done, a)
        sem2[active] = s
        active = active[~stop]
    samples = np.concatenate([rgb, n_i.astype(F)[:, None], nd], 1)
    moments = np.stack([S1.view(U), S2.view(U), sem2.view(U), n_i.astype(U)], 1)
    return dict(samples=samples, moments=moments, n=n_i, counts=counts, rounds=rounds, lists=lists)


@functools.lru_cache(maxsize=None)
def expected_for(name, spp_min=4, spp_step=4, spp_max=16, rel_error=0.5, floor=0.01, max_bounces=40):
    """expected() of scene `name`'s ray set (path_query_ref): computed once per setting, never written to"""
    e = expected(R.scene(name), R.ray_set(name), aopts(spp_min, spp_step, spp_max, rel_error, floor), R.options(max_bounces))
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return e
