"""The inputs of test_query_scale_gpu.py and test_query_scale_host.py: ray arrays far larger than path_query_ref.N_RAYS, the shape of
the adaptive query's compaction at such a size, a whole-array reference of an adaptive query composed from spp = 1 records, and
seeds next to 2^32.  Nothing here knows a GPU; the oracle is reached through path_query_ref, path_adaptive_ref and gather_ref."""
import functools

import numpy as np

import gather_ref as G
import path_adaptive_ref as A
import path_query_ref as R

U, F = np.uint32, np.float32
PA_THREADS = 256                    # kPaThreads: list entries of a compaction workgroup, and threads of the one scan workgroup
SCAN_TILE = PA_THREADS * PA_THREADS  # list entries beyond which a scan thread owns two or more counts
RUN = 70_001                        # rays of a run that the compaction sees as whole zero (or whole full) workgroups, > SCAN_TILE

# The large adaptive query.  Measured with the oracle on 30 000 rays of in_box_rays (4 / +4 / 16, rel_error 0.5, floor 0.01, cbox):
# 16.6 % of them enter the second round and 7.7 % the third, so the third round's list passes SCAN_TILE from about 851 000 such
# rays on.  930 000 leaves a margin of 9 % (the count's standard deviation is 0.04 %); the test asserts the lengths it got.
N_IN, N_BEFORE = 930_000, 300_000   # in-box rays in all, and those in front of the run of leaving rays
N_BIG = N_IN + RUN


def scan_shape(length):
    """k_pa_scan's view of a list of `length` entries -> (nb: counts, per: counts a thread owns)"""
    nb = -(-length // PA_THREADS)
    return nb, -(-nb // PA_THREADS)


def in_box_rays(n, rng):
    """origins uniform in the scene's root box (inside path_query_ref.domain, whose other two thirds are the empty space in front of
    the box up to the camera), unit directions uniform on the sphere, random seeds"""
    cs = R.scene("cbox")
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = rng.uniform(cs.bvh_f32[0, 0:3], cs.bvh_f32[0, 4:7], (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays.view(U)[:, 6] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return rays


def leaving_rays(n, rng):
    """rays that see nothing, as path_query_ref.ray_set makes them: from a point of the root box's faces, outwards"""
    cs = R.scene("cbox")
    blo, bhi = cs.bvh_f32[0, 0:3], cs.bvh_f32[0, 4:7]
    po = rng.uniform(blo, bhi, (n, 3))
    do = rng.normal(size=(n, 3))
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    rows = np.arange(n)
    po[rows, axis] = np.where(side == 1, bhi[axis], blo[axis])
    do[rows, axis] = np.where(side == 1, 1.0, -1.0) * (1.0 + np.abs(do[rows, axis]))
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6] = po, do / np.linalg.norm(do, axis=1, keepdims=True)
    rays.view(U)[:, 6] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return rays


@functools.lru_cache(maxsize=None)
def big_rays():
    """N_BIG rays of the cbox: [0, N_BEFORE) and [N_BEFORE + RUN, N_BIG) in_box_rays, between them RUN leaving_rays"""
    rng = np.random.default_rng(2024)
    inside = in_box_rays(N_IN, rng)
    rays = np.concatenate([inside[:N_BEFORE], leaving_rays(RUN, rng), inside[N_BEFORE:]])
    lo, hi = R.domain(R.scene("cbox"))
    assert len(rays) == N_BIG and ((rays[:, 0:3] >= lo) & (rays[:, 0:3] <= hi)).all()
    rays.setflags(write=False)
    return rays


def advanced(rays, k):
    """the seeds of `rays` advanced by k, uint32 wrap-around"""
    return ((rays.view(U)[:, 6].astype(np.uint64) + np.uint64(k)) & np.uint64(0xFFFFFFFF)).astype(U)


def from_table(rgb, nd, rows=None):
    """A sample source for path_adaptive_ref.expected out of recorded spp = 1 records: rgb[k] (n, 3) the radiance of sample k of
    every ray, nd (n, 4) the first hit of sample 0; rows: the table's row of every ray of the call (default: its own index).  Of the
    counts only `paths` is known."""
    def sample(active, k):
        at = active if rows is None else rows[active]
        smp = np.zeros((len(active), 8), F)
        smp[:, 0:3], smp[:, 3], smp[:, 4:8] = rgb[k][at], 1.0, nd[at]
        return smp, dict(dict.fromkeys(A.COUNTS, 0), paths=len(active))
    return sample


def sparse_indices(n, edges, total, seed):
    """`total` ray indices of a call of n rays: the first and the last, both sides of every edge (edges: ray indices at which something
    of the call's layout changes), the rest random; sorted"""
    must = {0, n - 1}
    for e in edges:
        must.update(i for i in (e - 1, e, e + 1) if 0 <= i < n)
    must = np.array(sorted(must))
    rest = np.setdiff1d(np.arange(n), must)
    fill = np.random.default_rng(seed).choice(rest, max(0, total - len(must)), replace=False)
    return np.sort(np.concatenate([must, fill]))


# ------------------------------------------------------------------------------------------------------ spp around and beyond 64

N_SPP = 300                          # rays or points: prefixes of the 3001-ray and 566-point sets
SPPS = (63, 64, 65, 130)
GATHER_MODES = {"hemisphere": (False, False), "sphere-sh9": (True, True)}
LONG = A.aopts(60, 70, 200, rel_error=0.1)    # rounds of 60, 70 and 70 samples


@functools.lru_cache(maxsize=None)
def paths_want(name, spp, n=N_SPP):
    samples, counts = R.compose(R.scene(name), R.ray_set(name)[:n], spp, R.options(40))
    samples.setflags(write=False)
    return samples, counts


@functools.lru_cache(maxsize=None)
def gather_want(name, spp, mode, n=N_SPP):
    sphere, sh9 = GATHER_MODES[mode]
    out, counts = G.gather(R.scene(name), G.point_set(name)[:n], spp, sphere, sh9, R.options(40))
    out.setflags(write=False)
    return out, counts


@functools.lru_cache(maxsize=None)
def long_rounds_want():
    return A.expected(R.scene("cbox"), R.ray_set("cbox")[:N_SPP], LONG, R.options(40))


# ------------------------------------------------------------------------------------------------------------ seeds at the wrap

N_WRAP = 64


def wrap_seeds():
    """0xFFFFFFFF - j: ray j's sample k has the seed 2^32 - 1 - j + k, which wraps to k - j - 1 from k = j + 1 on"""
    return (0xFFFFFFFF - np.arange(N_WRAP)).astype(U)


@functools.lru_cache(maxsize=None)
def wrap_rays():
    """The 64 rays of the cbox set that path_adaptive_ref.expected_for("cbox") gives the most samples (they keep much of that under
    new seeds: what a ray sees decides its variance), in the set's order, with wrap_seeds()"""
    n_i = A.expected_for("cbox")["n"]
    pick = np.sort(np.argsort(-n_i, kind="stable")[:N_WRAP])
    rays = R.ray_set("cbox")[pick].copy()
    rays.view(U)[:, 6] = wrap_seeds()
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def wrap_points():
    pts = G.point_set("cbox")[:N_WRAP].copy()
    pts.view(U)[:, 6] = wrap_seeds()
    pts.setflags(write=False)
    return pts
