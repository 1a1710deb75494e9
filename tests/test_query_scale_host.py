"""The premises of test_query_scale_gpu.py that need no GPU, from the oracle alone: the references wrap a seed at 2^32 as the header
promises, on rays and points that cross the wrap within their spp; a reference composed from a table of spp = 1 records is the
oracle's adaptive reference; the large ray array holds what its tests say of it; the settings spread the rays as the tests assume."""
import numpy as np

import gather_ref as G
import path_adaptive_ref as A
import path_query_ref as R
import query_scale_ref as Q

U, F = np.uint32, np.float32


def reseeded(rays, k):
    """`rays` with the seeds (seed + k) mod 2^32, computed in Python integers"""
    out = rays.copy()
    out.view(U)[:, 6] = np.array([(int(s) + k) % (1 << 32) for s in rays.view(U)[:, 6]], U)
    return out


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U), np.ascontiguousarray(b).view(U))


def test_seeds_at_the_wrap_cross_it():
    """seed 0xFFFFFFFF - j and sample k: the 33-bit sum passes 2^32 from k = j + 1 on - for rays 0..3 at spp 5, for every ray at spp
    65, for rays 0..14 within 16 adaptive samples; the advanced seeds and their RNG states are those of (seed + k) mod 2^32."""
    seeds = Q.wrap_seeds()
    assert seeds[0] == 0xFFFFFFFF and seeds[63] == 0xFFFFFFFF - 63 and (Q.wrap_rays().view(U)[:, 6] == seeds).all()
    assert (Q.wrap_points().view(U)[:, 6] == seeds).all()
    crossing = lambda spp: int((seeds.astype(np.int64) + spp - 1 >= 1 << 32).sum())  # noqa: E731
    assert (crossing(5), crossing(65), crossing(16)) == (4, 64, 15)
    for k in (0, 1, 4, 5, 64):
        want = np.array([(int(s) + k) % (1 << 32) for s in seeds], U)
        assert (Q.advanced(Q.wrap_rays(), k) == want).all() and (seeds + U(k) == want).all()
        assert (R.rng_states(seeds + U(k)) == R.rng_states(want)).all()
    assert Q.advanced(Q.wrap_rays(), 1)[0] == 0 and Q.advanced(Q.wrap_rays(), 64)[63] == 0


def test_compose_wraps_a_seed():
    """compose(spp) is the in-order float32 sum of compose(spp = 1) at the seeds (seed + k) mod 2^32, counts included"""
    cs, rays, o = R.scene("cbox"), Q.wrap_rays(), R.options(40)
    for spp in (5, 65):
        want, counts = R.compose(cs, rays, spp, o)
        total, summed = np.zeros((Q.N_WRAP, 3), F), dict.fromkeys(counts, 0)
        for k in range(spp):
            one, c = R.compose(cs, reseeded(rays, k), 1, o)
            total = total + one[:, 0:3]
            summed = {key: summed[key] + c[key] for key in summed}
        assert same(total, want[:, 0:3]) and summed == counts, spp
    assert not same(R.compose(cs, rays[:4], 5, o)[0], R.compose(cs, reseeded(rays[:4], 1 << 31), 5, o)[0])   # (the seed matters)


def test_gather_wraps_a_seed():
    """directions() of sample k is sample 0's at the seed (seed + k) mod 2^32 - direction and continued state -, and gather(spp)'s
    radiance is the in-order sum of gather(spp = 1) there"""
    cs, pts, o = R.scene("cbox"), Q.wrap_points(), R.options(40)
    for mode, (sphere, sh9) in Q.GATHER_MODES.items():
        d, states = G.directions(pts, 5, sphere)
        want, counts = G.gather(cs, pts, 5, sphere, sh9, o)
        total, paths = np.zeros((Q.N_WRAP, 3), F), 0
        for k in range(5):
            d1, s1 = G.directions(reseeded(pts, k), 1, sphere)
            assert same(d[:, k], d1[:, 0]) and (states[:, k] == s1[:, 0]).all(), (mode, k)
            one, c = G.gather(cs, reseeded(pts, k), 1, sphere, sh9, o)
            total = total + one[:, 0:3]
            paths += c["paths"]
        assert same(total, want[:, 0:3]) and paths == counts["paths"], mode


def test_the_adaptive_reference_wraps_a_seed():
    """expected() with its own samples equals expected() fed with compose at the seeds (seed + k) mod 2^32; rays that cross the wrap
    go on behind the first round, so that the seed of a later round's compacted ray (seed + n_after) wraps too"""
    cs, rays, o = R.scene("cbox"), Q.wrap_rays(), R.options(40)
    e = A.expected(cs, rays, A.aopts(), o)
    fed = A.expected(cs, rays, A.aopts(), o, sample=lambda active, k: R.compose(cs, reseeded(rays[active], k), 1, o))
    assert (e["n"] == fed["n"]).all() and same(e["samples"], fed["samples"]) and same(e["moments"], fed["moments"])
    assert e["counts"] == fed["counts"] and e["lists"] == fed["lists"]
    j = np.arange(Q.N_WRAP)
    assert any(((e["n"] > n_after) & (n_after > j)).any() for n_after in (4, 8, 12)), e["n"].tolist()


def test_a_table_of_spp1_records_composes_the_adaptive_reference():
    """from_table() on the oracle's own spp = 1 records of the 3001-ray set gives expected_for("cbox"): records, moments, n_i, lists;
    through a row map it gives the reference of the mapped rays"""
    cs, rays, o = R.scene("cbox"), R.ray_set("cbox"), R.options(40)
    want = A.expected_for("cbox")
    rgb, nd = [], None
    for k in range(16):
        sub = rays.copy()
        sub.view(U)[:, 6] = Q.advanced(rays, k)
        one, _ = R.compose(cs, sub, 1, o)
        rgb.append(one[:, 0:3].copy())
        nd = one[:, 4:8].copy() if k == 0 else nd
    e = A.expected(cs, rays, A.aopts(), o, sample=Q.from_table(rgb, nd))
    assert (e["n"] == want["n"]).all() and same(e["samples"], want["samples"]) and same(e["moments"], want["moments"])
    assert e["lists"] == want["lists"] and e["rounds"] == want["rounds"] and e["counts"]["paths"] == want["counts"]["paths"]
    rows = np.random.default_rng(3).permutation(R.N_RAYS)[:700]
    m = A.expected(cs, rays[rows], A.aopts(), o, sample=Q.from_table(rgb, nd, rows))
    assert same(m["samples"], want["samples"][rows]) and same(m["moments"], want["moments"][rows])


def test_scan_shape_is_the_kernels_arithmetic():
    """nb = ceil(length / 256), per = ceil(nb / 256): the 3001-ray set has one count a thread, 65 537 entries are the first with two"""
    assert Q.scan_shape(R.N_RAYS) == (12, 1) and Q.scan_shape(Q.SCAN_TILE) == (256, 1) and Q.scan_shape(Q.SCAN_TILE + 1) == (257, 2)
    assert Q.scan_shape(Q.N_BIG) == (3907, 16) and 3907 % 16 == 3                     # thread 244 owns 3 counts, threads 245.. none
    assert Q.scan_shape(Q.RUN)[1] == 2


def test_the_large_array():
    """unit directions, origins inside the domain, the run of leaving rays where the tests look for it - they hit nothing -, and rays
    that hit on both sides of it"""
    from oracle import hj_oracle as oracle
    from test_shade_step_gpu import KEPS
    cs, rays = R.scene("cbox"), Q.big_rays()
    assert rays.shape == (Q.N_BIG, 8) and Q.N_BIG % 2 == 1 and Q.RUN > Q.SCAN_TILE
    assert np.allclose(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1), 1.0, atol=1e-6)
    probe = rays[Q.N_BEFORE - 2000:Q.N_BEFORE + Q.RUN + 2000].copy()
    probe[:, 6], probe[:, 7] = KEPS, np.inf
    ids = oracle.intersect(cs, probe)[0]
    assert (ids[2000:2000 + Q.RUN] < 0).all()
    assert (ids[:2000] >= 0).mean() > 0.5 and (ids[-2000:] >= 0).mean() > 0.5
    assert len(np.unique(rays.view(U)[:, 6])) > 0.99 * Q.N_BIG


def test_the_settings_spread_the_rays():
    """60 / +70 / 200 on 300 rays takes all of 60, 130 and 200 samples; 300 rays at spp 63 are more 64-sample groups than three
    workgroups of 128 positions hold at once; the saturated plan's numbers"""
    e = Q.long_rounds_want()
    took = {m: int((e["n"] == m).sum()) for m in (60, 130, 200)}
    assert sum(took.values()) == Q.N_SPP and min(took.values()) >= 5 and e["rounds"] == 3, took
    assert Q.N_SPP * min(Q.SPPS) // 64 > 3 * 128 // 64
    assert Q.N_SPP <= len(G.point_set("cbox")) and Q.N_SPP <= R.N_RAYS
