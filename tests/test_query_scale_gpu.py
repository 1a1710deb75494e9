"""hj_trace_paths, hj_trace_paths_adaptive and hj_trace_irradiance beyond the sizes of their own test modules, bit for bit (0 differing
words everywhere):
  1. an adaptive query of a million rays, whose lists stay longer than one scan tile (256 x 256 entries) into the third round - every
     record and moment against a reference composed from spp = 1 queries (tied to the oracle at the 3001-ray size), 2000 of them
     against the oracle itself; whole zero and whole full tiles; a permutation; device tensors; small queries afterwards
  2. spp 63, 64, 65 and 130 - a ray's samples in two or three 64-sample groups, on different workgroups - on all three entry points
     against the oracle, also with three workgroups of 128 positions; adaptive rounds of 60, 70 and 70 samples; one ray larger than a
     launch
  3. seeds within spp of 2^32
  4. a fixed-spp query and a gather query of 4.34 million samples at the default launch plan: two launches of 2048 workgroups -
     1500 records against the oracle, every record and the counts against the same call made in pieces of 3001."""
import contextlib

import numpy as np
import pytest

import gather_ref as G
import path_adaptive_ref as A
import path_query_ref as R
import query_scale_ref as Q
from hijiki_amd import device
from test_gather_gpu import assert_records
from test_path_adaptive_gpu import assert_moments
from test_path_query_gpu import COUNTS, assert_counts, assert_samples, bits

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
KW = A.aopts()                                     # 4 / +4 / 16, rel_error 0.5, floor 0.01
THREE_WGS = "HJ_PATHS_WGS=3 HJ_PATHS_POOL=128"     # a ray's 64-sample groups land on three workgroups, and paths are regenerated


@pytest.fixture(scope="module")
def qs():
    with device.Renderer(0) as ctx:
        yield ctx


@contextlib.contextmanager
def context(qs, monkeypatch, switch):
    """the module's context at default switches, or one created under `switch`"""
    if not switch:
        yield qs
        return
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        yield r


def spp1_table(ctx, rays, spp_max):
    """sample k of every ray as hj_trace_paths gives it: spp = 1 with the seeds advanced by k -> (rgb[k] (n, 3), nd (n, 4) of k = 0)"""
    rgb, nd = [], None
    for k in range(spp_max):
        one = ctx.trace_paths(rays, seeds=Q.advanced(rays, k), opts=R.options(40))
        rgb.append(one[:, 0:3].copy())
        if k == 0:
            nd = one[:, 4:8].copy()
    return rgb, nd


# ------------------------------------------------------------------------------------------- 1. lists beyond one scan tile

_big = {}


def big_table(qs):
    qs.upload_scene(R.scene("cbox"))
    if "table" not in _big:
        _big["table"] = spp1_table(qs, Q.big_rays(), KW["spp_max"])
    return _big["table"]


def big_want(qs):
    """the whole-array reference of the large query at KW"""
    if "want" not in _big:
        _big["want"] = A.expected(R.scene("cbox"), Q.big_rays(), KW, R.options(40), sample=Q.from_table(*big_table(qs)))
    qs.upload_scene(R.scene("cbox"))
    return _big["want"]


def compacted(e, a):
    """the lists of the reference `e` that the call compacts: every round's but one that brings its rays to spp_max"""
    done, out = 0, []
    for length in e["lists"]:
        done += a["spp_min"] if done == 0 else min(a["spp_step"], a["spp_max"] - done)
        if done < a["spp_max"]:
            out.append(length)
    return out


def assert_whole(got, e, what):
    """samples, moments and statistics of a call against a reference out of a table: every word, the paths and the rounds"""
    samples, moments, stats = got
    print(f"{what}: lists {e['lists']}, scan shapes (nb, per) {[Q.scan_shape(n) for n in e['lists']]}, paths {int(e['n'].sum())}")
    assert_samples(samples, e["samples"], what)
    assert_moments(moments, e["moments"], what)
    assert stats["paths"] == int(e["n"].sum()) and stats["bounce_rounds"] == e["rounds"]


def test_spp1_queries_compose_the_oracles_adaptive_reference(qs):
    """Premise of the whole-array reference, at the pinned size: on the 3001-ray set the records, moments and sample counts composed
    from sixteen spp = 1 queries are path_adaptive_ref.expected_for("cbox"), the oracle's."""
    qs.upload_scene(R.scene("cbox"))
    rays, want = R.ray_set("cbox"), A.expected_for("cbox")
    e = A.expected(R.scene("cbox"), rays, KW, R.options(40), sample=Q.from_table(*spp1_table(qs, rays, KW["spp_max"])))
    assert (e["n"] == want["n"]).all() and e["rounds"] == want["rounds"] and e["lists"] == want["lists"]
    assert_samples(e["samples"], want["samples"], "composed from spp = 1 queries")
    assert_moments(e["moments"].view(F), want["moments"], "composed from spp = 1 queries")


def test_adaptive_lists_longer_than_a_scan_tile(qs):
    """A million rays at 4 / +4 / 16.  Asserted of the reference before anything is compared: the lists entering the second and the
    third round are longer than 65 536 entries, so that k_pa_scan's threads own two or more counts in two rounds whose list is an
    index list (src != NULL); in one round at least the counts are no multiple of a thread's share (a ragged last owner, idle owners
    behind it); the 70 001 leaving rays in the middle stop after the first round - whole workgroups of zero counts.  Then all 8 words
    of every record, all 4 of every moment, the paths and the rounds; and 2000 records against the oracle's own adaptive reference:
    the call's ends, rays 65 535 to 65 537, both sides of every multiple of 256 x per of the first round and of the run's ends."""
    rays, o = Q.big_rays(), R.options(40)
    e = big_want(qs)
    lists = compacted(e, KW)
    shapes = [Q.scan_shape(n) for n in lists]
    assert e["rounds"] == 4 and len(lists) == 3 and lists[0] == Q.N_BIG
    assert lists[1] > Q.SCAN_TILE and lists[2] > Q.SCAN_TILE, lists
    assert sum(per >= 2 for _, per in shapes[1:]) >= 2, shapes
    assert any(nb % per != 0 for nb, per in shapes), shapes
    run = slice(Q.N_BEFORE, Q.N_BEFORE + Q.RUN)
    assert Q.RUN > Q.SCAN_TILE and (e["n"][run] == 4).all() and set(e["n"].tolist()) == {4, 8, 12, 16}
    got = qs.trace_paths_adaptive(rays, opts=o, stats=True, moments=True, **KW)
    assert_whole(got, e, "a million rays")
    per0 = shapes[0][1]
    edges = [65536, Q.N_BEFORE, Q.N_BEFORE + Q.RUN] + list(range(Q.PA_THREADS * per0, Q.N_BIG, Q.PA_THREADS * per0))
    idx = Q.sparse_indices(Q.N_BIG, edges, 2000, seed=3)
    assert {0, 65535, 65536, 65537, Q.N_BIG - 1} <= set(idx.tolist())
    want = A.expected(R.scene("cbox"), rays[idx], KW, o)
    assert len(set(want["n"].tolist())) == 4
    assert_samples(got[0][idx], want["samples"], "2000 rays of the million against the oracle")
    assert_moments(got[1][idx], want["moments"], "2000 rays of the million against the oracle")


def test_whole_zero_and_whole_full_tiles(qs):
    """rel_error = 0 on 70 001 leaving rays, then 70 001 rays that keep their variance to spp_max (chosen from the table), then 5000
    of any kind: the first round's flags are a zero run and a full run longer than a scan tile each, and the later rounds' lists are
    full throughout - every count 256 - and longer than a scan tile too."""
    rays, o = Q.big_rays(), R.options(40)
    rgb, nd = big_table(qs)
    a0 = dict(KW, rel_error=0.0)
    cand = np.arange(120_000)                                                         # in-box rays: about 82 % of them have variance
    n_c = A.expected(R.scene("cbox"), rays[cand], a0, o, sample=Q.from_table(rgb, nd, cand))["n"]
    full = cand[n_c == 16][:Q.RUN]
    rows = np.concatenate([np.arange(Q.N_BEFORE, Q.N_BEFORE + Q.RUN), full, np.random.default_rng(8).choice(Q.N_BIG, 5000, replace=False)])
    e = A.expected(R.scene("cbox"), rays[rows], a0, o, sample=Q.from_table(rgb, nd, rows))
    assert len(full) == Q.RUN and (e["n"][:Q.RUN] == 4).all() and (e["n"][Q.RUN:2 * Q.RUN] == 16).all()
    lists = compacted(e, a0)
    assert e["rounds"] == 4 and all(n > Q.SCAN_TILE and Q.scan_shape(n)[1] >= 2 for n in lists), lists
    assert lists[1] == lists[2] == int((e["n"] == 16).sum())                          # nothing stops between the first round and spp_max
    got = qs.trace_paths_adaptive(rays[rows], opts=o, stats=True, moments=True, **a0)
    assert_whole(got, e, "zero and full tiles")


def test_a_permutation_of_a_million_rays_permutes_the_result(qs):
    e = big_want(qs)
    perm = np.random.default_rng(12).permutation(Q.N_BIG)
    got, mom = qs.trace_paths_adaptive(Q.big_rays()[perm], opts=R.options(40), moments=True, **KW)
    assert_samples(got, e["samples"][perm], "permuted rays")
    assert_moments(mom, e["moments"][perm], "permuted rays")


def test_a_million_rays_from_device_tensors(qs):
    import torch
    e = big_want(qs)
    t = torch.from_numpy(Q.big_rays().copy()).to(torch.device("cuda", 0))
    got, stats = qs.trace_paths_adaptive(t, opts=R.options(40), stats=True, **KW)      # (no moments: NULL)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (Q.N_BIG, 8)
    assert_samples(got.cpu().numpy(), e["samples"], "device tensors")
    assert stats["paths"] == int(e["n"].sum()) and stats["bounce_rounds"] == e["rounds"]


def test_small_queries_after_a_large_one(qs):
    """The path state and the adaptive arrays have grown for a million rays; a 3001-ray query of each entry point on the same context
    returns what its own module pins."""
    qs.upload_scene(R.scene("cbox"))
    o = R.options(40)
    qs.trace_paths_adaptive(Q.big_rays(), opts=o, **KW)
    got, stats = qs.trace_paths(R.ray_set("cbox"), opts=o, stats=True)
    assert_samples(got, R.expected("cbox", 40)[0], "trace_paths after the large query")
    assert_counts(stats, R.expected("cbox", 40)[1], "trace_paths after the large query")
    got, stats = qs.trace_irradiance(G.point_set("cbox"), spp=4, sphere=True, sh9=True, opts=o, stats=True)
    assert_records(got, G.expected("cbox", "sphere-sh9-4")[0], "trace_irradiance after the large query")
    assert_counts(stats, G.expected("cbox", "sphere-sh9-4")[1], "trace_irradiance after the large query")
    e = A.expected_for("cbox")
    got, mom, stats = qs.trace_paths_adaptive(R.ray_set("cbox"), opts=o, stats=True, moments=True, **KW)
    assert_samples(got, e["samples"], "trace_paths_adaptive after the large query")
    assert_moments(mom, e["moments"], "trace_paths_adaptive after the large query")
    assert_counts(stats, e["counts"], "trace_paths_adaptive after the large query")


# --------------------------------------------------------------------------------------------- 2. spp around and beyond 64

@pytest.mark.parametrize("switch", ["", THREE_WGS])
@pytest.mark.parametrize("spp", Q.SPPS)
@pytest.mark.parametrize("name", ["cbox", "env"])
def test_paths_with_samples_in_several_groups(qs, monkeypatch, name, spp, switch):
    want, counts = Q.paths_want(name, spp)
    with context(qs, monkeypatch, switch) as r:
        r.upload_scene(R.scene(name))
        got, stats = r.trace_paths(R.ray_set(name)[:Q.N_SPP], spp=spp, opts=R.options(40), stats=True)
    assert_samples(got, want, f"{name}, spp {spp} {switch}")
    assert_counts(stats, counts, f"{name}, spp {spp} {switch}")
    assert stats["batches"] == 1 and (got[:, 3] == spp).all()


@pytest.mark.parametrize("switch", ["", THREE_WGS])
@pytest.mark.parametrize("mode", list(Q.GATHER_MODES))
@pytest.mark.parametrize("spp", Q.SPPS)
@pytest.mark.parametrize("name", ["cbox", "env"])
def test_gather_with_samples_in_several_groups(qs, monkeypatch, name, spp, mode, switch):
    want, counts = Q.gather_want(name, spp, mode)
    sphere, sh9 = Q.GATHER_MODES[mode]
    with context(qs, monkeypatch, switch) as r:
        r.upload_scene(R.scene(name))
        got, stats = r.trace_irradiance(G.point_set(name)[:Q.N_SPP], spp=spp, sphere=sphere, sh9=sh9, opts=R.options(40), stats=True)
    assert_records(got, want, f"{name}, {mode}, spp {spp} {switch}")
    assert_counts(stats, counts, f"{name}, {mode}, spp {spp} {switch}")
    assert stats["batches"] == 1


@pytest.mark.parametrize("switch", ["", THREE_WGS])
def test_adaptive_rounds_of_60_70_and_70_samples(qs, monkeypatch, switch):
    e = Q.long_rounds_want()
    assert e["rounds"] == 3 and set(e["n"].tolist()) == {60, 130, 200}
    with context(qs, monkeypatch, switch) as r:
        r.upload_scene(R.scene("cbox"))
        got, mom, stats = r.trace_paths_adaptive(R.ray_set("cbox")[:Q.N_SPP], opts=R.options(40), stats=True, moments=True, **Q.LONG)
    assert_samples(got, e["samples"], f"60 / +70 / 200 {switch}")
    assert_moments(mom, e["moments"], f"60 / +70 / 200 {switch}")
    assert_counts(stats, e["counts"], f"60 / +70 / 200 {switch}")
    assert stats["paths"] == int(e["n"].sum()) and stats["bounce_rounds"] == 3


def test_one_ray_larger_than_a_launch(qs, monkeypatch):
    """HJ_PATHS_CHUNK = 64 and spp = 100: a launch takes one whole ray or point (chunk_rays = max(1, 64 / 100)), five launches for
    five of them; the records are the default context's, and the oracle's."""
    qs.upload_scene(R.scene("cbox"))
    o = R.options(40)
    rays, pts = R.ray_set("cbox")[:5], G.point_set("cbox")[:5]
    default = [qs.trace_paths(rays, spp=100, opts=o, stats=True)]
    default += [qs.trace_irradiance(pts, spp=100, sphere=s, sh9=h, opts=o, stats=True) for s, h in Q.GATHER_MODES.values()]
    monkeypatch.setenv("HJ_PATHS_CHUNK", "64")
    with device.Renderer(0) as r:
        r.upload_scene(R.scene("cbox"))
        got = [r.trace_paths(rays, spp=100, opts=o, stats=True)]
        got += [r.trace_irradiance(pts, spp=100, sphere=s, sh9=h, opts=o, stats=True) for s, h in Q.GATHER_MODES.values()]
    want = [Q.paths_want("cbox", 100, 5)] + [Q.gather_want("cbox", 100, mode, 5) for mode in Q.GATHER_MODES]
    for what, (rec, stats), (drec, dstats), (wrec, wcounts) in zip(("paths", "hemisphere", "sphere-sh9"), got, default, want):
        assert stats["batches"] == 5 and dstats["batches"] == 1, what
        assert_records(rec, drec, f"{what}: one launch a ray against the default context")
        assert_records(rec, wrec, f"{what}: one launch a ray against the oracle")
        assert_counts(stats, dstats, what)
        assert_counts(stats, wcounts, what)


# -------------------------------------------------------------------------------------------------- 3. seeds at the wrap

@pytest.mark.parametrize("spp", [5, 65])
def test_paths_with_seeds_at_the_wrap(qs, spp):
    qs.upload_scene(R.scene("cbox"))
    rays = Q.wrap_rays()
    want, counts = R.compose(R.scene("cbox"), rays, spp, R.options(40))
    got, stats = qs.trace_paths(rays, spp=spp, opts=R.options(40), stats=True)
    assert_samples(got, want, f"seeds at the wrap, spp {spp}")
    assert_counts(stats, counts, f"seeds at the wrap, spp {spp}")
    zeroed = rays.copy()
    zeroed.view(U)[:, 6] = 0
    assert_samples(qs.trace_paths(zeroed, seeds=Q.wrap_seeds(), spp=spp, opts=R.options(40)), want, f"seeds= at the wrap, spp {spp}")
    assert (zeroed.view(U)[:, 6] == 0).all()


@pytest.mark.parametrize("mode", list(Q.GATHER_MODES))
def test_gather_with_seeds_at_the_wrap(qs, mode):
    qs.upload_scene(R.scene("cbox"))
    sphere, sh9 = Q.GATHER_MODES[mode]
    want, counts = G.gather(R.scene("cbox"), Q.wrap_points(), 5, sphere, sh9, R.options(40))
    got, stats = qs.trace_irradiance(Q.wrap_points(), spp=5, sphere=sphere, sh9=sh9, opts=R.options(40), stats=True)
    assert_records(got, want, f"seeds at the wrap, {mode}")
    assert_counts(stats, counts, f"seeds at the wrap, {mode}")


def test_adaptive_with_seeds_at_the_wrap(qs):
    """4 / +4 / 16 on seeds 0xFFFFFFFF - j: ray j enters the round behind n_after samples with the seed 2^32 - 1 - j + n_after, which
    k_pa_scatter must wrap for n_after > j.  The reference says that this happens: some ray j goes on behind an n_after above j."""
    qs.upload_scene(R.scene("cbox"))
    rays = Q.wrap_rays()
    e = A.expected(R.scene("cbox"), rays, KW, R.options(40))
    j = np.arange(Q.N_WRAP)
    assert any(((e["n"] > n_after) & (n_after > j)).any() for n_after in (4, 8, 12)), e["n"].tolist()
    got, mom, stats = qs.trace_paths_adaptive(rays, opts=R.options(40), stats=True, moments=True, **KW)
    assert_samples(got, e["samples"], "adaptive, seeds at the wrap")
    assert_moments(mom, e["moments"], "adaptive, seeds at the wrap")
    assert_counts(stats, e["counts"], "adaptive, seeds at the wrap")


# --------------------------------------------------------------------------------------------- 4. the default plan, saturated

N_FIXED, SPP_FIXED = 140_000, 31                   # 4 340 000 samples: above 2^22 + 2^17
CHUNK_RAYS = (1 << 22) // SPP_FIXED                # rays of a launch at the default HJ_PATHS_CHUNK: 135 300


def in_pieces(query, n, width, piece=R.N_RAYS):
    """the same query made on [0, 3001), [3001, 6002), ...: the records concatenated, the additive counters summed"""
    out, total = np.zeros((n, width), F), dict.fromkeys(COUNTS, 0)
    for at in range(0, n, piece):
        rec, stats = query(slice(at, min(n, at + piece)))
        out[at:at + piece] = rec
        for key in COUNTS:
            total[key] += stats[key]
    return out, total


def fixed_indices():
    return Q.sparse_indices(N_FIXED, [CHUNK_RAYS, 65536], 1500, seed=6)


def test_the_plan_saturates():
    """what the two tests below rely on: more samples than the first launch and 2048 x 64 more take, so both launches have a 64-sample
    group for each of the 2048 workgroups; the launch boundary lies inside the call"""
    assert N_FIXED * SPP_FIXED > (1 << 22) + (1 << 17) and 0 < N_FIXED - CHUNK_RAYS < CHUNK_RAYS
    assert {0, CHUNK_RAYS - 1, CHUNK_RAYS, N_FIXED - 1} <= set(fixed_indices().tolist())


def test_paths_at_the_saturated_default_plan(qs):
    qs.upload_scene(R.scene("cbox"))
    rays, o = Q.big_rays()[:N_FIXED], R.options(40)
    got, stats = qs.trace_paths(rays, spp=SPP_FIXED, opts=o, stats=True)
    assert stats["batches"] == 2 and stats["paths"] == N_FIXED * SPP_FIXED
    idx = fixed_indices()
    want, _ = R.compose(R.scene("cbox"), rays[idx], SPP_FIXED, o)
    assert_samples(got[idx], want, "1500 rays of 140 000 against the oracle")
    pieces, total = in_pieces(lambda s: qs.trace_paths(rays[s], spp=SPP_FIXED, opts=o, stats=True), N_FIXED, 8)
    assert_samples(got, pieces, "one call against pieces of 3001")
    assert_counts(stats, total, "one call against pieces of 3001")


def test_gather_at_the_saturated_default_plan(qs):
    """sphere + SH9: the 36-word records of the second launch land behind the first launch's"""
    qs.upload_scene(R.scene("cbox"))
    pts, o = Q.big_rays()[:N_FIXED], R.options(40)                                      # (position, a unit normal, a seed)
    kw = dict(spp=SPP_FIXED, sphere=True, sh9=True, opts=o, stats=True)
    got, stats = qs.trace_irradiance(pts, **kw)
    assert stats["batches"] == 2 and stats["paths"] == N_FIXED * SPP_FIXED
    idx = fixed_indices()
    want, _ = G.gather(R.scene("cbox"), pts[idx], SPP_FIXED, True, True, o)
    assert_records(got[idx], want, "1500 points of 140 000 against the oracle")
    pieces, total = in_pieces(lambda s: qs.trace_irradiance(pts[s], **kw), N_FIXED, 36)
    assert_records(got, pieces, "one call against pieces of 3001")
    assert_counts(stats, total, "one call against pieces of 3001")
