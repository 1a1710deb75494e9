"""hj_trace_irradiance_adaptive and hj_bake_lightmap_adaptive on the GPU, bit for bit: every word of every record, every n_i, the
moments and the counts against gather_adaptive_ref.expected on three scenes (and one in sphere mode); the headline invariant on the
GPU alone - a point's record is hj_trace_irradiance's for that point at spp = n_i; the two ends of rel_error; a short last round;
spp_min == spp_max; pool, workgroup count, chunk size, point order, prefix length and the scan's run edge against each other; device
tensors; the context's state around a call; a call after hj_scene_update_shapes; refusals on the device route.  The bake: against
texels -> trace_irradiance_adaptive -> the reference's scatter / filter / dilation, its sample map against the reference's n_i, the
fixed-spp identity, the command line, and a property of the sample map."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_adaptive_ref as A
import gather_ref as G
import lightmap_filter_ref as FR
import lightmap_ref as LR
import lightmap_scenes as LS
import path_query_ref as R
import update_scenes
from refit_scenes import refit_numpy, shape_boxes
from hijiki_amd import abi, device, host
from test_abi import ROOT
from test_gather_gpu import assert_counts, assert_records, bits
from test_lightmap_filter_gpu import assert_image

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
KW = A.KW                                          # 4 / +4 / 16, rel_error 0.5, floor 0.01: test_gather_adaptive_host.py proves the spread


@pytest.fixture(scope="module")
def ga():
    with device.Renderer(0) as ctx:
        yield ctx


_default = {}


def default_result(ga, name="cbox", sphere=False):
    """(records, moments, statistics) of the scene's point set from the module's context: default switches, host arrays, KW"""
    ga.upload_scene(R.scene(name))
    if (name, sphere) not in _default:
        _default[name, sphere] = ga.trace_irradiance_adaptive(G.point_set(name), sphere=sphere, opts=R.options(40), stats=True, moments=True, **KW)
        _default[name, sphere][0].setflags(write=False)
        _default[name, sphere][1].setflags(write=False)
    return _default[name, sphere]


def assert_moments(got, want, what):
    bad = (bits(got) != want).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(want)} moment records differ, first at point {i}:\n  gpu  {bits(got)[i].tolist()}\n  want {want[i].tolist()}")


def assert_result(got, e, what):
    out, moments, stats = got
    took = np.bincount(e["n"])
    print(f"{what}: n_i {took.nonzero()[0].tolist()} x {took[took.nonzero()[0]].tolist()}, rounds {e['rounds']}, {e['counts']}")
    assert (out[:, 3] == e["n"]).all(), (what, int((out[:, 3] != e["n"]).sum()))
    assert_records(out, e["out"], what)
    assert_moments(moments, e["moments"], what)
    assert_counts(stats, e["counts"], what)
    assert stats["paths"] == int(e["n"].sum()) and stats["bounce_rounds"] == e["rounds"]
    assert stats["batches"] >= e["rounds"] and stats["total_ms"] > 0 and stats["path_launches"] == 0


def assert_grouped(r, pts, out, what, sphere=False, opts=None):
    """the headline invariant on the GPU alone: the points grouped by n_i, trace_irradiance(spp = n_i) of each group gives its records"""
    n_i = out[:, 3].astype(np.int64)
    for m in sorted(set(n_i.tolist())):
        idx = np.flatnonzero(n_i == m)
        assert_records(out[idx], r.trace_irradiance(pts[idx], spp=m, sphere=sphere, opts=opts or R.options(40)), f"{what}: the {len(idx)} points of n_i = {m}")
    return n_i


# ------------------------------------------------------------------------------------------------------------------ the gather

@pytest.mark.parametrize("name,sphere", [(n, False) for n in G.SCENES] + [("cbox", True)])
def test_every_record_matches_the_reference(ga, name, sphere):
    assert_result(default_result(ga, name, sphere), A.expected_for(name, sphere=sphere), f"{name}, sphere {sphere}")


@pytest.mark.parametrize("name,sphere", [("cbox", False), ("env", False), ("cbox", True)])
def test_a_record_is_the_fixed_spp_gather_of_its_point(ga, name, sphere):
    out, moments, _ = default_result(ga, name, sphere)
    n_i = assert_grouped(ga, G.point_set(name), out, name, sphere)
    assert set(n_i.tolist()) == {4, 8, 12, 16} and (bits(moments)[:, 3] == n_i).all()


def test_the_two_ends_of_rel_error(ga):
    """A huge rel_error stops every point after the first round: trace_irradiance(spp = spp_min).  rel_error = 0 stops a point before
    spp_max only when its samples so far have no variance at all (sem2 <= 0); every other point gets spp_max samples."""
    pts, o = G.point_set("cbox"), R.options(40)
    default_result(ga)
    got, stats = ga.trace_irradiance_adaptive(pts, opts=o, stats=True, **dict(KW, rel_error=1e18))
    assert_records(got, ga.trace_irradiance(pts, spp=4, opts=o), "rel_error 1e18")
    assert stats["bounce_rounds"] == 1 and stats["paths"] == 4 * len(pts) and stats["batches"] == 1
    got, mom, stats = ga.trace_irradiance_adaptive(pts, opts=o, stats=True, moments=True, **dict(KW, rel_error=0.0))
    e0 = A.expected_for("cbox", rel_error=0.0)
    n_i, full = bits(mom)[:, 3], bits(mom)[:, 3] == 16
    print(f"rel_error 0: {int(full.sum())} points at spp_max, {int((~full).sum())} without variance")
    assert (n_i == e0["n"]).all() and (mom[~full, 2] == 0).all() and full.sum() == int((e0["n"] == 16).sum()) > 300
    assert_records(got[full], ga.trace_irradiance(pts, spp=16, opts=o)[full], "rel_error 0, points with variance")
    assert_grouped(ga, pts, got, "rel_error 0")
    assert stats["bounce_rounds"] == e0["rounds"] and stats["paths"] == int(n_i.sum())


def test_a_short_last_round(ga):
    """4 / +5 / 11: rounds of 4, 5 and 2 samples"""
    e = A.expected_for("cbox", 4, 5, 11)
    assert set(e["n"].tolist()) == {4, 9, 11} and e["rounds"] == 3
    ga.upload_scene(R.scene("cbox"))
    got = ga.trace_irradiance_adaptive(G.point_set("cbox"), opts=R.options(40), stats=True, moments=True, **A.aopts(4, 5, 11))
    assert_result(got, e, "cbox, 4 / +5 / 11")


@pytest.mark.parametrize("spp", [2, 5])
def test_one_round_is_the_fixed_spp_gather(ga, spp):
    ga.upload_scene(R.scene("rich"))
    pts, o = G.point_set("rich"), R.options(40)
    want, want_stats = ga.trace_irradiance(pts, spp=spp, opts=o, stats=True)
    got, stats = ga.trace_irradiance_adaptive(pts, opts=o, stats=True, **A.aopts(spp, 3, spp, 0.25))
    assert_records(got, want, f"spp_min == spp_max == {spp}")
    for k in want_stats:
        assert k.endswith("_ms") or k == "bounce_rounds" or stats[k] == want_stats[k], (k, stats[k], want_stats[k])
    assert stats["bounce_rounds"] == 1


@pytest.mark.parametrize("switch", ["HJ_PATHS_POOL=64 HJ_PATHS_WGS=1", "HJ_PATHS_POOL=128 HJ_PATHS_WGS=3", "HJ_PATHS_CHUNK=1000"])
def test_scheduling_never_shows_in_a_result(ga, monkeypatch, switch):
    """A context created under the setting returns the bits of the default one, the same moments and the same counts.  Launches of
    1000 samples are launches of 250 points in every round (4 samples a point): one per 250 points of each round's list."""
    want, want_mom, want_stats = default_result(ga)
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(R.scene("cbox"))
        got, mom, stats = r.trace_irradiance_adaptive(G.point_set("cbox"), opts=R.options(40), stats=True, moments=True, **KW)
    assert_records(got, want, switch)
    assert_moments(mom, bits(want_mom), switch)
    assert_counts(stats, want_stats, switch)
    assert stats["bounce_rounds"] == want_stats["bounce_rounds"] == 4
    lists = A.expected_for("cbox")["lists"]
    assert stats["batches"] == (sum(-(-l // 250) for l in lists) if "CHUNK" in switch else 4)


def test_a_permutation_of_the_points_permutes_the_result(ga):
    want, want_mom, _ = default_result(ga)
    perm = np.random.default_rng(11).permutation(G.N_POINTS)
    got, mom = ga.trace_irradiance_adaptive(G.point_set("cbox")[perm], opts=R.options(40), moments=True, **KW)
    assert_records(got, want[perm], "permuted points")
    assert_moments(mom, bits(want_mom)[perm], "permuted points")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_prefixes(ga, n):
    """the compaction's wave and workgroup edges"""
    want, want_mom, _ = default_result(ga)
    got, mom = ga.trace_irradiance_adaptive(G.point_set("cbox")[:n], opts=R.options(40), moments=True, **KW)
    assert_records(got, want[:n], f"n = {n}")
    assert_moments(mom, bits(want_mom)[:n], f"n = {n}")


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_the_scans_run_edge(ga, n):
    """256 tiles of 256 points are one run of the scan's one workgroup: the point set tiled to one point below, at and above that
    edge, at 2 / +1 / 3, against the grouping invariant alone"""
    ga.upload_scene(R.scene("cbox"))
    pts = np.tile(G.point_set("cbox"), (n // G.N_POINTS + 1, 1))[:n]
    o = R.options(12)
    got, stats = ga.trace_irradiance_adaptive(pts, opts=o, stats=True, **A.aopts(2, 1, 3, 0.5))
    n_i = assert_grouped(ga, pts, got, f"n = {n}", opts=o)
    took = np.bincount(n_i, minlength=4)
    print(f"n = {n}: {took[2]} points at 2 samples, {took[3]} at 3")
    assert took[2] > 1000 and took[3] > 1000 and took[2] + took[3] == n
    assert stats["paths"] == int(n_i.sum()) and stats["bounce_rounds"] == 2
    assert np.array_equal(bits(got[:G.N_POINTS]), bits(got[G.N_POINTS:2 * G.N_POINTS]))


def test_device_tensors(ga):
    import torch
    want, want_mom, want_stats = default_result(ga, "rich")
    pts = G.point_set("rich")
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(pts.copy()).to(dev)
    keep = t.clone()
    got, mom, stats = ga.trace_irradiance_adaptive(t, opts=R.options(40), stats=True, moments=True, **KW)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.shape == (len(pts), 8) and mom.shape == (len(pts), 4)
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the point tensor changed"
    assert_records(got.cpu().numpy(), want, "device tensors")
    assert_moments(mom.cpu().numpy(), bits(want_mom), "device tensors")
    assert_counts(stats, want_stats, "device tensors")
    seeds = torch.from_numpy(pts.view(np.int32)[:, 6].copy()).to(dev)
    zeroed = t.clone()
    zeroed.view(torch.int32)[:, 6] = 0
    got2 = ga.trace_irradiance_adaptive(zeroed, seeds=seeds, opts=R.options(40), **KW)     # (no moments: NULL)
    assert int(zeroed.view(torch.int32)[:, 6].abs().sum()) == 0, "seeds were written into the caller's tensor"
    assert_records(got2.cpu().numpy(), want, "device tensors with seeds, no moments")
    for b in [t.cpu(), t.double(), t[::2], t[:, :7].contiguous(), t.reshape(-1)]:
        with pytest.raises(ValueError):
            ga.trace_irradiance_adaptive(b)
    assert tuple(ga.trace_irradiance_adaptive(t[:0]).shape) == (0, 8)


def test_the_texel_calls_own_tensor_as_it_stands(ga):
    """lightmap_texels(device=True) is a valid `points` argument: word 7 (the texel index) is ignored and survives"""
    import torch
    ga.upload_scene(LS.bake_scene())
    t = ga.lightmap_texels(64, 64, seed=11, seed_stride=7, offset=1e-3, device=True)
    keep = t.clone()
    got = ga.trace_irradiance_adaptive(t, opts=R.options(12), **KW)
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32))
    w7 = t.view(torch.int32)[:, 7].cpu().numpy()
    assert (np.diff(w7) > 0).all() and w7[-1] < 64 * 64 and w7[-1] > 0
    assert_records(got.cpu().numpy(), ga.trace_irradiance_adaptive(t.cpu().numpy(), opts=R.options(12), **KW), "the texel tensor against host arrays")
    assert len(set(got[:, 3].cpu().numpy().tolist())) == 4


def test_state_around_a_call():
    """A frame rendered before and after a call is the same frame - the call leaves the batch slots and the framebuffer alone -, and
    hj_trace_irradiance and hj_trace_paths_adaptive still answer as before."""
    cs, pts = R.scene("cbox"), G.point_set("cbox")
    e = A.expected_for("cbox")
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        r.create_framebuffer(96, 64)
        fixed_before = r.trace_irradiance(pts[:300], spp=2, opts=R.options(40))
        paths_before = r.trace_paths_adaptive(R.ray_set("cbox")[:300], opts=R.options(40), **KW)
        r.render_frame(2, 9)
        first = r.read().copy()
        got = r.trace_irradiance_adaptive(pts, opts=R.options(40), **KW)
        assert_records(got, e["out"], "between two frames")
        assert (bits(r.read()) == bits(first)).all(), "the call touched the framebuffer"
        r.clear()
        r.render_frame(2, 9)
        assert (bits(r.read()) == bits(first)).all(), "a frame after a call differs from the frame before it"
        assert_records(r.trace_irradiance(pts[:300], spp=2, opts=R.options(40)), fixed_before, "trace_irradiance after an adaptive gather")
        assert_records(r.trace_paths_adaptive(R.ray_set("cbox")[:300], opts=R.options(40), **KW), paths_before, "trace_paths_adaptive after an adaptive gather")


def test_after_an_update_with_moved_shapes(ga):
    rest, moved = update_scenes.light_show(triangles=150), update_scenes.light_show(moved=True, triangles=150)
    moved.set_bvh(refit_numpy(rest.bvh.copy(), shape_boxes(moved)))
    rng = np.random.default_rng(4)
    lo, hi = R.domain(moved)
    lo, hi = np.maximum(lo, [-1.2, 0.0, -1.2]), np.minimum(hi, [1.2, 2.0, 1.2])           # (inside the scene's box of quads)
    n = 600
    pts = np.zeros((n, 8), F)
    pts[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    pts[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    pts.view(U)[:, 6] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    o = R.options(40)
    e = A.expected(moved, pts, KW, o)
    assert len(set(e["n"].tolist())) >= 2
    ga.upload_scene(rest)
    before = ga.trace_irradiance_adaptive(pts, opts=o, **KW)
    ga.update_shapes(moved)
    got = ga.trace_irradiance_adaptive(pts, opts=o, stats=True, moments=True, **KW)
    assert (bits(got[0]) != bits(before)).any()
    assert_result(got, e, "moved shapes")


def test_refusals_on_the_device_route_write_nothing(ga):
    import torch
    L = device.lib()
    dev = torch.device("cuda", 0)
    ga.upload_scene(R.scene("cbox"))
    pts0 = G.point_set("cbox")[:64]
    pts, out, mom = torch.from_numpy(pts0.copy()).to(dev), torch.full((64, 8), 7.0, device=dev), torch.full((64, 4), 7.0, device=dev)
    img, smap = torch.full((16, 16, 4), 7.0, device=dev), torch.full((16, 16), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    DEV = abi.GATHER_DEVICE_ARRAYS
    ok, st, count = abi.AdaptiveOpts(4, 4, 16, 0.5, 0.01), abi.RenderStats(), C.c_size_t(77)
    o0 = abi.RenderOpts.default()
    o0.max_bounces = 0
    p, q, m = pts.data_ptr(), out.data_ptr(), mom.data_ptr()
    for args in ((p, 64, ok, None, DEV | 8, q, m), (p, 64, ok, None, DEV | abi.GATHER_SPHERE | abi.GATHER_SH9, q, m), (p, 64, None, None, DEV, q, m),
                 (p, 64, abi.AdaptiveOpts(1, 4, 16, 0.5, 0.01), None, DEV, q, m), (p, 64, abi.AdaptiveOpts(2, 1, 66, 0.5, 0.01), None, DEV, q, m),
                 (p + 4, 63, ok, None, DEV, q, m), (p, 63, ok, None, DEV, q, m + 4), (p, 64, ok, C.byref(o0), DEV, q, m), (None, 64, ok, None, DEV, q, m)):
        assert L.hj_trace_irradiance_adaptive(ga._h, *args, C.byref(st)) == abi.HJ_ERR_INVALID, args
        assert b"hj_trace_irradiance_adaptive" in L.hj_last_error(ga._h)
    bad = pts0.copy()
    bad[5, 3:6] = 0
    host_out = np.full((64, 8), 7.0, F)
    assert L.hj_trace_irradiance_adaptive(ga._h, bad.ctypes.data, 64, ok, None, 0, host_out.ctypes.data, None, C.byref(st)) == abi.HJ_ERR_INVALID
    assert b"point 5" in L.hj_last_error(ga._h)
    d = abi.LightmapDesc(16, 16, 0, 0, 0, 1, 0.0, abi.LIGHTMAP_DEVICE_ARRAYS)
    nine = abi.LightmapFilter(9, 0.1, 0.5, 0.0, 0)
    for a, gutter, f, im, sm in ((None, 2, None, img.data_ptr(), smap.data_ptr()), (abi.AdaptiveOpts(4, 0, 16, 0.5, 0.01), 2, None, img.data_ptr(), smap.data_ptr()),
                                 (ok, 65, None, img.data_ptr(), smap.data_ptr()), (ok, 2, C.byref(nine), img.data_ptr(), smap.data_ptr()),
                                 (ok, 2, None, img.data_ptr() + 8, smap.data_ptr()), (ok, 2, None, img.data_ptr(), smap.data_ptr() + 4)):
        assert L.hj_bake_lightmap_adaptive(ga._h, C.byref(d), a, gutter, f, None, im, sm, C.byref(count), C.byref(st)) == abi.HJ_ERR_INVALID
        assert b"hj_bake_lightmap_adaptive" in L.hj_last_error(ga._h)
    d_range = abi.LightmapDesc(16, 16, 1 << 30, 0, 0, 1, 0.0, abi.LIGHTMAP_DEVICE_ARRAYS)
    assert L.hj_bake_lightmap_adaptive(ga._h, C.byref(d_range), ok, 2, None, None, img.data_ptr(), smap.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_INVALID
    with device.Renderer(0) as r:                                       # no scene yet
        assert L.hj_trace_irradiance_adaptive(r._h, p, 64, ok, None, DEV, q, m, C.byref(st)) == abi.HJ_ERR_STATE
        assert b"scene" in L.hj_last_error(r._h)
        assert L.hj_bake_lightmap_adaptive(r._h, C.byref(d), ok, 2, None, None, img.data_ptr(), smap.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_STATE
    torch.cuda.synchronize(dev)
    assert bool((out == 7.0).all()) and bool((mom == 7.0).all()) and bool((img == 7.0).all()) and bool((smap == 7).all())
    assert (host_out == 7.0).all() and count.value == 77 and np.array_equal(bits(pts.cpu().numpy()), bits(pts0))
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


# ------------------------------------------------------------------------------------------------------------------ the bake

BAKE = dict(seed=11, seed_stride=7, offset=1e-3)


@pytest.mark.parametrize("W", [16, 64])
@pytest.mark.parametrize("env", [False, True], ids=["plain", "sky"])
def test_adaptive_bake_is_texels_adaptive_gather_scatter_filter_dilate(env, W):
    """... and its records and sample map are the reference's: gather_adaptive_ref.expected over the texels' points"""
    cs = LS.bake_scene(env)
    o = R.options(12)
    f = (2,) + device.default_filter_sigmas(cs)[0:2] + (0.8,)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        pts = r.lightmap_texels(W, W, **BAKE)
        rec, want_stats = r.trace_irradiance_adaptive(pts, opts=o, stats=True, **KW)
        e = A.expected(cs, pts, KW, o)
        assert_records(rec, e["out"], f"sky {env}, {W} x {W}: the gather")
        assert len(set(e["n"].tolist())) == 4
        scattered, want_map = A.scatter(pts, rec, W, W)
        ref_map = np.zeros(W * W, U)
        ref_map[pts.view(U)[:, 7]] = e["n"]
        assert np.array_equal(want_map.reshape(-1), ref_map)
        for gutter, flt in ((0, None), (2, None), (0, f), (2, f)):
            want = FR.run(scattered, pts, *flt) if flt else scattered
            for _ in range(gutter):
                want = LR.dilate(want)
            got, smap, stats = r.bake_lightmap(W, W, None, gutter=gutter, opts=o, stats=True, filter=flt, adaptive=KW, sample_map=True, **BAKE)
            what = f"sky {env}, {W} x {W}, gutter {gutter}, filter {flt is not None}"
            assert_image(got, want, what)
            assert smap.dtype == U and np.array_equal(smap, want_map), what
            for k in want_stats:                                        # every field of the gather's record but the times
                assert k.endswith("_ms") or stats[k] == want_stats[k], (k, stats[k], want_stats[k])
            assert stats["texels"] == len(pts) and (got[:, :, 3] == 1).sum() == len(pts) and ((got[:, :, 3] == 0.5).sum() > 0) == (gutter > 0)
            assert ((smap != 0) == (got[:, :, 3] == 1)).all()
        t, tmap = r.bake_lightmap(W, W, None, gutter=2, opts=o, device=True, filter=f, adaptive=KW, sample_map=True, **BAKE)
        assert t.is_cuda and tmap.is_cuda and np.array_equal(bits(t.cpu().numpy()), bits(got)) and np.array_equal(tmap.cpu().numpy().view(U), want_map)
        odd = r.bake_lightmap(W, W, None, gutter=1, opts=o, device=True, filter=f, adaptive=KW, **BAKE)      # 2 + 1 swaps, no sample map
        assert np.array_equal(bits(odd.cpu().numpy()), bits(r.bake_lightmap(W, W, None, gutter=1, opts=o, filter=f, adaptive=KW, **BAKE)))


@pytest.mark.parametrize("spp", [2, 5])
def test_one_round_is_the_fixed_spp_bake(spp):
    """spp_min == spp_max == spp: the image, the count and every statistic but the times are hj_bake_lightmap_filtered's at that spp -
    but bounce_rounds, which is the adaptive rounds run (1) here by the gather's contract and 0 in the fixed-spp bake; every texel
    with a record has `spp` in the sample map"""
    cs = LS.bake_scene()
    f = (2,) + device.default_filter_sigmas(cs)[0:2] + (0.8,)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        for W, gutter, flt in ((64, 2, f), (16, 0, None), (64, 1, None)):
            want, want_stats = r.bake_lightmap(W, W, spp, gutter=gutter, opts=R.options(12), stats=True, filter=flt, **BAKE)
            got, smap, stats = r.bake_lightmap(W, W, None, gutter=gutter, opts=R.options(12), stats=True, filter=flt, sample_map=True,
                                               adaptive=dict(spp_min=spp, spp_step=3, spp_max=spp, rel_error=0.1), **BAKE)
            assert_image(got, want, f"spp {spp}, {W} x {W}, gutter {gutter}")
            for k in want_stats:
                assert k.endswith("_ms") or k == "bounce_rounds" or stats[k] == want_stats[k], (k, stats[k], want_stats[k])
            assert stats["bounce_rounds"] == 1 and want_stats["bounce_rounds"] == 0 and stats["texels"] == want_stats["texels"] > 100
            assert np.array_equal(smap, np.where(want[:, :, 3] == 1, spp, 0).astype(U))


def test_cli_bakes_adaptively_like_the_library(tmp_path):
    import texture_scenes as ts
    obj = ts.write_obj_files(tmp_path, np.full((2, 2, 3), 0.5, F))
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    cs = host.Scene.from_obj(obj).compile()
    out, smap_file = str(tmp_path / "atlas.pfm"), str(tmp_path / "samples.pfm")
    r = subprocess.run([exe, "--bake-lightmap", "48x40", "--gutter", "1", "--filter", "2", "--adaptive", "4,4,16,0.5", "--sample-map", smap_file, "-s", "9",
                        "--seed", "6", "-o", out, obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Adaptive: " in r.stdout and "-s 9 is ignored" in r.stderr, r.stderr
    head, ghead = b"PF\n48 40\n-1.0\n", b"Pf\n48 40\n-1.0\n"
    assert open(out, "rb").read(len(head)) == head and open(smap_file, "rb").read(len(ghead)) == ghead
    got = np.frombuffer(open(out, "rb").read(), F, offset=len(head)).reshape(40, 48, 3)[::-1]
    got_map = np.frombuffer(open(smap_file, "rb").read(), F, offset=len(ghead)).reshape(40, 48)[::-1]
    with device.Renderer(0) as rr:
        rr.upload_scene(cs)
        want, want_map = rr.bake_lightmap(48, 40, None, gutter=1, seed=6, seed_stride=1, offset=1e-3, filter=(2,) + device.default_filter_sigmas(cs),
                                          adaptive=dict(spp_min=4, spp_step=4, spp_max=16, rel_error=0.5), sample_map=True)
    assert np.array_equal(bits(got), bits(want[:, :, 0:3])) and np.array_equal(got_map, want_map.astype(F))
    assert want_map.max() > 4 and set(np.unique(want_map).tolist()) <= {0, 4, 8, 12, 16}


def test_the_sample_map_spends_between_the_two_fixed_budgets():
    """A property: on the bake scene at 64 x 64 (seed 11, stride 7, offset 1e-3, max_bounces 12) with 4 / +4 / 16, rel_error 0.5,
    floor 0.01, the samples taken lie strictly between spp_min and spp_max a texel.  The setting was chosen on the CPU: the reference
    alone (gather_adaptive_ref.expected over lightmap_ref.texels) gives 3115 texels at 1858 / 593 / 193 / 471 points of 4 / 8 / 12 /
    16 samples, 22 028 samples in all, between 12 460 and 49 840 with room on both sides."""
    with device.Renderer(0) as r:
        r.upload_scene(LS.bake_scene())
        _, smap, stats = r.bake_lightmap(64, 64, None, gutter=2, opts=R.options(12), stats=True, adaptive=KW, sample_map=True, **BAKE)
    total, count = int(smap.sum(dtype=np.int64)), stats["texels"]
    print(f"{count} texels, {total} samples: between {4 * count} and {16 * count}; n_i {np.bincount(smap.reshape(-1))[[4, 8, 12, 16]].tolist()}")
    assert count == (smap != 0).sum() > 1000 and stats["paths"] == total
    assert 4 * count < total < 16 * count
