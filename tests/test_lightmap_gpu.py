"""hj_lightmap_texels and hj_bake_lightmap on the GPU, bit for bit: points and owner map against lightmap_ref (the contract in numpy
float32) on the edge-case scene at four atlas sizes, on a pair that covers a 1024 x 1024 atlas (the wave-walked route, several
scan tiles, the second scan level), on 20 000 sub-texel triangles (the lane-walked route), on sub-ranges, offsets and wrapping
seeds, under other launch shapes, with a capacity that is too small, as device tensors, after hj_scene_update_shapes; the bake
against the composition texels -> trace_irradiance -> the reference's scatter and dilation, against a closed form under a constant
sky, through the command line, and its refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lightmap_ref as LR
import lightmap_scenes as LS
import path_query_ref as R
from hijiki_amd import abi, device, host
from test_abi import ROOT

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
NONE = LR.NONE


def bits(a):
    return np.ascontiguousarray(a).view(U)


def assert_texels(got, want, what):
    (gp, go), (wp, wo) = got, want
    assert go.shape == wo.shape and np.array_equal(go, wo), (what, "owner map", int((go != wo).sum()), np.argwhere(go != wo)[:4].tolist())
    assert gp.shape == wp.shape, (what, gp.shape, wp.shape)
    diff = bits(gp) != bits(wp)
    if diff.any():
        i = int(np.argmax(diff.any(axis=1)))
        raise AssertionError(f"{what}: {int(diff.sum())} differing words in {int(diff.any(axis=1).sum())} of {len(wp)} points, first at {i}, words "
                             f"{np.flatnonzero(diff[i]).tolist()}:\n  gpu  {gp[i].tolist()}\n  want {wp[i].tolist()}")


def ref(cs, W, H, **kw):
    return LR.texels(cs.triangles, cs.vertices, W, H, **kw)


@pytest.fixture(scope="module")
def lm():
    with device.Renderer(0) as ctx:
        yield ctx


_edge = {}


def edge_reference(W, H):
    if (W, H) not in _edge:
        _edge[W, H] = ref(LS.edge_scene()[0], W, H)
        for a in _edge[W, H]:
            a.setflags(write=False)
    return _edge[W, H]


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (64, 64), (257, 131), (256, 256), (256, 257)])
def test_edge_cases_at_four_atlas_sizes(lm, W, H):
    """(the last two: 256 and 257 scan tiles - k_lm_scan's threads own one count each, then two, the last threads' runs empty)"""
    cs, case = LS.edge_scene()
    lm.upload_scene(cs)
    want = edge_reference(W, H)
    got = lm.lightmap_texels(W, H, owner=True)
    print(f"{W} x {H}: {len(want[0])} owned texels, {len(np.unique(want[1])) - 1} owning triangles")
    assert_texels(got, want, f"{W} x {H}")
    if (W, H) == (64, 64):
        assert len(want[0]) > 1000 and not (want[1] == case["zero normals"]).any()


def test_a_pair_over_all_of_1024_x_1024(lm):
    """the wave-walked route, 4096 scan tiles, the second scan level: every texel is owned, the diagonal by triangle 0"""
    cs = LS.full_pair_scene()
    lm.upload_scene(cs)
    pts, owner = lm.lightmap_texels(1024, 1024, seed=5, seed_stride=3, owner=True)
    assert len(pts) == 1 << 20
    want = ref(cs, 1024, 1024, seed=5, seed_stride=3)
    assert_texels((pts, owner), want, "1024 x 1024")
    assert np.array_equal(pts.view(U)[:, 7], np.arange(1 << 20, dtype=U)) and (np.diagonal(owner) == 0).all() and (owner == 1).sum() == 1023 * 512


_tiny = []


def tiny_reference():
    if not _tiny:
        _tiny.append(ref(LS.tiny_scene(), 512, 512))
        for a in _tiny[0]:
            a.setflags(write=False)
    return _tiny[0]


def test_20000_triangles_of_under_a_texel(lm):
    """the lane-walked route: most triangles cover no centre"""
    cs = LS.tiny_scene()
    lm.upload_scene(cs)
    want = tiny_reference()
    got = lm.lightmap_texels(512, 512, owner=True)
    print(f"{len(want[0])} owned texels of 20000 triangles")
    assert 500 < len(want[0]) < 10000
    assert_texels(got, want, "20000 tiny triangles")


@pytest.mark.parametrize("kw", [dict(first_triangle=0, num_triangles=0), dict(first_triangle=0, num_triangles=1), dict(first_triangle=3, num_triangles=11),
                                dict(first_triangle=14, num_triangles=0, offset=1e-3), dict(seed=0xFFFFFFF0, seed_stride=0x10000001, offset=1e-3)])
def test_sub_ranges_offsets_and_wrapping_seeds(lm, kw):
    cs, _ = LS.edge_scene()
    lm.upload_scene(cs)
    r = dict(kw)
    r["first"], r["num"] = r.pop("first_triangle", 0), r.pop("num_triangles", 0)
    want = ref(cs, 64, 64, **r)
    assert_texels(lm.lightmap_texels(64, 64, owner=True, **kw), want, str(kw))
    if r["num"]:
        o = want[1][want[1] != NONE]
        assert len(o) and o.min() >= r["first"] and o.max() < r["first"] + r["num"]
    if "seed" in kw:
        t = want[0].view(U)[:, 7].astype(np.uint64)
        assert (kw["seed"] + t * kw["seed_stride"] >= 1 << 32).any()                   # it does wrap
    n = len(cs.triangles)
    count = C.c_size_t(0)
    end = abi.LightmapDesc(64, 64, n, 0, 0, 1, 0.0, 0)                                   # no triangle in range: HJ_OK, a count of 0
    assert device.lib().hj_lightmap_texels(lm._h, C.byref(end), None, 0, None, C.byref(count)) == abi.HJ_OK and count.value == 0


@pytest.mark.parametrize("switch", ["HJ_LIGHTMAP_LANE_TEXELS=0 HJ_LIGHTMAP_SLICES=3", "HJ_LIGHTMAP_LANE_TEXELS=268435456", "HJ_LIGHTMAP_SLICES=7"])
def test_the_launch_shape_never_shows_in_a_result(monkeypatch, switch):
    """Every box walked by waves in three grid rows (the 20 000 sub-texel ones too), every box by one lane, seven rows on an atlas
    that is no power of two: a context created and loaded under the setting returns the REFERENCE's bytes - computed on the host,
    so no switch can reach it.  (An upload refreshes the context's copy of the switches: a result taken from another context in
    this test would be one under the same setting.)"""
    want = {"257 x 131": edge_reference(257, 131), "64 x 64": edge_reference(64, 64), "tiny": tiny_reference()}
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(LS.edge_scene()[0])
        assert_texels(r.lightmap_texels(257, 131, owner=True), want["257 x 131"], switch + ", 257 x 131")
        assert_texels(r.lightmap_texels(64, 64, owner=True), want["64 x 64"], switch + ", 64 x 64")
        r.upload_scene(LS.tiny_scene())
        assert_texels(r.lightmap_texels(512, 512, owner=True), want["tiny"], switch + ", tiny triangles")
        r.upload_scene(LS.full_pair_scene())
        pts, owner = r.lightmap_texels(96, 80, owner=True)               # two boxes of the whole atlas: 7680 points, the diagonal to 0
        assert_texels((pts, owner), ref(LS.full_pair_scene(), 96, 80), switch + ", a pair over 96 x 80")


def test_capacity(lm):
    cs, _ = LS.edge_scene()
    lm.upload_scene(cs)
    L = device.lib()
    want, want_owner = edge_reference(64, 64)
    n = len(want)
    d = abi.LightmapDesc(64, 64, 0, 0, 0, 1, 0.0, 0)
    count = C.c_size_t(0)
    assert L.hj_lightmap_texels(lm._h, C.byref(d), None, 0, None, C.byref(count)) == abi.HJ_OK and count.value == n
    pts, own = np.full((n, 8), 7.0, F), np.full((64, 64), 7, U)
    count.value = 0
    assert L.hj_lightmap_texels(lm._h, C.byref(d), pts.ctypes.data, n - 1, own.ctypes.data, C.byref(count)) == abi.HJ_ERR_INVALID
    assert count.value == n and (pts == 7.0).all() and (own == 7).all() and b"room for" in L.hj_last_error(lm._h)
    assert L.hj_lightmap_texels(lm._h, C.byref(d), pts.ctypes.data, n, own.ctypes.data, C.byref(count)) == abi.HJ_OK
    assert_texels((pts, own), (want, want_owner), "capacity = count")
    import torch
    dev = torch.device("cuda", 0)
    d.flags = abi.LIGHTMAP_DEVICE_ARRAYS
    tp, to = torch.full((n, 8), 7.0, device=dev), torch.full((64, 64), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    count.value = 0
    assert L.hj_lightmap_texels(lm._h, C.byref(d), tp.data_ptr(), n - 1, to.data_ptr(), C.byref(count)) == abi.HJ_ERR_INVALID
    assert count.value == n and bool((tp == 7.0).all()) and bool((to == 7).all())


def test_device_tensors(lm):
    """tensors hold the host arrays' bytes; the point tensor goes into trace_irradiance as it stands: word 7 is ignored there"""
    import torch
    cs, _ = LS.edge_scene()
    lm.upload_scene(cs)
    want = edge_reference(64, 64)
    pts, own = lm.lightmap_texels(64, 64, owner=True, device=True)
    assert isinstance(pts, torch.Tensor) and pts.is_cuda and own.dtype == torch.int32
    assert_texels((pts.cpu().numpy(), own.cpu().numpy().view(U)), want, "device tensors")
    assert tuple(lm.lightmap_texels(64, 64, first_triangle=len(cs.triangles), device=True).shape) == (0, 8)
    got, stats = lm.trace_irradiance(pts, spp=3, opts=R.options(8), stats=True)
    zeroed = pts.clone()
    zeroed.view(torch.int32)[:, 7] = 0
    got0, stats0 = lm.trace_irradiance(zeroed, spp=3, opts=R.options(8), stats=True)
    assert torch.equal(got.view(torch.int32), got0.view(torch.int32)) and stats["closest_rays"] == stats0["closest_rays"]
    assert np.array_equal(bits(pts.cpu().numpy()), bits(want[0])), "the point tensor changed"


def test_texels_follow_update_shapes(lm):
    """hj_scene_update_shapes rewrites the vertices the texel kernels read: after it the points are the reference's on the new arrays"""
    cs, _ = LS.edge_scene.__wrapped__()                                  # a scene of its own: the vertices are moved in place
    lm.upload_scene(cs)
    before = lm.lightmap_texels(64, 64, offset=1e-3, owner=True)
    LS.moved(cs)
    lm.update_shapes(cs)
    want = ref(cs, 64, 64, offset=1e-3)
    got = lm.lightmap_texels(64, 64, offset=1e-3, owner=True)
    assert_texels(got, want, "after update_shapes")
    assert not np.array_equal(bits(got[0][:, 0:3]), bits(before[0][:, 0:3])) if got[0].shape == before[0].shape else True


# ---------------------------------------------------------------------------------------------------------------------- the bake

W_B, H_B = 96, 80


def compose(r, W, H, spp, gutter, opts, **kw):
    """lightmap_texels -> trace_irradiance -> the reference's scatter and dilation"""
    pts = r.lightmap_texels(W, H, **kw)
    rec, stats = r.trace_irradiance(pts, spp=spp, opts=opts, stats=True)
    return LR.image(pts, rec, W, H, spp, gutter), stats, len(pts)


@pytest.mark.parametrize("env", [False, True], ids=["cbox", "env"])
def test_bake_is_texels_gather_scatter_dilate(lm, env):
    lm.upload_scene(LS.bake_scene(env))
    kw = dict(seed=11, seed_stride=7, offset=1e-3)
    for spp, gutters in ((1, (0, 1, 3)), (5, (0, 1, 3))) if not env else ((5, (1,)),):
        for gutter in gutters:
            want, want_stats, n = compose(lm, W_B, H_B, spp, gutter, R.options(12), **kw)
            got, stats = lm.bake_lightmap(W_B, H_B, spp, gutter=gutter, opts=R.options(12), stats=True, **kw)
            assert got.shape == (H_B, W_B, 4) and np.array_equal(bits(got), bits(want)), (env, spp, gutter, int((bits(got) != bits(want)).sum()))
            for k in want_stats:                                        # every field of the gather's record but the times
                assert k.endswith("_ms") or stats[k] == want_stats[k], (k, stats[k], want_stats[k])
            assert stats["paths"] == n * spp and stats["total_ms"] > 0
            assert stats["texels"] == n and 1500 < n < W_B * H_B and (got[:, :, 3] == 1).sum() == n
            assert ((got[:, :, 3] == 0.5).sum() > 0) == (gutter > 0) and (got[:, :, 0:3][got[:, :, 3] == 1] > 0).any()
    import torch
    t = lm.bake_lightmap(W_B, H_B, 5, gutter=3 if not env else 1, opts=R.options(12), device=True, **kw)
    assert t.is_cuda and np.array_equal(bits(t.cpu().numpy()), bits(got))
    even = lm.bake_lightmap(W_B, H_B, 5, gutter=2, opts=R.options(12), device=True, **kw)
    assert np.array_equal(bits(even.cpu().numpy()), bits(lm.bake_lightmap(W_B, H_B, 5, gutter=2, opts=R.options(12), **kw)))
    assert torch.cuda.is_available()


def test_closed_form_under_a_constant_sky(lm):
    """One upward pair alone under a constant sky of 0.5, spp = 64, points lifted off the surface: every sample leaves the scene
    with exactly 0.5, so a covered texel is exactly 32 * scale; the first gutter ring repeats it with alpha 0.5; beyond the passes: zero."""
    lm.upload_scene(LS.sky_pair_scene())
    W = H = 32
    scale = F(3.14159274) / F(64)
    value = F(32) * scale
    inside = np.zeros((H, W), bool)
    inside[8:24, 8:24] = True
    for gutter in (0, 1, 3):
        img = lm.bake_lightmap(W, H, 64, gutter=gutter, offset=1e-3, seed=9, opts=R.options(40))
        assert np.array_equal(img[:, :, 3] == 1, inside) and (img[inside][:, 0:3] == value).all()
        ring = np.zeros((H, W), bool)
        ring[8 - gutter:24 + gutter, 8 - gutter:24 + gutter] = True
        assert (img[~ring] == 0).all()
        assert (img[ring & ~inside][:, 3] == 0.5).all()
        if gutter:
            first = np.zeros((H, W), bool)
            first[7:25, 7:25] = True
            assert (img[first & ~inside][:, 0:3] == value).all()


def test_cli_bakes_like_the_library(tmp_path):
    import texture_scenes as ts
    obj = ts.write_obj_files(tmp_path, np.full((2, 2, 3), 0.5, F))
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    out = str(tmp_path / "atlas.pfm")
    r = subprocess.run([exe, "--bake-lightmap", "48x40", "--gutter", "3", "-s", "4", "--seed", "6", "-o", out, obj], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    head = b"PF\n48 40\n-1.0\n"
    got = np.frombuffer(open(out, "rb").read(), F, offset=len(head)).reshape(40, 48, 3)[::-1]
    with device.Renderer(0) as rr:
        rr.upload_scene(host.Scene.from_obj(obj).compile())
        want = rr.bake_lightmap(48, 40, 4, gutter=3, seed=6, seed_stride=1, offset=1e-3)
    assert np.array_equal(bits(got), bits(want[:, :, 0:3])) and (want[:, :, 3] == 1).sum() > 1000 and (want[:, :, 0:3] > 0).any()
    r = subprocess.run([exe, "--gutter", "3", obj], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--gutter without --bake-lightmap" in r.stderr


def test_refusals_on_the_device_route_write_nothing(lm):
    import torch
    cs, _ = LS.edge_scene()
    lm.upload_scene(cs)
    L = device.lib()
    dev = torch.device("cuda", 0)
    n = len(cs.triangles)
    pts, own = torch.full((4096, 8), 7.0, device=dev), torch.full((64, 64), 7, dtype=torch.int32, device=dev)
    img = torch.full((64, 64, 4), 7.0, device=dev)
    torch.cuda.synchronize(dev)
    count, st = C.c_size_t(77), abi.RenderStats()
    DEV = abi.LIGHTMAP_DEVICE_ARRAYS
    o0 = abi.RenderOpts.default()
    o0.max_bounces = 0
    for d in (abi.LightmapDesc(64, 64, n + 1, 0, 0, 1, 0.0, DEV), abi.LightmapDesc(64, 64, 2, n - 1, 0, 1, 0.0, DEV), abi.LightmapDesc(64, 64, 0, 0, 0, 1, 0.0, DEV | 2),
              abi.LightmapDesc(64, 0, 0, 0, 0, 1, 0.0, DEV), abi.LightmapDesc(64, 64, 0, 0, 0, 1, float("inf"), DEV)):
        assert L.hj_lightmap_texels(lm._h, C.byref(d), pts.data_ptr(), 4096, own.data_ptr(), C.byref(count)) == abi.HJ_ERR_INVALID
        assert b"hj_lightmap_texels" in L.hj_last_error(lm._h)
        assert L.hj_bake_lightmap(lm._h, C.byref(d), 4, 2, None, img.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_INVALID
        assert b"hj_bake_lightmap" in L.hj_last_error(lm._h)
    ok = abi.LightmapDesc(64, 64, 0, 0, 0, 1, 0.0, DEV)
    for args in ((0, 2, None), (4, 65, None), (4, 2, C.byref(o0))):
        assert L.hj_bake_lightmap(lm._h, C.byref(ok), args[0], args[1], args[2], img.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_INVALID
    assert L.hj_bake_lightmap(lm._h, C.byref(ok), 4, 2, None, img.data_ptr() + 4, C.byref(count), C.byref(st)) == abi.HJ_ERR_INVALID
    with device.Renderer(0) as r:                                       # no scene yet
        assert L.hj_lightmap_texels(r._h, C.byref(ok), pts.data_ptr(), 4096, own.data_ptr(), C.byref(count)) == abi.HJ_ERR_STATE
        assert L.hj_bake_lightmap(r._h, C.byref(ok), 4, 2, None, img.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_STATE
        assert b"scene" in L.hj_last_error(r._h)
    torch.cuda.synchronize(dev)
    assert bool((pts == 7.0).all()) and bool((own == 7).all()) and bool((img == 7.0).all()) and count.value == 77
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)
