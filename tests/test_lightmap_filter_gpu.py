"""hj_filter_lightmap and hj_bake_lightmap_filtered on the GPU, bit for bit against lightmap_filter_ref (the contract in numpy
float32): the edge-case scene's texels at four atlas sizes under eleven filters, a pair over 1024 x 1024 through both kernel forms,
two charts side by side in the atlas and apart in space, both forms forced at every step size, the call routes (host arrays, device
tensors, the texel call's tensor as it stands, a point that names no texel), the filtered bake against the composition of its
parts, the refusals on the device route - and one property: the filter brings a 4-spp bake closer to a 4096-spp one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lightmap_filter_ref as FR
import lightmap_ref as LR
import lightmap_scenes as LS
import path_query_ref as R
from hijiki_amd import abi, device, host
from test_abi import ROOT

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32


def bits(a):
    return np.ascontiguousarray(a).view(U)


def assert_image(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = (bits(got) != bits(want)).any(axis=-1)
    if diff.any():
        y, x = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} texels differ, first at x = {x}, y = {y}:\n  gpu  {got[y, x].tolist()}\n"
                             f"  want {want[y, x].tolist()}")


@pytest.fixture(scope="module")
def lm():
    with device.Renderer(0) as ctx:
        ctx.upload_scene(LS.edge_scene()[0])                            # (the filter reads no scene, but a query needs one uploaded)
        yield ctx


_edge = {}


def edge_case(W, H):
    """the edge-case scene's texels as guides (positions scattered over space: neighbours in the atlas are often far apart) and an image"""
    if (W, H) not in _edge:
        cs = LS.edge_scene()[0]
        pts, _ = LR.texels(cs.triangles, cs.vertices, W, H, offset=1e-3)
        img = np.random.default_rng([W, H]).uniform(0.0, 2.0, (H, W, 4)).astype(F)
        pts.setflags(write=False)
        img.setflags(write=False)
        _edge[W, H] = (img, pts)
    return _edge[W, H]


# (iterations, sigma_position, sigma_normal, sigma_color).  1e-6: 1 / sigma^2 = 1e12, so hj_exp underflows to 0 for every tap that is
# not at the texel's own position; 1e15: 1 / sigma^2 = 1e-30, a normal float32, and hj_exp(-a) is 1 or its neighbour.
FILTERS = [(1, 0.3, 0.5, 0.4), (2, 0.3, 0.5, 0.4), (5, 0.3, 0.5, 0.4), (8, 0.3, 0.5, 0.4), (3, 0.3, 0.0, 0.0), (3, 0.0, 0.5, 0.0), (3, 0.0, 0.0, 0.4),
           (3, 0.0, 0.0, 0.0), (2, 1e-6, 0.0, 0.0), (2, 1e15, 1e15, 1e15), (4, 0.05, 0.1, 0.02)]


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (64, 64), (257, 131)])
def test_edge_scene_texels_under_eleven_filters(lm, W, H):
    """257 x 131 is a multiple of no tile shape and has a ragged apron on every side; at 64 x 64 eight iterations reach the steps
    16 ... 128, beyond the atlas; each sigma alone, all together, none; a sigma so small that only taps at the texel's own position
    count; a very large one."""
    img, pts = edge_case(W, H)
    guided = FR.guides(pts, W, H)[0]
    for f in FILTERS:
        want = FR.run(img, pts, *f)
        got = lm.filter_lightmap(img, pts, *f)
        assert_image(got, want, f"{W} x {H}, filter {f}")
        if f[1] == 1e-6 and len(pts):
            assert np.allclose(want[guided][:, 0:3], img[guided][:, 0:3], rtol=1e-6, atol=0)      # c * w / w, two roundings an iteration
        if f == FILTERS[0] and W >= 64:
            assert (bits(want[guided][:, 0:3]) != bits(img[guided][:, 0:3])).any(axis=1).mean() > 0.5


_full = []


def full_case():
    if not _full:
        cs = LS.full_pair_scene()
        pts, _ = LR.texels(cs.triangles, cs.vertices, 1024, 1024)
        img = np.random.default_rng(1024).uniform(0.9, 1.1, (1024, 1024, 4)).astype(F)      # (noise small enough that the colour stop,
        #                                                         sixteen times as strong at the step 4, still lets that step's taps count)
        _full.append((img, pts, FR.run(img, pts, 3, 0.004, 0.5, 0.5, keep=True)))
    return _full[0]


def test_a_pair_over_all_of_1024_x_1024(lm):
    """Every texel guided, 4096 tiles a lattice.  The call has no "start at step s": one iteration is the step 1, three iterations add
    the steps 2 and 4 on top of it - each checked against the reference's image after that iteration, so a fault at the step 4
    cannot hide behind the steps before it.  Here in the default form of each step; test_each_form_alone_at_1024_x_1024 forces both."""
    img, pts, want = full_case()
    assert len(pts) == 1 << 20
    assert_image(lm.filter_lightmap(img, pts, 1, 0.004, 0.5, 0.5), want[0], "1024 x 1024, step 1")
    assert_image(lm.filter_lightmap(img, pts, 3, 0.004, 0.5, 0.5), want[2], "1024 x 1024, steps 1, 2, 4")
    assert (bits(want[2]) != bits(want[1])).any(axis=-1).mean() > 0.9


def test_each_form_alone_at_1024_x_1024(monkeypatch):
    """the same three iterations with every step in the direct form, then with every step in the LDS form"""
    img, pts, want = full_case()
    for step in ("0", "128"):
        monkeypatch.setenv("HJ_LIGHTMAP_FILTER_LDS_STEP", step)
        with device.Renderer(0) as r:
            r.upload_scene(LS.full_pair_scene())
            assert_image(r.filter_lightmap(img, pts, 3, 0.004, 0.5, 0.5), want[2], f"1024 x 1024, HJ_LIGHTMAP_FILTER_LDS_STEP={step}")


@pytest.mark.parametrize("step", ["0", "1", "128"])
def test_the_kernel_form_never_shows_in_a_result(monkeypatch, step):
    """Both forms forced by their switch at every step size (0: the direct form at every step, 128: the LDS form at every step, 1: the
    LDS form for the step 1 alone, the direct form above it): a context created under the setting returns the REFERENCE's bytes - computed on the host, so no
    switch can reach it - and so the forms agree with each other."""
    monkeypatch.setenv("HJ_LIGHTMAP_FILTER_LDS_STEP", step)
    with device.Renderer(0) as r:
        r.upload_scene(LS.edge_scene()[0])
        for (W, H), f in (((64, 64), FILTERS[3]), ((257, 131), FILTERS[3]), ((257, 131), FILTERS[10]), ((7, 5), FILTERS[2]), ((1, 1), FILTERS[1])):
            img, pts = edge_case(W, H)
            assert_image(r.filter_lightmap(img, pts, *f), FR.run(img, pts, *f), f"HJ_LIGHTMAP_FILTER_LDS_STEP={step}, {W} x {H}, filter {f}")


def test_two_charts_side_by_side_in_the_atlas_and_apart_in_space(lm):
    """Two charts that share the atlas column u = 0.5, one at height 0, one at height 5, sigma_position = 0.05: across the seam
    a >= 25 / 0.0025 = 10^4 and hj_exp(-a) = +0.  The result equals the reference; and it equals, bit for bit, the filter run on each
    chart's texels alone: a tap with w == +0 adds c * 0 = +0 to sums that are +0 or positive, and +0 to wsum - exact for the finite,
    positive colours used here."""
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    white = s.add_diffuse((0.6, 0.6, 0.6))
    LS._add_mesh(s, *LS._pair(0.125, 0.125, 0.5, 0.875, y=0.0), white)
    LS._add_mesh(s, *LS._pair(0.5, 0.125, 0.875, 0.875, y=5.0), white)
    cs = s.compile()
    W, H = 48, 32
    pts, owner = LR.texels(cs.triangles, cs.vertices, W, H)
    left = (owner.ravel()[pts.view(U)[:, 7]] < 2)
    x = pts.view(U)[:, 7] % W
    assert left.sum() > 300 and (~left).sum() > 300 and x[left].max() + 1 == x[~left].min()      # the charts touch in the atlas
    img = np.random.default_rng(7).uniform(0.1, 2.0, (H, W, 4)).astype(F)
    f = (4, 0.05, 0.5, 0.0)
    want = FR.run(img, pts, *f)
    got = lm.filter_lightmap(img, pts, *f)
    assert_image(got, want, "two charts")
    a, b = lm.filter_lightmap(img, pts[left], *f), lm.filter_lightmap(img, pts[~left], *f)
    G = FR.guides(pts[left], W, H)[0]
    assert_image(got, np.where(G[:, :, None], a, b), "each chart alone")
    bleeding = lm.filter_lightmap(img, pts, 4, 0.0, 0.5, 0.0)                                      # (without the stop they do bleed)
    seam = int(x[left].max())
    assert (bits(bleeding[:, seam]) != bits(got[:, seam])).any()


def test_host_arrays_device_tensors_and_the_texel_calls_own_tensor(lm):
    import torch
    W, H = 64, 64
    img, pts = edge_case(W, H)
    f = FILTERS[2]
    want = FR.run(img, pts, *f)
    dev = torch.device("cuda", 0)
    for iterations in (2, 5):                                           # an even and an odd number of swaps: the result is in `image`
        t_img, t_pts = torch.from_numpy(img.copy()).to(dev), torch.from_numpy(pts.copy()).to(dev)
        out = lm.filter_lightmap(t_img, t_pts, iterations, *f[1:], device=True)
        assert out is t_img and np.array_equal(bits(t_pts.cpu().numpy()), bits(pts))
        assert_image(t_img.cpu().numpy(), FR.run(img, pts, iterations, *f[1:]), f"device tensors, {iterations} iterations")
    own = lm.lightmap_texels(W, H, offset=1e-3, device=True)            # the texel call's tensor, fed unchanged
    assert np.array_equal(bits(own.cpu().numpy()), bits(pts))
    t_img = torch.from_numpy(img.copy()).to(dev)
    assert_image(lm.filter_lightmap(t_img, own, *f, device=True).cpu().numpy(), want, "lightmap_texels(device=True) as guides")
    none = torch.zeros((0, 8), device=dev)
    t_img = torch.from_numpy(img.copy()).to(dev)
    assert_image(lm.filter_lightmap(t_img, none, 3, 0.3, 0.5, device=True).cpu().numpy(), img, "no points: every texel copied")
    assert_image(lm.filter_lightmap(img, pts[:0], 3, 0.3, 0.5), img, "no points, host arrays")
    zero = lm.filter_lightmap(img, pts, 0, 0.3, 0.5)                    # no iterations: HJ_OK, nothing touched
    assert_image(zero, img, "0 iterations")
    nan = img.copy()                                                     # unguided texels are never read as taps; alpha is carried
    nan[~FR.guides(pts, W, H)[0]] = np.nan
    nan[:, :, 3] = np.arange(W * H, dtype=F).reshape(H, W)
    assert_image(lm.filter_lightmap(nan, pts, *f), FR.run(nan, pts, *f), "NaN in unguided texels, alpha of any value")


def test_a_device_point_that_names_no_texel_is_skipped(lm):
    """device arrays with an out-of-range word 7 (and, behind it, one that is merely out of order): no error, that texel is not
    guided, the rest equals the reference over the remaining points"""
    import torch
    W, H = 64, 64
    img, pts = edge_case(W, H)
    bad = pts.copy()
    k = len(bad) // 2
    bad.view(U)[k, 7] = W * H
    bad.view(U)[k + 1, 7] = 0xFFFFFFFF
    bad[[3, 9]] = bad[[9, 3]]                                            # (unsorted: the caller's business on this route)
    dev = torch.device("cuda", 0)
    t_img = torch.from_numpy(img.copy()).to(dev)
    got = lm.filter_lightmap(t_img, torch.from_numpy(bad).to(dev), *FILTERS[2], device=True).cpu().numpy()
    assert_image(got, FR.run(img, np.delete(pts, [k, k + 1], axis=0), *FILTERS[2]), "two points that name no texel")
    t = int(pts.view(U)[k, 7])
    assert np.array_equal(bits(got.reshape(-1, 4)[t]), bits(img.reshape(-1, 4)[t]))


W_B, H_B = 96, 80


@pytest.mark.parametrize("env", [False, True], ids=["cbox", "env"])
def test_filtered_bake_is_texels_gather_scatter_filter_dilate(lm, env):
    cs = LS.bake_scene(env)
    kw = dict(seed=11, seed_stride=7, offset=1e-3)
    f = (3,) + device.default_filter_sigmas(cs)[0:2] + (0.8,)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        for spp, gutter in ((1, 0), (1, 2), (5, 0), (5, 2)) if not env else ((5, 2), (1, 0)):
            pts = r.lightmap_texels(W_B, H_B, **kw)
            rec, want_stats = r.trace_irradiance(pts, spp=spp, opts=R.options(12), stats=True)
            want = FR.run(LR.scatter(pts, rec, W_B, H_B, spp), pts, *f)
            for _ in range(gutter):
                want = LR.dilate(want)
            got, stats = r.bake_lightmap(W_B, H_B, spp, gutter=gutter, opts=R.options(12), stats=True, filter=f, **kw)
            assert_image(got, want, f"env {env}, spp {spp}, gutter {gutter}")
            for k in want_stats:                                        # every field of the gather's record but the times
                assert k.endswith("_ms") or stats[k] == want_stats[k], (k, stats[k], want_stats[k])
            assert stats["texels"] == len(pts) and (got[:, :, 3] == 1).sum() == len(pts) and ((got[:, :, 3] == 0.5).sum() > 0) == (gutter > 0)
            raw = r.bake_lightmap(W_B, H_B, spp, gutter=gutter, opts=R.options(12), **kw)
            assert (bits(raw) != bits(got)).any()
        t = r.bake_lightmap(W_B, H_B, spp, gutter=gutter, opts=R.options(12), device=True, filter=f, **kw)
        assert t.is_cuda and np.array_equal(bits(t.cpu().numpy()), bits(got))
        odd = r.bake_lightmap(W_B, H_B, spp, gutter=1, opts=R.options(12), device=True, filter=f, **kw)      # 3 + 1 swaps
        assert np.array_equal(bits(odd.cpu().numpy()), bits(r.bake_lightmap(W_B, H_B, spp, gutter=1, opts=R.options(12), filter=f, **kw)))


def test_no_filter_is_the_unfiltered_bake(lm):
    """hj_bake_lightmap_filtered with NULL, and with a filter of 0 iterations, is hj_bake_lightmap: image, count and statistics (but
    the times)"""
    L = device.lib()
    with device.Renderer(0) as r:
        r.upload_scene(LS.bake_scene())
        d = abi.LightmapDesc(W_B, H_B, 0, 0, 11, 7, 1e-3, 0)
        o = R.options(12)
        results = []
        for f in ("plain", None, abi.LightmapFilter(0, 0.04, 0.5, 0.3, 0)):
            img, count, st = np.full((H_B, W_B, 4), 7.0, F), C.c_size_t(0), abi.RenderStats()
            if f == "plain":
                rc = L.hj_bake_lightmap(r._h, C.byref(d), 5, 2, C.byref(o), img.ctypes.data, C.byref(count), C.byref(st))
            else:
                rc = L.hj_bake_lightmap_filtered(r._h, C.byref(d), 5, 2, C.byref(f) if f is not None else None, C.byref(o), img.ctypes.data,
                                                 C.byref(count), C.byref(st))
            assert rc == abi.HJ_OK, L.hj_last_error(r._h)
            results.append((img, count.value, {k: v for k, v in device.stats_dict(st).items() if not k.endswith("_ms")}))
        for img, count, st in results[1:]:
            assert np.array_equal(bits(img), bits(results[0][0])) and count == results[0][1] > 1500 and st == results[0][2]
        assert results[0][2]["paths"] == 5 * results[0][1]


def test_refusals_on_the_device_route_write_nothing(lm):
    import torch
    L = device.lib()
    dev = torch.device("cuda", 0)
    W, H = 64, 64
    img0, pts0 = edge_case(W, H)
    img, pts = torch.full((H, W, 4), 7.0, device=dev), torch.from_numpy(pts0.copy()).to(dev)
    torch.cuda.synchronize(dev)
    DEV = abi.LIGHTMAP_DEVICE_ARRAYS
    n = len(pts0)
    for f, w, h, cnt in ((abi.LightmapFilter(9, 0.1, 0.5, 0.0, DEV), W, H, n), (abi.LightmapFilter(2, -0.1, 0.5, 0.0, DEV), W, H, n),
                         (abi.LightmapFilter(2, 0.1, float("nan"), 0.0, DEV), W, H, n), (abi.LightmapFilter(2, 0.1, 0.5, float("inf"), DEV), W, H, n),
                         (abi.LightmapFilter(2, 0.1, 0.5, 0.0, DEV | 4), W, H, n), (abi.LightmapFilter(2, 0.1, 0.5, 0.0, DEV), 0, H, n),
                         (abi.LightmapFilter(2, 0.1, 0.5, 0.0, DEV), W, 16385, n), (abi.LightmapFilter(2, 0.1, 0.5, 0.0, DEV), 8, 8, n)):
        assert L.hj_filter_lightmap(lm._h, w, h, pts.data_ptr(), cnt, C.byref(f), img.data_ptr()) == abi.HJ_ERR_INVALID
        assert b"hj_filter_lightmap" in L.hj_last_error(lm._h)
    ok = abi.LightmapFilter(2, 0.1, 0.5, 0.0, DEV)
    assert L.hj_filter_lightmap(lm._h, W, H, pts.data_ptr() + 4, n - 1, C.byref(ok), img.data_ptr()) == abi.HJ_ERR_INVALID
    assert L.hj_filter_lightmap(lm._h, W, H, pts.data_ptr(), n, C.byref(ok), img.data_ptr() + 8) == abi.HJ_ERR_INVALID
    assert L.hj_filter_lightmap(lm._h, W, H, None, n, C.byref(ok), img.data_ptr()) == abi.HJ_ERR_INVALID
    host_img = np.full((H, W, 4), 7.0, F)                                # host arrays: the indices and the values are checked
    unsorted = pts0.copy()
    unsorted[[3, 9]] = unsorted[[9, 3]]
    nan = pts0.copy()
    nan[5, 4] = np.nan
    for p in (unsorted, nan):
        with pytest.raises(abi.HijikiError) as e:
            lm.filter_lightmap(host_img, p, 2, 0.1, 0.5)
        assert e.value.status == abi.HJ_ERR_INVALID
    d = abi.LightmapDesc(W, H, 0, 0, 0, 1, 0.0, DEV)
    count, st = C.c_size_t(77), abi.RenderStats()
    nine = abi.LightmapFilter(9, 0.1, 0.5, 0.0, 0)
    assert L.hj_bake_lightmap_filtered(lm._h, C.byref(d), 4, 2, C.byref(nine), None, img.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_INVALID
    assert b"hj_bake_lightmap_filtered" in L.hj_last_error(lm._h)
    with device.Renderer(0) as r:                                       # no scene yet
        assert L.hj_filter_lightmap(r._h, W, H, pts.data_ptr(), n, C.byref(ok), img.data_ptr()) == abi.HJ_ERR_STATE
        assert b"scene" in L.hj_last_error(r._h)
        assert L.hj_bake_lightmap_filtered(r._h, C.byref(d), 4, 2, C.byref(ok), None, img.data_ptr(), C.byref(count), C.byref(st)) == abi.HJ_ERR_STATE
    torch.cuda.synchronize(dev)
    assert bool((img == 7.0).all()) and (host_img == 7.0).all() and count.value == 77
    assert np.array_equal(bits(pts.cpu().numpy()), bits(pts0)) and not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


def test_cli_filters_like_the_library(tmp_path):
    """--filter N alone takes the default sigmas (1 % of the root box's diagonal, 0.5, colour off); all four values are passed on as given"""
    import texture_scenes as ts
    obj = ts.write_obj_files(tmp_path, np.full((2, 2, 3), 0.5, F))
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    cs = host.Scene.from_obj(obj).compile()
    head = b"PF\n48 40\n-1.0\n"
    with device.Renderer(0) as rr:
        rr.upload_scene(cs)
        for arg, f in (("3", (3,) + device.default_filter_sigmas(cs)), ("2,0.25,0.75,0.5", (2, 0.25, 0.75, 0.5))):
            out = str(tmp_path / "atlas.pfm")
            r = subprocess.run([exe, "--bake-lightmap", "48x40", "--gutter", "1", "--filter", arg, "-s", "4", "--seed", "6", "-o", out, obj],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "Filter: " in r.stdout, r.stderr
            got = np.frombuffer(open(out, "rb").read(), F, offset=len(head)).reshape(40, 48, 3)[::-1]
            want = rr.bake_lightmap(48, 40, 4, gutter=1, seed=6, seed_stride=1, offset=1e-3, filter=f)
            assert np.array_equal(bits(got), bits(want[:, :, 0:3])), arg
            assert (bits(want) != bits(rr.bake_lightmap(48, 40, 4, gutter=1, seed=6, seed_stride=1, offset=1e-3))).any()


def test_it_denoises(lm):
    """A property, not a parity check: the bake scene at 64 x 64, 4 samples a texel, filtered with 3 iterations and the command line's
    default sigmas (1 % of the root box's diagonal, 0.5, colour stop off), is strictly closer in RMSE over the owned texels to a
    4096-sample bake than the unfiltered 4-sample bake is.  No ratio is fixed; it is printed (DESIGN.md quotes a run's)."""
    cs = LS.bake_scene()
    sig = device.default_filter_sigmas(cs)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        kw = dict(gutter=0, offset=1e-3, opts=R.options(12))
        truth = r.bake_lightmap(64, 64, 4096, seed=1, seed_stride=4096, **kw)
        raw = r.bake_lightmap(64, 64, 4, seed=1 << 30, seed_stride=4, **kw)
        flt = r.bake_lightmap(64, 64, 4, seed=1 << 30, seed_stride=4, filter=(3,) + sig, **kw)
    owned = truth[:, :, 3] == 1
    assert owned.sum() > 1000 and np.array_equal(owned, raw[:, :, 3] == 1) and np.array_equal(bits(flt[~owned]), bits(raw[~owned]))
    rmse = lambda a: float(np.sqrt(np.mean((a[owned][:, 0:3].astype(np.float64) - truth[owned][:, 0:3]) ** 2)))  # noqa: E731
    e_raw, e_flt = rmse(raw), rmse(flt)
    print(f"sigmas {sig}: RMSE against 4096 spp: unfiltered {e_raw:.5f}, filtered {e_flt:.5f}, ratio {e_flt / e_raw:.3f}")
    assert e_flt < e_raw
