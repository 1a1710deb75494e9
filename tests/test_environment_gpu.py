"""Environment lighting on the MI355X: the lookup and sampling probes against their numpy restatements, an environment-only frame
bit for bit against the oracle's camera rays and reconstruction, black environments through the environment kernels bit for bit
against the unchanged oracle, an analytic sky, linearity of area and environment light, and route consistency."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import env_scenes as es
from hijiki_amd import abi, device, host

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def opts(flags=0):
    o = device.default_opts()
    o.flags = flags
    return o


def test_lookup_probe_is_bit_exact(gpu_renderer, oracle):
    rng = np.random.default_rng(21)
    v = [0.0, -0.0, 1.0, -1.0, 2.5, -3e-20, 1e-30]
    grid = np.array(np.meshgrid(v, v, v)).reshape(3, -1).T
    rand = rng.normal(size=(30000, 3)) * rng.uniform(1e-3, 1e3, (30000, 1))
    extra = [[0, 1, 0], [0, -1, 0], [0, 7, 1e-7], [0, -7, -1e-7], [1e-8, 1, 0], [np.inf, 0, 1], [np.nan, 1, 0]]
    dirs = np.concatenate([grid, rand, extra]).astype(F)
    r = gpu_renderer
    for filt, (H, W) in ((abi.TEX_NEAREST, (32, 64)), (abi.TEX_BILINEAR, (9, 13)), (abi.TEX_BILINEAR, (1, 5))):
        tex = es.random_env(rng, H, W)
        scale = (0.5, 2.0, 1.25)
        cs = es.env_only_scene(tex, filt, scale).compile()
        r.upload_scene(cs)
        got = r.env_lookup(dirs)
        want = es.lookup(oracle, cs.texture_set, cs.environment.texture, scale, dirs)
        bad = (bits(got) != bits(want)).any(axis=1)
        assert not bad.any(), f"{W} x {H}, filter {filt}: {int(bad.sum())} lookups differ, first {dirs[bad][0]}"


def test_sample_probe(gpu_renderer):
    rng = np.random.default_rng(5)
    r = gpu_renderer
    n = 1 << 20
    for filt, (H, W) in ((abi.TEX_NEAREST, (32, 64)), (abi.TEX_BILINEAR, (9, 13))):
        tex = es.random_env(rng, H, W)
        scale = (1.0, 0.5, 2.0)
        cs = es.env_only_scene(tex, filt, scale).compile()
        r.upload_scene(cs)
        out = r.env_sample(rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        d, pdf, cell, w = out[:, :3], out[:, 3], out[:, 4].astype(np.int64), out[:, 5:]
        np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-5)
        # every direction lies inside its texel (float64 angles; a hair of slack for the float32 direction)
        x, y = cell % W, cell // W
        dd = d.astype(np.float64)
        u = (0.5 + np.arctan2(dd[:, 2], dd[:, 0]) / (2 * np.pi)) * W
        q = (0.5 - np.arctan2(dd[:, 1], np.hypot(dd[:, 0], dd[:, 2])) / np.pi) * H
        u = np.where(u - x > W / 2, u - W, np.where(x - u > W / 2, u + W, u))       # (phi wraps at u = 0 = 1)
        assert ((u >= x - 1e-4) & (u <= x + 1 + 1e-4)).all() and ((q >= y - 1e-4) & (q <= y + 1 + 1e-4)).all()
        wgt = es.weights(tex, scale, filt)
        P = (wgt / wgt.sum()).ravel()
        np.testing.assert_allclose(pdf, (P / es.solid_angles(H, W).ravel())[cell], rtol=1e-6)
        counts = np.bincount(cell, minlength=H * W)
        assert counts[P == 0].sum() == 0
        e = n * P[P > 0]
        chi2 = float((((counts[P > 0] - e) ** 2) / e).sum())
        assert stats.chi2.sf(chi2, len(e) - 1) > 1e-4, (W, H, filt, chi2, len(e))
        le = r.env_lookup(d)
        assert (bits(w) == bits(le * (F(1.0) / pdf)[:, None])).all()


def test_refusals_and_state(gpu_renderer):
    r = gpu_renderer
    L = device.lib()
    tex = es.sky_texels(8, 16)
    lit = host.Scene.synthetic(host.SYNTH_CBOX)
    t = lit.add_texture(tex)
    cs = lit.compile()
    dark = es.env_only_scene(np.zeros((4, 4, 4), F)).compile()

    def refused(c, e):
        rc = L.hj_scene_upload_env(r._h, C.byref(c.desc), C.byref(c.texture_set), C.byref(e))
        assert rc == abi.HJ_ERR_INVALID and b"environment" in L.hj_last_error(r._h)
        # (refused before anything happens: the scene before it - without an environment - stays)
        assert L.hj_debug_env_lookup(r._h, (C.c_float * 3)(0, 1, 0), 1, (C.c_float * 3)()) == abi.HJ_ERR_STATE

    r.upload_scene(cs)                                                                   # no environment
    assert L.hj_debug_env_sample(r._h, (C.c_uint32 * 1)(7), 1, (C.c_float * 8)()) == abi.HJ_ERR_STATE
    refused(cs, host.environment(cs, t + 1, select_prob=0.5))
    refused(cs, host.environment(cs, t, (1.0, -2.0, 1.0), select_prob=0.5))
    refused(cs, host.environment(cs, t, select_prob=1.25))
    refused(dark, host.environment(dark, dark.environment.texture, select_prob=0.5))     # no emitters: must be 1
    refused(dark, host.environment(dark, dark.environment.texture, select_prob=1.0))     # black, but sampled
    r.upload_scene(cs, environment=host.environment(cs, t, (0.0, 0.0, 0.0)))             # black, never sampled: fine
    assert (r.env_lookup([[0, 1, 0]]) == 0).all()


def test_environment_only_frame_is_bit_exact(gpu_renderer, oracle):
    """Every camera ray misses: each sample is Le(d) of its camera ray, so the frame is the oracle's reconstruction of the
    lookup restatement at the oracle's camera rays."""
    rng = np.random.default_rng(8)
    r = gpu_renderer
    W, H, spp, seed = 160, 96, 2, 3
    for filt in (abi.TEX_NEAREST, abi.TEX_BILINEAR):
        tex = es.random_env(rng, 17, 33)
        cs = es.env_only_scene(tex, filt, (1.5, 1.0, 0.5)).compile()
        for flags in (0, abi.RENDER_SPLIT_KERNELS):
            r.upload_scene(cs)
            r.create_framebuffer(W, H)
            st = r.render_frame(spp, seed, opts=opts(flags))
            got = r.read()
            assert st["hits"] == 0 and st["shadow_rays"] == 0 and st["closest_rays"] == st["paths"] == W * H * spp
            accum = np.zeros((H, W, 4), F)
            o = opts(flags)
            for b in host.make_blocks(W, H, spp, seed):
                dx, dy = b.dimension[0], b.dimension[1]
                lx, ly = np.meshgrid(np.arange(dx), np.arange(dy))
                pix = np.stack([(lx + b.origin[0]).astype(F) + F(b.sample_offset[0]),
                                (ly + b.origin[1]).astype(F) + F(b.sample_offset[1])], -1).reshape(-1, 2)
                rays = oracle.camera_rays(cs.desc.camera, b.original_dimension[0], b.original_dimension[1], pix)
                smp = np.zeros((dy * dx, 8), F)
                smp[:, :3] = es.lookup(oracle, cs.texture_set, cs.environment.texture, (1.5, 1.0, 0.5), rays[:, 3:])
                smp[:, 3] = 1.0
                oracle.reconstruct_block(b, smp.reshape(dy, dx, 8), accum, o)
            bad = (bits(got) != bits(accum)).any(axis=-1)
            assert not bad.any(), f"filter {filt}, flags {flags}: {int(bad.sum())} pixels differ"


BLACK_ROUTES = ("default", "split-kernels", "no-light-grid", "resident-tree")


def render_route(r, cs, route, W, H, spp, seed):
    o = opts({"split-kernels": abi.RENDER_SPLIT_KERNELS, "no-light-grid": abi.RENDER_NO_LIGHT_GRID}.get(route, 0))
    on_device = route == "resident-tree"
    if on_device:                                     # hj_scene_upload_env takes the tree over; the oracle walks its copy
        r.build_bvh(cs, keep_on_device=True)
        cs.set_bvh(r.read_device_bvh())
    r.upload_scene(cs, device_tree=on_device)
    r.create_framebuffer(W, H)
    st = r.render_frame(spp, seed, opts=o)
    return r.read().copy(), st, o


@pytest.mark.parametrize("route", BLACK_ROUTES)
def test_black_environment_is_the_plain_render(gpu_renderer, oracle, route):
    """A black environment (select_prob 0) goes through the environment kernels - miss bin, remapped emitter choice - and must
    change no bit: frames and counters are the unchanged oracle's render of the scene without it."""
    W, H, spp, seed = 96, 64, 3, 5
    for kind in (host.SYNTH_CBOX, host.SYNTH_CBOX_SPHERES):
        s = host.Scene.synthetic(kind)
        s.set_environment(s.add_texture(np.zeros((6, 10, 4), F), abi.TEX_BILINEAR))
        cs = s.compile()
        assert cs.environment is not None and cs.environment.select_prob == 0.0
        got, st, o = render_route(gpu_renderer, cs, route, W, H, spp, seed)
        want, ctr, _ = oracle.render_blocks(cs, host.make_blocks(W, H, spp, seed), W, H, opts=o)
        bad = (bits(got) != bits(want)).any(axis=-1)
        assert not bad.any(), f"{kind}, {route}: {int(bad.sum())} pixels differ from the oracle"
        assert (st["closest_rays"], st["shadow_rays"], st["hits"], st["paths"]) == \
            (ctr["closest_calls"], ctr["shadow_calls"], ctr["hits"], ctr["paths"])


def sample_stats(r, W, H, spp, seed):
    """Mean and standard error per channel of every path sample of a W x H x spp frame (hj_debug_samples, block by block)."""
    vals = [r.samples(b, opts())[..., :3].reshape(-1, 3).astype(np.float64) for b in host.make_blocks(W, H, spp, seed)]
    v = np.concatenate(vals)
    return v.mean(0), v.std(0) / np.sqrt(len(v))


def test_analytic_sky(gpu_renderer):
    """An upward diffuse quad of albedo rho filling a downward camera's frame under a nearest 64 x 32 sky with a sun texel: every
    pixel's expectation is rho / pi * sum over the upper cells of L * dphi * (y1^2 - y0^2) / 2."""
    H, W = 32, 64
    tex = es.sky_texels(H, W)
    rho = np.array([0.5, 0.6, 0.7])
    s = host.Scene()
    s.set_camera((0.0, 1.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)     # looking down -y
    s.add_quad((-5.0, 0.0, -5.0), (0.0, 0.0, 10.0), (10.0, 0.0, 0.0), s.add_diffuse(tuple(rho)))   # edge1 x edge2 = +y
    s.add_sphere((0.0, -50.0, 0.0), 0.1, s.add_diffuse((0.5, 0.5, 0.5)))
    s.set_environment(s.add_texture(tex, abi.TEX_NEAREST))
    cs = s.compile()
    assert cs.environment.select_prob == 1.0
    y = np.sin(np.pi * (0.5 - np.arange(H + 1) / H))                               # sin(latitude) of the row edges
    cosw = (2 * np.pi / W) * (y[:-1] ** 2 - y[1:] ** 2) / 2                          # integral of cos over a cell, per row
    up = np.arange(H) < H // 2
    expect = rho / np.pi * (tex[up, :, :3].astype(np.float64) * cosw[up, None, None]).sum((0, 1))
    r = gpu_renderer
    r.upload_scene(cs)
    Wf, Hf, spp, seed = 128, 128, 32, 9
    mean, se = sample_stats(r, Wf, Hf, spp, seed)
    assert (np.abs(mean - expect) < 4 * se).all(), (mean, expect, se)
    r.create_framebuffer(Wf, Hf)
    r.render_frame(spp, seed)
    fmean = r.resolve().reshape(-1, 3).astype(np.float64).mean(0)
    assert (np.abs(fmean - expect) < 4 * se).all(), (fmean, expect, se)


def light_and_env_scene(power, env=True, select_prob=None):
    s = host.Scene()
    s.set_camera((0.0, 1.0, 1.2), (-0.38268343, 0.0, 0.0, 0.92387953), 50.0)       # 45 degrees down
    s.add_quad((-3.0, 0.0, -3.0), (0.0, 0.0, 6.0), (6.0, 0.0, 0.0), s.add_diffuse((0.6, 0.5, 0.4)))
    s.add_quad((-0.3, 1.5, -0.3), (0.6, 0.0, 0.0), (0.0, 0.0, 0.6), s.add_emissive((power, power * 0.9, power * 0.8)))   # faces down
    s.add_sphere((0.4, 0.3, -0.2), 0.3, s.add_diffuse((0.3, 0.6, 0.3)))
    if env:
        s.set_environment(s.add_texture(es.sky_texels(16, 32), abi.TEX_BILINEAR), 0.5, select_prob)
    return s.compile()


def test_area_light_plus_environment_is_linear(gpu_renderer):
    r = gpu_renderer
    W, H, spp, seed = 128, 128, 48, 12
    res = {}
    for name, cs in (("both", light_and_env_scene(8.0, select_prob=0.5)), ("light", light_and_env_scene(8.0, env=False)),
                     ("env", light_and_env_scene(0.0))):
        r.upload_scene(cs)
        res[name] = sample_stats(r, W, H, spp, seed + len(res))
    diff = res["both"][0] - (res["light"][0] + res["env"][0])
    se = np.sqrt(res["both"][1] ** 2 + res["light"][1] ** 2 + res["env"][1] ** 2)
    assert (np.abs(diff) < 4 * se).all(), (res, diff, se)
    assert (res["env"][0] > 20 * res["env"][1]).all()                # (the environment's share is not nothing)


def mixed_scene():
    """cbox with its mirror and glass spheres, diffuse walls and area light, a textured quad, under a bilinear sky (select_prob 0.5)."""
    s = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES)
    rng = np.random.default_rng(2)
    m = s.add_diffuse_textured(s.add_texture(rng.uniform(0.1, 0.9, (5, 7, 4)).astype(F), abi.TEX_BILINEAR))
    s.add_quad((-0.6, 0.2, 0.4), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0), m)
    s.set_environment(s.add_texture(es.sky_texels(16, 32), abi.TEX_BILINEAR), 2.0)
    return s.compile()


def test_routes_agree_under_an_environment(gpu_renderer):
    r = gpu_renderer
    W, H, spp, seed = 160, 96, 4, 7
    cs = mixed_scene()
    assert cs.environment.select_prob == 0.5
    ref, st_ref, _ = render_route(r, cs, "default", W, H, spp, seed)
    for route in ("split-kernels", "no-light-grid"):
        got, st, _ = render_route(r, cs, route, W, H, spp, seed)
        assert (bits(got) == bits(ref)).all(), route
        assert (st["closest_rays"], st["hits"], st["paths"]) == (st_ref["closest_rays"], st_ref["hits"], st_ref["paths"]), route
    # resident tree: the same tree through the host gives the same bits
    res = mixed_scene()
    got, st, _ = render_route(r, res, "resident-tree", W, H, spp, seed)
    same_tree = mixed_scene()
    same_tree.set_bvh(res.bvh)
    want, _, _ = render_route(r, same_tree, "default", W, H, spp, seed)
    assert (bits(got) == bits(want)).all()
    assert (got[..., :3] > 0).any()


def test_tile_sharding_under_an_environment(gpu_renderer):
    r = gpu_renderer
    W, H, spp, seed = 288, 160, 3, 4
    cs = mixed_scene()
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    st_full = r.render_frame(spp, seed)
    full = r.read().copy()
    parts, paths = [], 0
    for rank in range(3):
        r.clear()
        st = r.render_frame(spp, seed, rank=rank, world=3)
        paths += st["paths"]
        parts.append(r.read().astype(np.float64))
    assert paths == st_full["paths"]
    np.testing.assert_allclose(np.sum(parts, axis=0), full, rtol=3e-6, atol=1e-6)
