"""Environment lighting on the MI355X: the lookup and sampling probes against their numpy restatements and the oracle's, an
environment-only frame bit for bit against the oracle's camera rays and reconstruction, black environments through the environment
kernels bit for bit against the oracle, environment-LIT frames bit for bit against the oracle on every route of the renderer (in
tile shards, with bounce limits, small batches, a refitted tree; every ray of one replayed), an analytic sky, linearity of area and
environment light, and route consistency."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import env_scenes as es
import fuzz_cases
from hijiki_amd import abi, device, host
from refit_scenes import Deformation

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
    tex = es.sky_texels(32, 64)
    cs = es.analytic_sky_scene(tex)                     # (scene and closed form shared with tests/test_environment_oracle.py)
    assert cs.environment.select_prob == 1.0
    expect = es.analytic_sky_expectation(tex)
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


mixed_scene = es.mixed_scene      # (shared with tests/test_environment_oracle.py)


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


def test_tile_sharding_under_an_environment(gpu_renderer, oracle):
    """Each rank's share of a lit frame is the oracle's render of that rank's blocks, and the shares sum to the 1-GPU frame."""
    r = gpu_renderer
    W, H, spp, seed = 288, 160, 3, 4
    cs = mixed_scene()
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    st_full = r.render_frame(spp, seed)
    full = r.read().copy()
    assert_oracle_frame(oracle, cs, full, st_full, opts(), W, H, spp, seed, "full frame")
    L = host.lib()
    blocks = host.make_blocks(W, H, spp, seed)
    per = host.blocks_per_pass(W, H)
    parts, paths = [], 0
    for rank in range(3):
        r.clear()
        st = r.render_frame(spp, seed, rank=rank, world=3)
        paths += st["paths"]
        mine = [b for k, b in enumerate(blocks) if L.hj_block_owner(W, H, k // per, k % per, 3) == rank]
        assert_oracle_frame(oracle, cs, r.read().copy(), st, opts(), W, H, spp, seed, f"rank {rank} of 3",
                            blocks=(abi.ImageBlock * len(mine))(*mine))
        parts.append(r.read().astype(np.float64))
    assert paths == st_full["paths"]
    np.testing.assert_allclose(np.sum(parts, axis=0), full, rtol=3e-6, atol=1e-6)


# ------------------------------------------------------------------ environment-lit frames against the oracle, bit for bit

def test_sample_probe_is_the_oracles(gpu_renderer, oracle):
    """hj_debug_env_sample == hjo_env_sample bit for bit: random states, states whose coin equals their column's threshold, and
    the ends of both draws (tests/test_environment_oracle.py pins the oracle's to the numpy restatement of DESIGN.md)."""
    rng = np.random.default_rng(5)
    r = gpu_renderer
    for filt, (H, W) in ((abi.TEX_NEAREST, (32, 64)), (abi.TEX_BILINEAR, (9, 13)), (abi.TEX_BILINEAR, (1, 7)), (abi.TEX_NEAREST, (5, 1)),
                         (abi.TEX_BILINEAR, (1, 1))):
        cs = es.env_only_scene(es.random_env(rng, H, W), filt, (1.0, 0.5, 2.0)).compile()
        table = oracle.env_table(cs.texture_set, cs.environment)
        thr = es.threshold_states(table, W, H)
        assert H * W <= 16 or len(thr) >= 1
        ends = [es.states_with_draws(second=0xFFFFFFFF), es.states_with_draws(second=1), es.states_with_draws(third=0xFFFFFFFF),
                es.states_with_draws(third=1), es.states_with_draws(first=0xFFFFFFFF), es.states_with_draws(first=1)]
        states = np.concatenate([rng.integers(1, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32), thr, np.array(ends, np.uint32)])
        r.upload_scene(cs)
        got = r.env_sample(states)
        want = oracle.env_sample(cs, states)
        bad = (bits(got) != bits(want)).any(axis=1)
        assert not bad.any(), f"{W} x {H}, filter {filt}: {int(bad.sum())} samples differ, first state {states[bad][0]}: {got[bad][0]} {want[bad][0]}"


ROUTES = ("default", "split-kernels", "no-light-grid", "linear-scan", "device-re-layout", "device-built-tree", "resident-tree")


def render_on(r, cs, route, W, H, spp, seed, monkeypatch, o=None):
    """cs on one route of the renderer (tests/test_textures_gpu.py render_route) -> (frame, stats, the oracle's RenderOpts)."""
    o = opts() if o is None else o
    o.flags = {"split-kernels": abi.RENDER_SPLIT_KERNELS, "no-light-grid": abi.RENDER_NO_LIGHT_GRID}.get(route, 0)
    if route == "linear-scan":
        o.use_bvh = 0
    if route == "device-re-layout":
        monkeypatch.setenv("HJ_UPLOAD_DEVICE", "1")
    else:
        monkeypatch.delenv("HJ_UPLOAD_DEVICE", raising=False)
    on_device = False
    if route == "device-built-tree":
        cs.set_bvh(r.build_bvh(cs))
    elif route == "resident-tree":
        r.build_bvh(cs, keep_on_device=True)
        cs.set_bvh(r.read_device_bvh())
        on_device = True
    r.upload_scene(cs, device_tree=on_device)
    r.create_framebuffer(W, H)
    st = r.render_frame(spp, seed, opts=o)
    return r.read().copy(), st, o


def assert_oracle_frame(oracle, cs, got, st, o, W, H, spp, seed, what, blocks=None):
    blocks = host.make_blocks(W, H, spp, seed) if blocks is None else blocks
    want, ctr, _ = oracle.render_blocks(cs, blocks, W, H, opts=o)
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ from the oracle"
    assert (st["closest_rays"], st["shadow_rays"], st["hits"], st["paths"]) == \
        (ctr["closest_calls"], ctr["shadow_calls"], ctr["hits"], ctr["paths"]), what
    return ctr


def single_texel(H=6, W=9):
    """Nearest, one non-zero texel: almost every column of the alias table is an alias of it."""
    t = np.zeros((H, W, 4), F)
    t[1, 4, :3] = (30.0, 25.0, 20.0)
    return t


def half_dark(H=8, W=12):
    """A sky whose right half (and the lower rows) weighs nothing."""
    t = es.sky_texels(H, W, sun=(1, 2))
    t[:, W // 2:, :3] = 0.0
    return t


def lit_scenes():
    """name -> (compiled scene, premises its ray log must show).  Small enough that the oracle takes seconds."""
    one = np.full((1, 1, 4), 1.25, F)
    row = es.sky_texels(1, 7, sun=(0, 2), sun_rgb=(6.0, 5.0, 4.0)) + F(0.5)
    colm = es.sky_texels(5, 1, sun=(1, 0), sun_rgb=(6.0, 5.0, 4.0))
    return {
        "mixed": (es.mixed_scene(), ("area", "discrete")),
        "tinted glass, open scene": (es.mixed_scene(tinted=True), ("area", "discrete", "tinted", "camera")),
        "analytic sky, no emitters": (es.analytic_sky_scene(es.sky_texels(32, 64)), ("no-area",)),
        "sphere cluster, no emitters": (es.cluster_scene(), ("no-area", "discrete", "camera")),
        "random 1, select_prob 0.125": (es.random_scene_with_env(1, 0.125), ("area", "discrete")),
        "random 2, select_prob 0.875": (es.random_scene_with_env(2, 0.875, abi.TEX_NEAREST), ("area", "discrete")),
        "1 x 1": (es.cluster_scene(one, abi.TEX_BILINEAR, light=True), ("area", "discrete", "camera")),
        "1 x 7": (es.cluster_scene(row, abi.TEX_BILINEAR, (1.0, 0.5, 2.0), light=True), ("area", "discrete", "camera")),
        "5 x 1": (es.cluster_scene(colm, abi.TEX_NEAREST, light=True), ("area", "discrete", "camera")),
        "one bright texel": (es.cluster_scene(single_texel(), abi.TEX_NEAREST), ("no-area", "discrete", "camera")),
        "half of the sky dark": (es.cluster_scene(half_dark(), abi.TEX_BILINEAR, select_prob=0.75, light=True), ("area", "discrete", "camera")),
    }


def assert_premises(oracle, cs, name, want, W, H, seed, o=None):
    """The frame exercises what it claims to: from the oracle's ray log of its first pass."""
    p = es.ray_log_premises(cs, oracle.logged_rays(cs, host.make_blocks(W, H, 1, seed), o))
    assert p["env_shadow"] > 50 and p["env_shadow_free"] > 20, (name, p)
    if "area" in want:
        assert p["area_shadow"] > 50, (name, p)
    if "no-area" in want:
        assert p["area_shadow"] == 0, (name, p)
    if "discrete" in want:
        assert p["discrete_misses"] > 10, (name, p)
    if "camera" in want:
        assert p["camera_misses"] > 50, (name, p)
    if "tinted" in want:
        assert p["tinted_misses"] > 20, (name, p)
    return p


@pytest.mark.parametrize("route", ROUTES)
def test_lit_frames_match_the_oracle(gpu_renderer, oracle, monkeypatch, route):
    """Frames an environment lights - next-event samples of it and of area emitters, misses after camera, mirror and glass rays,
    tinted glass, no emitters, tiny and mostly-dark environments - bit for bit against the oracle, counters included, on every
    route of the renderer."""
    linear = route == "linear-scan"
    W, H, spp = (64, 40, 2) if linear else (160, 96, 3)
    for k, (name, (cs, want)) in enumerate(lit_scenes().items()):
        seed = 20 + k
        if route == "default":
            assert_premises(oracle, cs, name, want, W, H, seed)
        got, st, o = render_on(gpu_renderer, cs, route, W, H, spp, seed, monkeypatch)
        assert_oracle_frame(oracle, cs, got, st, o, W, H, spp, seed, f"{name}, {route}")
        assert (got[..., :3] > 0).any()


@pytest.mark.parametrize("max_bounces,rr_start", [(1, 4), (2, 4), (2, 0), (6, 0), (1000, 0)])
def test_bounce_limits_and_early_roulette(gpu_renderer, oracle, monkeypatch, max_bounces, rr_start):
    """max_bounces 1 and 2 (a miss at bounce 0 and 1 is all the environment adds besides next-event samples) and roulette from
    bounce 0 (T is divided by q before the miss reads it)."""
    W, H, spp, seed = 160, 96, 3, 31
    for name, cs in (("mixed", es.mixed_scene()), ("tinted", es.mixed_scene(tinted=True)), ("cluster", es.cluster_scene())):
        o = opts()
        o.max_bounces, o.rr_start = max_bounces, rr_start
        got, st, o = render_on(gpu_renderer, cs, "default", W, H, spp, seed, monkeypatch, o)
        ctr = assert_oracle_frame(oracle, cs, got, st, o, W, H, spp, seed, f"{name}, {max_bounces} bounces, roulette from {rr_start}")
        if max_bounces == 1:
            assert ctr["closest_calls"] == ctr["paths"]
        if name != "mixed":                               # (camera rays leave these scenes: bounce-0 misses)
            assert ctr["hits"] < ctr["closest_calls"]


@pytest.mark.parametrize("batch_blocks", [1, 5])
def test_ragged_image_in_small_batches(gpu_renderer, oracle, monkeypatch, batch_blocks):
    """An image that is no multiple of the block size, rendered one and five ImageBlocks per batch: regenerated camera paths
    miss in the same round as stored ones."""
    W, H, spp, seed = 200, 150, 3, 41
    for name, cs in (("tinted", es.mixed_scene(tinted=True)), ("cluster", es.cluster_scene(light=True))):
        o = opts()
        o.batch_blocks = batch_blocks
        got, st, o = render_on(gpu_renderer, cs, "default", W, H, spp, seed, monkeypatch, o)
        assert_oracle_frame(oracle, cs, got, st, o, W, H, spp, seed, f"{name}, {batch_blocks} blocks per batch")


def test_every_ray_of_a_lit_frame(gpu_renderer, oracle):
    """oracle.logged_rays of one lit frame - the environment's shadow rays with tMax = inf among them - through hj_debug_trace:
    the same shape, the same t bits, the same any-hit answer."""
    cs = es.mixed_scene(tinted=True)
    blocks = host.make_blocks(160, 96, 1, 7)
    log = oracle.logged_rays(cs, blocks)
    env_rays = (log[:, 8] == 1) & (log[:, 10] == 8)
    assert env_rays.sum() > 1000 and np.isinf(log[env_rays, 7]).all() and (log[env_rays, 9] < 0).any() and (log[env_rays, 9] >= 0).any()
    n, bad = fuzz_cases.replay_scene(gpu_renderer, cs, blocks)
    assert n == len(log) and bad == 0, (n, bad)


def test_refit_under_an_environment(gpu_renderer, oracle):
    """hj_refit_bvh_device for a deformed scene under an environment: the frame on the refitted tree (left on the device) is the
    oracle's on the read-back copy."""
    r = gpu_renderer
    cs = es.mixed_scene(tinted=True)
    topo = r.build_bvh(cs)
    d = Deformation(cs, seed=3)
    d.apply(0.02, t=0.4)
    try:
        r.refit_bvh(cs, topology=topo, keep_on_device=True)
        nodes = r.read_device_bvh()
        assert (nodes != topo).any()
        r.upload_scene(cs, device_tree=True)
        W, H, spp, seed = 160, 96, 3, 9
        r.create_framebuffer(W, H)
        st = r.render_frame(spp, seed)
        got = r.read().copy()
        cs.set_bvh(nodes)
        assert_oracle_frame(oracle, cs, got, st, opts(), W, H, spp, seed, "refitted tree under an environment")
    finally:
        d.restore()
