"""Environment lighting in the C oracle (no GPU): its lookup and its next-event sample bit for bit against the numpy restatements
of DESIGN.md "Environment lighting" (tests/env_scenes.py: the definitions the kernels' probes are pinned to), environment-lit
frames and shading steps against the float64 restatement (tests/golden/glsl_f64.py), closed forms, the premises of the scenes the
GPU tests render, and the environments it refuses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import glsl_f64 as G  # noqa: E402
import env_scenes as es  # noqa: E402
from hijiki_amd import abi, host  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def probe_dirs(rng):
    """The direction set of test_environment_gpu.py test_lookup_probe_is_bit_exact."""
    v = [0.0, -0.0, 1.0, -1.0, 2.5, -3e-20, 1e-30]
    grid = np.array(np.meshgrid(v, v, v)).reshape(3, -1).T
    rand = rng.normal(size=(30000, 3)) * rng.uniform(1e-3, 1e3, (30000, 1))
    extra = [[0, 1, 0], [0, -1, 0], [0, 7, 1e-7], [0, -7, -1e-7], [1e-8, 1, 0], [np.inf, 0, 1], [np.nan, 1, 0]]
    return np.concatenate([grid, rand, extra]).astype(F)


def test_oracle_lookup_is_bit_exact(oracle):
    rng = np.random.default_rng(21)
    dirs = probe_dirs(rng)
    for filt, (H, W) in ((abi.TEX_NEAREST, (32, 64)), (abi.TEX_BILINEAR, (9, 13)), (abi.TEX_BILINEAR, (1, 5)),
                         (abi.TEX_NEAREST, (1, 7)), (abi.TEX_BILINEAR, (5, 1)), (abi.TEX_NEAREST, (1, 1))):
        scale = (0.5, 2.0, 1.25)
        cs = es.env_only_scene(es.random_env(rng, H, W), filt, scale).compile()
        got = oracle.env_lookup(cs, dirs)
        want = es.lookup(oracle, cs.texture_set, cs.environment.texture, scale, dirs)
        bad = (bits(got) != bits(want)).any(axis=1)
        assert not bad.any(), f"{W} x {H}, filter {filt}: {int(bad.sum())} lookups differ, first {dirs[bad][0]}"


def edge_states(table, W, H):
    """States whose coin equals a threshold exactly, and whose draws a / b are 0xFFFFFFFF or as close to 0 as xorshift32 gets
    (it never draws 0: 1 stands in, which picks column 0 and the first sub-cell like 0 would)."""
    thr = es.threshold_states(table, W, H)
    ends = [es.states_with_draws(second=0xFFFFFFFF), es.states_with_draws(second=1), es.states_with_draws(third=0xFFFFFFFF),
            es.states_with_draws(third=1), es.states_with_draws(third=0xFFFF), es.states_with_draws(third=0xFFFF0000),
            es.states_with_draws(first=0xFFFFFFFF), es.states_with_draws(first=1)]
    return thr, np.array(ends, np.uint32)


@pytest.mark.parametrize("filt,size", [(abi.TEX_NEAREST, (32, 64)), (abi.TEX_BILINEAR, (9, 13)), (abi.TEX_BILINEAR, (1, 7)),
                                       (abi.TEX_NEAREST, (5, 1))])
def test_oracle_sample_is_bit_exact(oracle, filt, size):
    """hjo_env_sample == es.sample (direction, pdf, cell, Le / pdf) for 2^20 random states, states whose coin is exactly their
    column's threshold (there `>=` takes the alias: the restatement and the oracle must both) and the ends of both draws."""
    H, W = size
    rng = np.random.default_rng(5 + H)
    cs = es.env_only_scene(es.random_env(rng, H, W), filt, (1.0, 0.5, 2.0)).compile()
    table = oracle.env_table(cs.texture_set, cs.environment)
    thr, ends = edge_states(table, W, H)
    if H * W > 16:
        assert len(thr) >= 1                                    # (a column whose threshold some coin equals exactly was reached)
    states = np.concatenate([rng.integers(1, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32), thr, ends])
    got = oracle.env_sample(cs, states)
    want = es.sample(oracle, cs, table, states)
    bad = (bits(got) != bits(want)).any(axis=1)
    assert not bad.any(), f"{W} x {H}: {int(bad.sum())} samples differ, first state {states[bad][0]}: {got[bad][0]} {want[bad][0]}"
    if len(thr):                                                # the threshold-equal states did take the alias cell
        k = len(states) - len(ends) - len(thr)
        s1 = es.rng_next(thr)
        col = ((es.rng_next(s1).astype(np.uint64) * np.uint64(W * H)) >> np.uint64(32)).astype(np.int64)
        assert (s1.astype(F) * F(2.0 ** -32) == table[col, 0]).all()
        assert (got[k:k + len(thr), 4].astype(np.int64) == table[col, 1].copy().view(np.uint32)).all()
    d = got[:, :3].astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)


def _close(a32, a64, frac):
    """tests/test_textures_oracle.py's bars (= tests/test_glsl_f64.py's for random scenes)."""
    close = (np.abs(a64 - a32) <= 1e-4 * np.maximum(1.0, np.abs(a32))).all(-1)
    assert close.mean() > frac, close.mean()
    np.testing.assert_allclose(a64[..., 3], a32[..., 3], rtol=3e-4)
    s32, s64 = a32[..., :3].sum(), a64[..., :3].sum()
    assert abs(s64 - s32) < 0.03 * abs(s32)


def f64_scene(oracle, cs):
    return G.Scene(cs, env_table=oracle.env_table(cs.texture_set, cs.environment))


FRAME_SCENES = {
    "mixed": (lambda: es.mixed_scene(), 5),                     # (scene, master seed of the frame's blocks)
    "tinted": (lambda: es.mixed_scene(tinted=True), 5),
    "cluster, no emitters": (lambda: es.cluster_scene(), 5),
    "cluster, one bright texel": (lambda: es.cluster_scene(single_texel(), abi.TEX_NEAREST), 5),
    "random 1, p 0.125": (lambda: es.random_scene_with_env(1, 0.125), 1),       # (test_glsl_f64.py's frames of random_scene)
    "random 2, p 0.875": (lambda: es.random_scene_with_env(2, 0.875, abi.TEX_NEAREST), 2),
}


def single_texel(H=6, W=9):
    t = np.zeros((H, W, 4), F)
    t[1, 4, :3] = (30.0, 25.0, 20.0)
    return t


@pytest.mark.parametrize("name", list(FRAME_SCENES))
def test_environment_frames_oracle_vs_float64(oracle, name):
    """Whole frames under an environment - misses after camera, mirror and glass rays, the per-channel extinction rule, both
    branches of the selection - against the float64 integrator at the bars of the textured and random scenes."""
    make, seed = FRAME_SCENES[name]
    cs = make()
    W, H = 80, 48
    blocks = host.make_blocks(W, H, 2, seed)
    a32, ctr, _ = oracle.render_blocks(cs, blocks, W, H)
    _close(a32, G.render_blocks(f64_scene(oracle, cs), blocks, W, H), 0.95)
    assert ctr["nee_evals"] > 0 and ctr["shadow_calls"] > 0


def test_scene_premises(oracle):
    """The GPU tests' frames exercise what they claim to (conditions on the inputs, from the oracle's ray log): environment
    shadow rays exist and some are unoccluded, rays leave the scene after mirror and glass bounces and from the camera, and in the
    tinted scene with non-zero extinction."""
    W, H = 160, 96
    blocks = host.make_blocks(W, H, 1, 7)
    for name, cs in (("mixed", es.mixed_scene()), ("tinted", es.mixed_scene(tinted=True)), ("cluster", es.cluster_scene()),
                     ("random", es.random_scene_with_env(1, 0.125))):
        p = es.ray_log_premises(cs, oracle.logged_rays(cs, blocks))
        assert p["env_shadow"] > 100 and p["env_shadow_free"] > 50 and p["discrete_misses"] > 20, (name, p)
        if name == "cluster":
            assert p["area_shadow"] == 0 and p["camera_misses"] > 100 and p["diffuse_misses"] > 100, p
        else:
            assert p["area_shadow"] > 100, (name, p)
        if name == "tinted":
            assert p["tinted_misses"] > 50 and p["camera_misses"] > 100, p


def sample_stats(oracle, cs, W, H, spp, seed):
    vals = [oracle.integrate_block(cs, b)[0][..., :3].reshape(-1, 3).astype(np.float64) for b in host.make_blocks(W, H, spp, seed)]
    v = np.concatenate(vals)
    return v.mean(0), v.std(0) / np.sqrt(len(v))


def test_analytic_sky(oracle):
    """test_environment_gpu.py test_analytic_sky on the oracle: every pixel's expectation in closed form, 4 standard errors."""
    tex = es.sky_texels(32, 64)
    cs = es.analytic_sky_scene(tex)
    assert cs.environment.select_prob == 1.0
    mean, se = sample_stats(oracle, cs, 128, 128, 8, 9)
    expect = es.analytic_sky_expectation(tex)
    assert (np.abs(mean - expect) < 4 * se).all(), (mean, expect, se)


def test_uniform_sky_on_a_convex_sphere(oracle):
    """A convex diffuse sphere of albedo rho under a uniform sky L, select_prob 1: the sphere never sees itself, so its pixels
    expect rho * L (4 standard errors of the mean over the disc); a background sample is L exactly."""
    L, rho = 1.5, 0.6
    cs = es.uniform_sky_sphere_scene(L, rho)
    W = H = 128
    disc, wall = __import__("scenes").furnace_masks(W, H)
    v = np.stack([oracle.integrate_block(cs, b)[0][..., :3].astype(np.float64) for b in host.make_blocks(W, H, 16, 3)])
    assert (v[:, wall] == np.float64(F(L))).all()
    on = v[:, disc].reshape(-1, 3)
    mean, se = on.mean(0), on.std(0) / np.sqrt(len(on))
    assert (se > 0).all() and (np.abs(mean - rho * L) < 4 * se).all(), (mean, rho * L, se)


def test_select_prob_leaves_the_mean(oracle):
    """select_prob 0.125 / 0.5 / 0.875 are three estimators of one integral: pairwise within 4 standard errors."""
    res = [sample_stats(oracle, es.cluster_scene(select_prob=p, light=True), 128, 128, 6, 11 + k)
           for k, p in enumerate((0.125, 0.5, 0.875))]
    for i in range(3):
        assert (res[i][0] > 10 * res[i][1]).all()
        for j in range(i + 1, 3):
            se = np.sqrt(res[i][1] ** 2 + res[j][1] ** 2)
            assert (np.abs(res[i][0] - res[j][0]) < 4 * se).all(), (i, j, res[i], res[j])


def test_environment_shading_step_vectors(oracle):
    """hjo_shade_probe under an environment against the float64 step: the next-event term (either branch of the selection),
    shadow direction and tMax, the RNG state after the step."""
    cs = es.random_scene_with_env(3, 0.5)
    sc = f64_scene(oracle, cs)
    rs = np.random.RandomState(3)
    n = 20000
    o = rs.uniform((-1.1, 0.05, -1.1), (1.1, 1.9, 1.1), (n, 3))
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.concatenate([o, d, np.full((n, 1), 1e-4), np.full((n, 1), np.inf)], 1).astype(F)
    rng0 = G.seed_rng(np.arange(n, dtype=np.uint32) * 5 + 1)
    out, ids, rng_after = oracle.shade_probe(cs, rays, rng0)
    r = rays.astype(np.float64)
    its = G.intersect_scene(sc, r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7])
    mat = sc.materials[np.maximum(its.id, 0)]
    tag, midx = mat >> G.TAG_SHIFT, mat & ((1 << G.TAG_SHIFT) - 1)
    dif = (its.id == ids) & (ids >= 0) & ((tag == G.DIFFUSE) | (tag == G.CBOARD) | (tag == G.TEXTURED))
    idx = np.nonzero(dif)[0]
    assert len(idx) > 5000
    rng = G.Rng(rng0)
    imp, sdir, stmax = G.sample_emitter(sc, its.p[idx], rng, idx)
    env = np.isinf(stmax)
    assert env.sum() > 1500 and (~env).sum() > 1500
    assert (np.isinf(out[idx, 7]) == env).all()                       # the same branch of the selection, path by path
    np.testing.assert_allclose(out[idx, 4:7], sdir, atol=2e-4)
    fin = ~env
    np.testing.assert_allclose(out[idx[fin], 7], stmax[fin], rtol=1e-4, atol=1e-4)
    want = (np.sqrt((imp * imp).sum(1)) > G.EPS) & ((sdir * its.n[idx]).sum(1) > 0)
    col = G.albedo(sc, tag[idx], midx[idx], its.u[idx], its.v[idx])
    f = np.where(want[:, None], (its.n[idx] * sdir).sum(1)[:, None] * col / G.PI * imp, 0.0)
    got = out[idx, 1:4]
    ok = (np.abs(got - f) <= 1e-4 * np.maximum(1.0, np.abs(f))).all(1)
    assert ok[env].mean() > 0.99 and ok[~env].mean() > 0.99, (ok[env].mean(), ok[~env].mean())
    assert (got[env] != 0).any(axis=1).sum() > 500 and (got[~env] != 0).any(axis=1).sum() > 500


def test_black_environment_changes_no_bit(oracle):
    """select_prob 0 over black texels: the oracle's frame and counters are those of the scene without an environment."""
    W, H, spp, seed = 96, 64, 2, 5
    s = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES)
    plain = s.compile()
    s.set_environment(s.add_texture(np.zeros((6, 10, 4), F), abi.TEX_BILINEAR))
    cs = s.compile()
    assert cs.environment.select_prob == 0.0
    blocks = host.make_blocks(W, H, spp, seed)
    a, ca, _ = oracle.render_blocks(cs, blocks, W, H)
    b, cb, _ = oracle.render_blocks(plain, blocks, W, H)
    assert (bits(a) == bits(b)).all() and ca == cb


def env(texture=0, scale=(1.0, 1.0, 1.0), select_prob=0.5):
    e = abi.Environment()
    e.texture = texture
    for k in range(3):
        e.scale[k] = scale[k]
    e.select_prob = select_prob
    return e


def test_oracle_refuses_what_the_upload_refuses(oracle):
    """Every case of test_environment_host.py test_refusals_carry_a_message (on a scene WITH emitters, so that the case's own
    reason is what refuses), the two of test_environment_gpu.py that need a scene - no emitters but select_prob != 1, a black
    environment that is sampled - and a table of the wrong size: HJ_ERR_INVALID from every shading entry point, nothing rendered."""
    L = oracle.lib()
    tex = np.ones((4, 6, 4), F)
    bad = tex.copy()
    bad[2, 3, 1] = np.inf

    def cbox(t):
        s = host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=64)
        i = s.add_texture(t, abi.TEX_NEAREST)
        return s.compile(), i

    cs, t = cbox(tex)
    cs_inf, _ = cbox(bad)
    cs_black, _ = cbox(np.zeros((4, 6, 4), F))
    dark = es.env_only_scene(tex).compile()                     # no emitters
    good = oracle.env_table(cs.texture_set, env(t))
    cases = [(cs, env(t + 1), good), (cs, env(t, scale=(1.0, -1.0, 1.0)), good), (cs, env(t, scale=(np.nan, 1.0, 1.0)), good),
             (cs, env(t, scale=(1.0, 1.0, np.inf)), good), (cs, env(t, select_prob=-0.25), good), (cs, env(t, select_prob=1.5), good),
             (cs, env(t, select_prob=float("nan")), good), (cs_inf, env(t), good),
             (dark, env(dark.environment.texture, select_prob=0.5), good),
             (cs_black, env(t, select_prob=0.5), oracle.env_table(cs_black.texture_set, env(t, select_prob=0.0))),
             (cs, env(t), good[:-1]), (cs, env(t), None)]
    W, H = 32, 16
    blocks = host.make_blocks(W, H, 1, 3)
    rays = np.array([[0, 1, 3, 0, 0, -1, 1e-4, np.inf]], F)
    for k, (c, e, table) in enumerate(cases):
        acc = np.zeros((H, W, 4), F)
        out = np.zeros((16, 16, 8), F)
        probe = np.zeros(20, F)
        blk = host.make_blocks(16, 16, 1, 3)[0]
        tset = c.texture_set                                    # (held: the oracle borrows it)
        L.hjo_set_textures(C.byref(tset))
        L.hjo_set_environment(C.byref(e), table.ctypes.data_as(C.POINTER(C.c_float)) if table is not None else None,
                              len(table) if table is not None else 0)
        try:
            o = abi.RenderOpts.default()
            assert L.hjo_render_blocks(C.byref(c.desc), blocks, len(blocks), C.byref(o), W, H, acc.ctypes.data_as(C.POINTER(C.c_float)),
                                       2, None, None) == abi.HJ_ERR_INVALID, k
            assert L.hjo_integrate_block(C.byref(c.desc), C.byref(blk), C.byref(o), out.ctypes.data_as(C.POINTER(C.c_float)),
                                         None) == abi.HJ_ERR_INVALID, k
            assert L.hjo_shade_probe(C.byref(c.desc), rays.ctypes.data_as(C.POINTER(C.c_float)),
                                     np.ones(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), 1,
                                     probe.ctypes.data_as(C.POINTER(C.c_float))) == abi.HJ_ERR_INVALID, k
        finally:
            L.hjo_set_environment(None, None, 0)
            L.hjo_set_textures(None)
        assert not acc.any() and not out.any() and not probe.any(), k
    with pytest.raises(abi.HijikiError) as err:                 # the Python path: the refusal arrives as the status
        oracle.env_lookup(cs, [[0, 1, 0]], env=env(t + 1))
    assert err.value.status == abi.HJ_ERR_INVALID
    with pytest.raises(abi.HijikiError) as err:                 # a probe without an environment
        oracle.env_lookup(cs, [[0, 1, 0]])
    assert err.value.status == abi.HJ_ERR_STATE
    acc, _, _ = _render(oracle, cs, env(t), blocks, W, H)       # and the good one renders
    assert (acc[..., 3] > 0).all()


def _render(oracle, cs, e, blocks, W, H):
    cs.environment = e
    try:
        return oracle.render_blocks(cs, blocks, W, H)
    finally:
        cs.environment = None
