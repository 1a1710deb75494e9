"""Environment lighting without a GPU: the sampling distribution hj_debug_env_distribution returns against its numpy restatement,
the refusals of bad environments, Scene.set_environment and its PFM path, the CLI's --env flags and the ABI 0.5 struct."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_scenes as es
import texture_scenes as ts
from hijiki_amd import abi, device, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 1), (1, 7), (5, 1), (5, 7), (9, 13), (32, 64), (31, 17))      # (H, W): odd sizes, rows and columns of one


def texture_set(texels, filt):
    s = host.Scene()
    t = s.add_texture(texels, filt)
    m = s.add_diffuse((0.5, 0.5, 0.5))
    s.add_sphere((0.0, 0.0, -3.0), 0.5, m)                      # (a scene needs two shapes)
    s.add_sphere((1.0, 0.0, -3.0), 0.5, m)
    return s.compile(), t


def env(texture=0, scale=(1.0, 1.0, 1.0), select_prob=0.5):
    e = abi.Environment()
    e.texture = texture
    for k in range(3):
        e.scale[k] = scale[k]
    e.select_prob = select_prob
    return e


@pytest.mark.parametrize("filt", [abi.TEX_NEAREST, abi.TEX_BILINEAR])
def test_distribution_matches_numpy(filt):
    rng = np.random.default_rng(3 + filt)
    for H, W in SIZES:
        tex = es.random_env(rng, H, W)
        scale = tuple(float(np.float32(v)) for v in rng.uniform(0.2, 3.0, 3))     # (the struct holds float32)
        cs, t = texture_set(tex, filt)
        d = device.env_distribution(cs.texture_set, env(t, scale))
        w = es.weights(tex, scale, filt)
        want = w / w.sum()
        np.testing.assert_allclose(d["weight_sum"], w.sum(), rtol=1e-12)
        np.testing.assert_allclose(d["prob"], want, rtol=1e-6, atol=0)
        got = es.alias_probabilities(d["alias_prob"], d["alias"])
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-12, err_msg=f"{W} x {H}, filter {filt}")
        assert abs(got.sum() - 1.0) < 1e-6 and abs(float(d["prob"].astype(np.float64).sum()) - 1.0) < 1e-6
        # every cell in which a lookup can be non-zero can be sampled
        m = np.maximum((tex[..., :3].astype(np.float64) * scale).max(-1), 0)
        reach = m if filt == abi.TEX_NEAREST else np.max([np.roll(np.roll(m, a, 0), b, 1) for a in (-1, 0, 1) for b in (-1, 0, 1)], 0)
        assert (got[reach > 0] > 0).all() and (d["prob"][reach > 0] > 0).all()
        assert (d["prob"][reach == 0] == 0).all()
        np.testing.assert_allclose(d["pdf"], want / es.solid_angles(H, W), rtol=1e-6)
        assert (d["alias"] < H * W).all()


def test_black_and_scaled_out_environments():
    cs, t = texture_set(np.zeros((4, 6, 4), np.float32), abi.TEX_BILINEAR)
    d = device.env_distribution(cs.texture_set, env(t, select_prob=0.0))
    assert d["weight_sum"] == 0.0 and (d["prob"] == 0).all()
    cs, t = texture_set(np.ones((4, 6, 4), np.float32), abi.TEX_NEAREST)
    d = device.env_distribution(cs.texture_set, env(t, scale=(0.0, 0.0, 0.0)))
    assert d["weight_sum"] == 0.0
    d = device.env_distribution(cs.texture_set, env(t, scale=(0.0, 2.0, 0.0)))      # one channel is enough
    np.testing.assert_allclose(d["prob"], es.solid_angles(4, 6) / (4 * np.pi), rtol=1e-6)


def test_refusals_carry_a_message():
    L = device.lib()
    cs, t = texture_set(np.ones((4, 6, 4), np.float32), abi.TEX_NEAREST)
    bad = np.ones((4, 6, 4), np.float32)
    bad[2, 3, 1] = np.inf
    cs_inf, _ = texture_set(bad, abi.TEX_NEAREST)
    cases = [(cs, env(1)), (cs, env(t, scale=(1.0, -1.0, 1.0))), (cs, env(t, scale=(np.nan, 1.0, 1.0))),
             (cs, env(t, scale=(1.0, 1.0, np.inf))), (cs, env(t, select_prob=-0.25)), (cs, env(t, select_prob=1.5)),
             (cs, env(t, select_prob=float("nan"))), (cs_inf, env(t))]
    for k, (c, e) in enumerate(cases):
        ts_ = c.texture_set
        rc = L.hj_debug_env_distribution(C.byref(ts_), C.byref(e), None, None, None, None, None)
        assert rc == abi.HJ_ERR_INVALID, k
        assert b"environment" in L.hj_last_error(None), k
    assert L.hj_debug_env_distribution(None, None, None, None, None, None, None) == abi.HJ_ERR_INVALID


def test_scene_set_environment_defaults():
    tex = es.sky_texels(8, 16)
    s = host.Scene.synthetic(host.SYNTH_CBOX)                   # has emitters
    t = s.add_texture(tex, abi.TEX_BILINEAR)
    assert host.Scene.synthetic(host.SYNTH_CBOX).compile().environment is None
    s.set_environment(t, 2.0)
    e = s.compile().environment
    assert (e.texture, list(e.scale), e.select_prob) == (t, [2.0, 2.0, 2.0], 0.5)
    s.set_environment(t, (1.0, 0.5, 0.25), select_prob=0.125)
    e = s.compile().environment
    assert (list(e.scale), e.select_prob) == ([1.0, 0.5, 0.25], 0.125)
    s.set_environment(t, 0.0)                                  # black: NEE never picks it
    assert s.compile().environment.select_prob == 0.0
    assert es.env_only_scene(tex).compile().environment.select_prob == 1.0     # no emitters
    with pytest.raises(ValueError):
        s.set_environment(t, (1.0, 2.0))


def test_environment_from_pfm(tmp_path):
    rgb = es.sky_texels(6, 10)[..., :3]
    path = str(tmp_path / "sky.pfm")
    host.write_image(path, rgb)
    s = host.Scene.synthetic(host.SYNTH_CBOX)
    t = s.set_environment_file(path, scale=3.0, select_prob=0.25)
    cs = s.compile()
    e = cs.environment
    assert (e.texture, e.select_prob, list(e.scale)) == (t, 0.25, [3.0, 3.0, 3.0])
    rec, texels = cs.textures
    assert tuple(rec[t][:3]) == (10, 6, abi.TEX_BILINEAR)
    np.testing.assert_array_equal(texels[rec[t][3]:rec[t][3] + 60, :3].reshape(6, 10, 3), rgb)
    ppm = str(tmp_path / "sky.ppm")
    ts.write_ppm(ppm, ts.PPM_PIX)
    s2 = host.Scene.synthetic(host.SYNTH_CBOX)
    s2.set_environment_file(ppm, filter=abi.TEX_NEAREST)
    assert s2.compile().environment.select_prob == 0.5
    with pytest.raises(abi.HijikiError):
        host.Scene().set_environment_file(str(tmp_path / "missing.pfm"))


def test_cli_env_flags(tmp_path):
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--env <file>" in r.stderr and "--env-scale" in r.stderr
    for bad in (["--env-scale", "x"], ["--env-scale", "-1"], ["--env-scale", "nan"], ["--env"]):
        r = subprocess.run([exe, *bad, "synthetic:cbox"] if bad != ["--env"] else [exe, "synthetic:cbox", "--env"],
                           capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr, bad
    r = subprocess.run([exe, "--env-scale", "2", "synthetic:cbox"], capture_output=True, text=True)
    assert r.returncode == 2 and "--env-scale without --env" in r.stderr
    r = subprocess.run([exe, "--env", str(tmp_path / "missing.pfm"), "synthetic:cbox"], capture_output=True, text=True)
    assert r.returncode == 1 and "missing.pfm" in r.stderr            # (read before any GPU work)


def test_abi_struct_and_version():
    assert C.sizeof(abi.Environment) == 24
    assert abi.Environment.scale.offset == 4 and abi.Environment.select_prob.offset == 16
    L = device.lib()
    assert L.hj_version() >= 0x000500
    for name in ("hj_scene_upload_env", "hj_debug_env_lookup", "hj_debug_env_sample", "hj_debug_env_distribution"):
        assert hasattr(L, name) and name in device.EXPORTS
