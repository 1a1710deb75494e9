"""hj_trace_paths_adaptive, the part that needs no GPU: the symbol is declared, listed and exported; every argument refusal comes
before the device is touched, with its status and a message, and writes nothing; a valid call gets HJ_ERR_DEVICE where there is no
device; the Python wrapper's own checks raise before any call; and, from the oracle alone, the premises of the GPU tests: their
setting spreads the rays over every possible sample count, and the reference (path_adaptive_ref.expected) agrees with the headline
invariant - a ray's record is path_query_ref.compose of that ray alone at spp = n_i."""
import os

import numpy as np
import pytest

import path_adaptive_ref as A
import path_query_ref as R
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions

U, F = np.uint32, np.float32


def _aopts(spp_min=4, spp_step=4, spp_max=16, rel_error=0.5, floor=0.01):
    return abi.AdaptiveOpts(spp_min, spp_step, spp_max, rel_error, floor)


def _opts(**kw):
    o = abi.RenderOpts.default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _call(rays, n, a, opts, flags, samples, moments=None, stats=None, ctx=None):
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)  # noqa: E731
    return device.lib().hj_trace_paths_adaptive(ctx, p(rays), n, a, opts, flags, p(samples), p(moments), stats)


def test_entry_point_is_declared_listed_and_exported():
    assert "hj_trace_paths_adaptive" in declared_functions("hijiki_hip.h")
    assert "hj_trace_paths_adaptive" in device.EXPORTS and hasattr(device.lib(), "hj_trace_paths_adaptive")
    assert device.lib().hj_version() >= 0x000D00
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    assert "typedef struct hj_adaptive_opts" in header
    import ctypes as C
    assert C.sizeof(abi.AdaptiveOpts) == 20 and abi.AdaptiveOpts.rel_error.offset == 12
    assert callable(device.Renderer.trace_paths_adaptive)


def test_argument_refusals_come_before_the_device():
    L = device.lib()
    rays, out, mom = np.zeros((4, 8), F), np.zeros((4, 8), F), np.zeros((4, 4), F)
    st = abi.RenderStats()
    INV, UNS = abi.HJ_ERR_INVALID, abi.HJ_ERR_UNSUPPORTED
    DEV = abi.PATHS_DEVICE_ARRAYS
    ok = _aopts()
    nan, inf = float("nan"), float("inf")
    cases = {
        "null rays": (INV, (None, 4, ok, None, 0, out, mom)),
        "null samples": (INV, (rays, 4, ok, None, 0, None, mom)),
        "unknown flag bits": (INV, (rays, 4, ok, None, 2, out, mom)),
        "unknown flag bits beside the known one": (INV, (rays, 4, ok, None, 0x80000001, out, mom)),
        "null adaptive opts": (INV, (rays, 4, None, None, 0, out, mom)),
        "spp_min 0": (INV, (rays, 4, _aopts(spp_min=0), None, 0, out, mom)),
        "spp_min 1": (INV, (rays, 4, _aopts(spp_min=1), None, 0, out, mom)),
        "spp_step 0": (INV, (rays, 4, _aopts(spp_step=0), None, 0, out, mom)),
        "spp_max below spp_min": (INV, (rays, 4, _aopts(spp_min=8, spp_max=7), None, 0, out, mom)),
        "spp_max above 65536": (INV, (rays, 4, _aopts(spp_step=4096, spp_max=65537), None, 0, out, mom)),
        "rel_error NaN": (INV, (rays, 4, _aopts(rel_error=nan), None, 0, out, mom)),
        "rel_error negative": (INV, (rays, 4, _aopts(rel_error=-0.5), None, 0, out, mom)),
        "rel_error infinite": (INV, (rays, 4, _aopts(rel_error=inf), None, 0, out, mom)),
        "floor NaN": (INV, (rays, 4, _aopts(floor=nan), None, 0, out, mom)),
        "floor negative": (INV, (rays, 4, _aopts(floor=-1e-3), None, 0, out, mom)),
        "floor infinite": (INV, (rays, 4, _aopts(floor=inf), None, 0, out, mom)),
        "65 rounds": (INV, (rays, 4, _aopts(spp_min=2, spp_step=1, spp_max=66), None, 0, out, mom)),
        "65 rounds, the last one short": (INV, (rays, 4, _aopts(spp_min=4, spp_step=4, spp_max=4 + 63 * 4 + 1), None, 0, out, mom)),
        "too many rays": (INV, (rays, 0x80000000, ok, None, 0, out, mom)),
        "misaligned device rays": (INV, (rays.ctypes.data + 4, 3, ok, None, DEV, out, mom)),
        "misaligned device samples": (INV, (rays, 3, ok, None, DEV, out.ctypes.data + 8, mom)),
        "misaligned device moments": (INV, (rays, 3, ok, None, DEV, out, mom.ctypes.data + 4)),
        "max_bounces 0": (INV, (rays, 4, ok, _opts(max_bounces=0), 0, out, mom)),
        "use_bvh 0": (UNS, (rays, 4, ok, _opts(use_bvh=0), 0, out, mom)),
        "split kernels": (INV, (rays, 4, ok, _opts(flags=abi.RENDER_SPLIT_KERNELS), 0, out, mom)),
        "no drain beside the light grid bit": (INV, (rays, 4, ok, _opts(flags=abi.RENDER_NO_DRAIN | abi.RENDER_NO_LIGHT_GRID), 0, out, mom)),
    }
    for name, (status, args) in cases.items():
        L.hj_context_create(-1, None)                                  # (leaves ITS text in hj_last_error(NULL))
        before = L.hj_last_error(None)
        assert _call(*args, stats=st) == status, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_trace_paths_adaptive" in text, (name, text)
    assert (out == 0).all() and (rays == 0).all() and (mom == 0).all()
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


def test_a_valid_call_without_a_gpu_is_a_device_error():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none.  64 rounds, a last
    short round, spp_max = spp_min, rel_error = 0, floor = 0 and no moments are all valid."""
    L = device.lib()
    rays, out, mom = np.zeros((4, 8), F), np.full((4, 8), 7.0, F), np.full((4, 4), 7.0, F)
    for a, n, o, m in ((_aopts(), 4, None, mom), (_aopts(2, 1, 65), 4, _opts(flags=abi.RENDER_NO_LIGHT_GRID), None),
                       (_aopts(4, 4, 4 + 63 * 4), 4, None, mom), (_aopts(4, 5, 16, 0.0, 0.0), 4, None, mom), (_aopts(65536, 1, 65536), 4, None, None),
                       (_aopts(), 0, None, None)):
        rc = _call(rays, n, a, o, 0, out, m)
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert (out == 7.0).all() and (mom == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = np.zeros((3, 8), F)
    for bad in (good.astype(np.float64), np.zeros((3, 7), F), np.zeros(8, F)):
        with pytest.raises(ValueError):
            r.trace_paths_adaptive(bad)
    for seeds in (np.zeros(3, np.int32), np.zeros(4, U), np.zeros((3, 1), U), np.zeros(3, F)):
        with pytest.raises(ValueError):
            r.trace_paths_adaptive(good, seeds=seeds)
    for kw in (dict(spp_min=1), dict(spp_min=0), dict(spp_step=0), dict(spp_min=8, spp_max=7), dict(spp_max=65537, spp_step=4096),
               dict(spp_min=2, spp_step=1, spp_max=66), dict(rel_error=-1.0), dict(rel_error=float("nan")), dict(rel_error=float("inf")),
               dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf"))):
        with pytest.raises(ValueError):
            r.trace_paths_adaptive(good, **kw)
    import torch
    for bad in (torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.float64)):      # on the host: not the renderer's GPU
        with pytest.raises(ValueError):
            r.trace_paths_adaptive(bad)
    assert (good == 0).all()


def test_the_setting_spreads_the_rays_over_every_sample_count():
    """Premise, from the oracle alone: on the cbox ray set at max_bounces = 40, rounds 4 / +4 / up to 16, rel_error = 0.5, floor =
    0.01, each of the four possible n_i is taken by at least 50 rays; the 200 rays that leave the scene stop at spp_min; the ray
    whose seed wraps around (0xFFFFFFFE) is among the rays."""
    e = A.expected_for("cbox")
    took = {m: int((e["n"] == m).sum()) for m in (4, 8, 12, 16)}
    print("cbox, 4 / +4 / 16, rel_error 0.5:", took, "rounds", e["rounds"], e["counts"])
    assert sum(took.values()) == R.N_RAYS
    assert min(took.values()) >= 50, took
    assert (e["n"][-200:] == 4).all() and e["rounds"] == 4
    assert e["counts"]["paths"] == int(e["n"].sum())
    assert (e["samples"][:, 3] == e["n"]).all() and (e["moments"][:, 3] == e["n"]).all()


def test_the_reference_agrees_with_the_headline_invariant():
    """expected()'s record of ray i equals compose(cs, ray_i, n_i) for 50 sampled rays, at least 8 of every sample count: the
    reference's running sums are hj_trace_paths' sum of the ray alone, word for word."""
    cs, rays, o = R.scene("cbox"), R.ray_set("cbox"), R.options(40)
    e = A.expected_for("cbox")
    rng = np.random.default_rng(5)
    pick = np.concatenate([rng.choice(np.flatnonzero(e["n"] == m), 8, replace=False) for m in (4, 8, 12, 16)] + [np.arange(3)])
    rest = np.setdiff1d(np.arange(R.N_RAYS), pick)
    pick = np.concatenate([pick, rng.choice(rest, 50 - len(pick), replace=False)])
    assert len(set(pick.tolist())) == 50
    for i in pick:
        want, _ = R.compose(cs, rays[i:i + 1], int(e["n"][i]), o)
        assert np.array_equal(want.view(U), e["samples"][i:i + 1].view(U)), (int(i), int(e["n"][i]))


def test_stop_rule_restatement_on_hand_made_sums():
    """The numpy restatement on sums whose answer is known: equal samples have no variance and stop at once, also at rel_error =
    0; two samples 0 and 1 have mean 0.5, var 0.5, sem2 0.25 and stop exactly at rel_error = 1; spp_max stops whatever the sums; below
    the floor the threshold is rel_error * floor."""
    f = lambda *v: np.array(v, F)  # noqa: E731
    stop, sem2 = A.stops(f(4.0), f(4.0), 4, A.aopts(rel_error=0.0, floor=0.0))
    assert stop[0] and sem2[0] == 0
    stop, sem2 = A.stops(f(1.0), f(1.0), 2, A.aopts(rel_error=1.0))
    assert stop[0] and sem2[0] == F(0.25)
    assert not A.stops(f(1.0), f(1.0), 2, A.aopts(rel_error=0.99))[0][0]
    assert A.stops(f(1.0), f(1.0), 16, A.aopts(rel_error=0.0))[0][0]
    lo = A.aopts(rel_error=0.5, floor=0.01)        # two samples of mean 1e-3, below the floor: thr = 0.5 * 0.01, thr^2 = 2.5e-5
    S1 = f(2e-3)                                   # S1 * mean = 2e-6, so sem2 = (S2 - 2e-6) / 2: 2e-5 stops, 3e-5 does not
    assert A.stops(S1, f(4.2e-5), 2, lo)[0][0] and not A.stops(S1, f(6.2e-5), 2, lo)[0][0]
    assert not A.stops(S1, f(4.2e-5), 2, A.aopts(rel_error=0.5, floor=0.0))[0][0]
