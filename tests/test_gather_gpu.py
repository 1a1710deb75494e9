"""hj_trace_irradiance on the GPU: gather records against gather_ref (the oracle) bit for bit - every word of every record, and the
statistics against the reference's counts - on three scenes (pair nodes on and off, an environment) in hemisphere mode at spp 1 and
5 and in sphere + SH9 mode at spp 4; sphere without SH9 against the SH9 record's first eight words; pool, workgroup count, chunk size
and prefix length against each other; device tensors against host arrays; a refused call; a closed form under a constant sky."""
import numpy as np
import pytest

import gather_ref as G
import path_query_ref as R
from hijiki_amd import abi, device

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(U)


def assert_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = bits(got) != bits(want)
    if diff.any():
        i = int(np.argmax(diff.any(axis=1)))
        raise AssertionError(f"{what}: {int(diff.sum())} differing words in {int(diff.any(axis=1).sum())} of {len(want)} records, first at point {i}, "
                             f"words {np.flatnonzero(diff[i]).tolist()}:\n  gpu  {got[i].tolist()}\n  want {want[i].tolist()}")


def assert_counts(stats, counts, what):
    assert {k: stats[k] for k in G.COUNTS} == {k: counts[k] for k in G.COUNTS}, what


def run(r, name, mode, points=None, **kw):
    spp, sphere, sh9 = G.MODES[mode]
    return r.trace_irradiance(G.point_set(name) if points is None else points, spp=spp, sphere=sphere, sh9=sh9, opts=R.options(40), stats=True, **kw)


@pytest.fixture(scope="module")
def gq():
    with device.Renderer(0) as ctx:
        yield ctx


_default = {}


def default_result(gq, name, mode):
    """(records, statistics) of the scene's point set from the module's context: default switches, host arrays"""
    gq.upload_scene(R.scene(name))
    if (name, mode) not in _default:
        _default[name, mode] = run(gq, name, mode)
        _default[name, mode][0].setflags(write=False)
    return _default[name, mode]


@pytest.mark.parametrize("mode", list(G.MODES))
@pytest.mark.parametrize("name", G.SCENES)
def test_records_match_the_reference(gq, name, mode):
    want, counts = G.expected(name, mode)
    got, stats = default_result(gq, name, mode)
    print(f"{name}, {mode}: {counts}; first hits {int(want[:, 4].sum())} of {counts['paths']}")
    assert_records(got, want, f"{name}, {mode}")
    assert_counts(stats, counts, f"{name}, {mode}")
    assert stats["batches"] == 1 and stats["total_ms"] > 0


@pytest.mark.parametrize("name", G.SCENES)
def test_sphere_without_sh9_is_the_sh9_records_head(gq, name):
    want, want_stats = default_result(gq, name, "sphere-sh9-4")
    got, stats = gq.trace_irradiance(G.point_set(name), spp=4, sphere=True, opts=R.options(40), stats=True)
    assert_records(got, want[:, 0:8], f"{name}: sphere, no SH9")
    assert_counts(stats, want_stats, f"{name}: sphere, no SH9")
    assert (want[:, 35] == 0).all() and (want[:, 6:8] == 0).all()


@pytest.mark.parametrize("switch", ["HJ_PATHS_WGS=1 HJ_PATHS_POOL=64", "HJ_PATHS_WGS=3 HJ_PATHS_POOL=128", "HJ_PATHS_CHUNK=1000"])
def test_scheduling_never_shows_in_a_result(gq, monkeypatch, switch):
    """One workgroup of 64 positions (dozens of top-ups, and the one-wave tail), three of 128, launches of 1000 samples (whole
    points: 200 at spp 5, 250 at spp 4): a context created under the setting returns the bits of the default one, and its counts."""
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(R.scene("cbox"))
        for mode in ("hemisphere-5", "sphere-sh9-4"):
            want, want_stats = G.expected("cbox", mode)
            got, stats = run(r, "cbox", mode)
            assert_records(got, want, f"{switch}, {mode}")
            assert_counts(stats, want_stats, f"{switch}, {mode}")
            assert stats["batches"] == (3 if "CHUNK" in switch else 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_prefixes(gq, n):
    for mode in ("hemisphere-5", "sphere-sh9-4"):
        want, _ = default_result(gq, "cbox", mode)
        got, _ = run(gq, "cbox", mode, G.point_set("cbox")[:n])
        assert_records(got, want[:n], f"n = {n}, {mode}")


def test_device_tensors(gq):
    import torch
    pts = G.point_set("rich")
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(pts.copy()).to(dev)
    keep = t.clone()
    for mode in ("hemisphere-5", "sphere-sh9-4"):
        want, want_stats = default_result(gq, "rich", mode)
        got, stats = run(gq, "rich", mode, t)
        assert isinstance(got, torch.Tensor) and got.device == dev and tuple(got.shape) == want.shape
        assert_records(got.cpu().numpy(), want, f"device tensors, {mode}")
        assert_counts(stats, want_stats, f"device tensors, {mode}")
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the point tensor changed"
    seeds = torch.from_numpy(pts.view(np.int32)[:, 6].copy()).to(dev)
    zeroed = t.clone()
    zeroed.view(torch.int32)[:, 6] = 0
    got2, _ = run(gq, "rich", "hemisphere-5", zeroed, seeds=seeds)
    assert (zeroed.view(torch.int32)[:, 6] == 0).all(), "seeds were written into the caller's tensor"
    assert_records(got2.cpu().numpy(), default_result(gq, "rich", "hemisphere-5")[0], "device tensors with seeds")
    zp = pts.copy()
    zp.view(U)[:, 6] = 0
    got3, _ = run(gq, "rich", "hemisphere-5", zp, seeds=pts.view(U)[:, 6].copy())
    assert_records(got3, default_result(gq, "rich", "hemisphere-5")[0], "host arrays with seeds")
    for b in (t.cpu(), t.double(), t[::2], t[:, :7].contiguous(), t.reshape(-1)):
        with pytest.raises(ValueError):
            gq.trace_irradiance(b)
    assert tuple(gq.trace_irradiance(t[:0], sphere=True, sh9=True).shape) == (0, 36)


def test_a_refused_call_leaves_out_untouched(gq):
    """With a live context and a scene: every kind of refusal writes nothing, neither records nor statistics; the context's text."""
    gq.upload_scene(R.scene("cbox"))
    L = device.lib()
    pts = G.point_set("cbox")[:64].copy()
    out = np.full((64, 36), 7.0, F)
    st = abi.RenderStats()
    zero = pts.copy()
    zero[63, 3:6] = 0
    o0 = abi.RenderOpts.default()
    o0.max_bounces = 0
    for p, spp, o, flags in ((pts, 1, None, 8), (pts, 1, None, abi.GATHER_SH9), (pts, 0, None, 0), (pts, 1, o0, 0), (zero, 1, None, 0)):
        rc = L.hj_trace_irradiance(gq._h, p.ctypes.data, 64, spp, o, flags, out.ctypes.data, st)
        assert rc == abi.HJ_ERR_INVALID and b"hj_trace_irradiance" in L.hj_last_error(gq._h)
    assert (out == 7.0).all() and not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)
    with device.Renderer(0) as r:                                      # no scene yet
        assert L.hj_trace_irradiance(r._h, pts.ctypes.data, 64, 1, None, 0, out.ctypes.data, st) == abi.HJ_ERR_STATE
        assert b"scene" in L.hj_last_error(r._h)
        assert L.hj_trace_irradiance(r._h, None, 0, 1, None, 0, None, None) == abi.HJ_ERR_STATE
    assert (out == 7.0).all()
    assert L.hj_trace_irradiance(gq._h, None, 0, 1, None, 0, None, None) == abi.HJ_OK       # n == 0: nothing to do
    got = gq.trace_irradiance(zero, spp=4, sphere=True, opts=R.options(40))   # (sphere mode never reads the normal)
    assert_records(got, default_sphere_head(gq)[:64], "an all-zero normal in sphere mode")


def default_sphere_head(gq):
    return default_result(gq, "cbox", "sphere-sh9-4")[0][:, 0:8]


def test_closed_form_under_a_constant_sky(gq):
    """Points above all geometry, facing up, under a constant environment of 0.5, spp = 64: every cosine sample leaves the scene and
    brings exactly 0.5, so the sums are exactly 32, nothing is hit and the nearest hit is +inf."""
    gq.upload_scene(G.closed_form_scene())
    got, stats = gq.trace_irradiance(G.closed_form_points(), spp=64, opts=R.options(40), stats=True)
    assert (got[:, 0:3] == 32.0).all(), got[(got[:, 0:3] != 32.0).any(1)][:3]
    assert (got[:, 3] == 64.0).all() and (got[:, 4] == 0).all() and np.isposinf(got[:, 5]).all() and (got[:, 6:8] == 0).all()
    assert stats["paths"] == 64 * len(got) == stats["closest_rays"] and stats["hits"] == 0 and stats["shadow_rays"] == 0
