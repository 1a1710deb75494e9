"""hj_probe_points, hj_bake_probes and hj_sample_probes on the GPU, bit for bit against probe_ref: the points of small grids and of
one beyond a workgroup; the bake on three scenes (pair nodes on and off, an environment) with its statistics; the bake as the
composition of the public gather and the resolve, also when the gather is split into several launches; the validity rule; the
look-up on fabricated volumes - invalid probes, whole invalid cells, fractional validity, NaN behind zero validity - at points
inside, on every plane, outside and at the corners, with NaN and infinite positions on the device route, at sizes around a wave and
at one the grid-stride loop takes a second trip for; guard patterns and refused calls; bake and look-up end to end."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G
import path_query_ref as R
import probe_ref as P
from hijiki_amd import abi, device

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SEED, STRIDE = 0xFFFFFFF0, 7                                            # (the seed wraps at the third probe)


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(U)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = bits(got) != bits(want)
    if diff.any():
        g2, w2, d2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]), diff.reshape(-1, got.shape[-1])
        i = int(np.argmax(d2.any(axis=1)))
        raise AssertionError(f"{what}: {int(diff.sum())} differing words in {int(d2.any(axis=1).sum())} of {len(w2)} records, first at record {i}, "
                             f"words {np.flatnonzero(d2[i]).tolist()}:\n  gpu  {g2[i].tolist()}\n  want {w2[i].tolist()}")


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def grid_kw(d, **kw):
    """a probe_ref desc as the wrapper's keywords"""
    return dict(dict(origin=d["origin"], spacing=d["spacing"], count=d["count"]), **kw)


@pytest.fixture(scope="module")
def pv():
    with device.Renderer(0) as ctx:
        yield ctx


# ---------------------------------------------------------------------------------------------------------------------- points

@pytest.mark.parametrize("count", [(1, 1, 1), (3, 2, 2), (5, 4, 3), (64, 1, 65)])
def test_points_match_the_reference(pv, count):
    """(64, 1, 65): 4160 probes - more than one workgroup, and no multiple of 64.  No scene is needed: the module's context has none
    when this runs first, and any it has later is not read."""
    import torch
    d = P.desc((-1.25, 0.5, 3.0), (0.3, 0.7, 0.011), count, SEED, STRIDE)
    want = P.points(d)
    got = pv.probe_points(**grid_kw(d, seed=SEED, seed_stride=STRIDE))
    assert_bits(got, want, f"points {count}, host arrays")
    t = pv.probe_points(**grid_kw(d, seed=SEED, seed_stride=STRIDE), device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert_bits(t.cpu().numpy(), want, f"points {count}, device arrays")
    if len(want) > 3:
        assert want.view(U)[2:4, 6].tolist() == [0xFFFFFFFE, 5]         # (the seed wraps between probes 2 and 3)


# ------------------------------------------------------------------------------------------------------------------------ bake

@pytest.mark.parametrize("name", G.SCENES)
def test_bake_matches_the_reference(pv, name):
    d, want, rec, counts = P.expected_bake(name)
    pv.upload_scene(R.scene(name))
    got, stats = pv.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=P.BAKE_SPP, opts=R.options(40), stats=True)
    print(f"{name}: {counts}; nearest hits {rec[:, 5].tolist()}")
    assert got.shape == (2, 2, 3, 28)
    assert_bits(got.reshape(-1, 28), want, f"bake, {name}")
    assert {k: stats[k] for k in G.COUNTS} == {k: counts[k] for k in G.COUNTS}, name
    assert (got[..., 27] == 1).all()                                    # min_distance = 0 validates every probe
    t, tstats = pv.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=P.BAKE_SPP, opts=R.options(40), stats=True, device=True)
    assert_bits(t.cpu().numpy().reshape(-1, 28), want, f"bake, {name}, device arrays")
    assert {k: tstats[k] for k in G.COUNTS} == {k: counts[k] for k in G.COUNTS}, name


def composed(r, d, spp):
    """the bake from its public parts: probe_points -> trace_irradiance(sphere, sh9) -> probe_ref.resolve"""
    pts = r.probe_points(**grid_kw(d, seed=SEED, seed_stride=STRIDE))
    rec, stats = r.trace_irradiance(pts, spp=spp, sphere=True, sh9=True, opts=R.options(40), stats=True)
    return P.resolve(rec, spp, d["min_distance"]), stats


_composed = {}


def composed_default(pv):
    """(the composition on cbox at (5, 4, 3), spp 5, from the module's context with default switches, its statistics, the desc)"""
    cs = R.scene("cbox")
    pv.upload_scene(cs)
    if "v" not in _composed:
        d = P.grid_in_domain(cs, (5, 4, 3))
        _composed["v"] = composed(pv, d, 5) + (d,)
        _composed["v"][0].setflags(write=False)
    return _composed["v"]


def test_bake_is_the_composition_of_its_public_parts(pv):
    want, want_stats, d = composed_default(pv)
    got, stats = pv.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=5, opts=R.options(40), stats=True)
    assert_bits(got.reshape(-1, 28), want, "bake against probe_points -> trace_irradiance -> resolve")
    assert {k: stats[k] for k in G.COUNTS} == {k: want_stats[k] for k in G.COUNTS} and stats["batches"] == 1
    assert np.isfinite(got).all() and (got[..., 0:3] != 0).any()


@pytest.mark.parametrize("switch", ["HJ_PATHS_WGS=1 HJ_PATHS_POOL=64", "HJ_PATHS_CHUNK=100"])
def test_scheduling_never_shows_in_a_bake(pv, monkeypatch, switch):
    """One workgroup of 64 positions (several top-ups); launches of 100 samples (whole probes: 20 at spp 5, three launches for 60
    probes): a context created under the setting bakes the bits of the default one, with its counts."""
    want, want_stats, d = composed_default(pv)
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(R.scene("cbox"))
        got, stats = r.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=5, opts=R.options(40), stats=True)
        assert_bits(got.reshape(-1, 28), want, switch)
        assert {k: stats[k] for k in G.COUNTS} == {k: want_stats[k] for k in G.COUNTS}
        assert stats["batches"] == (3 if "CHUNK" in switch else 1)


def test_validity_is_the_min_distance_rule(pv):
    """min_distance from the reference's own nearest-hit column: the median of its distinct finite values, so that some probes lie
    nearer to a surface than it and some do not; the coefficients do not depend on it."""
    d, want0, rec, _ = P.expected_bake("cbox")
    near = np.unique(rec[np.isfinite(rec[:, 5]), 5])
    assert len(near) >= 2, near
    md = float(near[len(near) // 2])
    want = P.resolve(rec, P.BAKE_SPP, md)
    assert (want[:, 27] == 1).any() and (want[:, 27] == 0).any(), want[:, 27]
    pv.upload_scene(R.scene("cbox"))
    got = pv.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE, min_distance=md), spp=P.BAKE_SPP, opts=R.options(40)).reshape(-1, 28)
    assert_bits(got, want, f"min_distance {md}")
    assert_bits(got[:, 0:27], want0[:, 0:27], "the coefficients under another min_distance")
    assert (got[:, 27] == 1).any() and (got[:, 27] == 0).any()


# ---------------------------------------------------------------------------------------------------------------------- sample

COUNTS = [(1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2), (5, 4, 3)]
GRID = dict(origin=(0.5, -1.0, 2.0), spacing=(0.5, 0.25, 1.5))


def second_trip():
    """a point count for which k_pv_sample's grid - 8 workgroups of 256 a compute unit - takes a second trip of its loop, with a
    ragged end: 524 353 on a card of 256 compute units"""
    return cus() * 8 * 256 + 65


@pytest.mark.parametrize("count", COUNTS)
def test_sample_matches_the_reference(pv, count):
    """host arrays (finite points) and device tensors (NaN and infinite positions as well), n = 1, 63, 64, 65 and 260; the output
    tensor beyond n keeps its guard pattern"""
    import torch
    d = P.desc(GRID["origin"], GRID["spacing"], count)
    vol = P.fabricated_volume(count, 9)
    dev = torch.device("cuda", 0)
    tvol = torch.from_numpy(vol).to(dev)
    for n in (1, 63, 64, 65, 260):
        pts = P.sample_points(d, n, 3)
        got = pv.sample_probes(vol, GRID["origin"], GRID["spacing"], pts)
        assert_bits(got, P.sample(d, vol, pts), f"sample {count}, n = {n}, host arrays")
        pts = P.sample_points(d, n, 5, nonfinite=True)
        want = P.sample(d, vol, pts)
        tp = torch.from_numpy(pts).to(dev)
        keep = tp.clone()
        t = pv.sample_probes(tvol, GRID["origin"], GRID["spacing"], tp)
        assert isinstance(t, torch.Tensor) and t.device == dev and tuple(t.shape) == (n, 4)
        assert_bits(t.cpu().numpy(), want, f"sample {count}, n = {n}, device arrays")
        assert torch.equal(tp.view(torch.int32), keep.view(torch.int32)), "the point tensor changed"
        assert np.isfinite(want).all()
        # the raw call into a larger tensor: nothing beyond n is written
        out = torch.full((n + 64, 4), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        dd = P.abi_desc(GRID["origin"], GRID["spacing"], count, flags=abi.PROBES_DEVICE_ARRAYS)
        assert device.lib().hj_sample_probes(pv._h, C.byref(dd), tvol.data_ptr(), tp.data_ptr(), n, out.data_ptr()) == abi.HJ_OK
        assert_bits(out[:n].cpu().numpy(), want, f"sample {count}, n = {n}, raw call")
        assert (out[n:] == 7.0).all(), "written beyond n"
    pos, nm = np.ascontiguousarray(pts[:, 0:3]), np.ascontiguousarray(pts[:, 3:6])       # positions and normals apart
    t2 = pv.sample_probes(tvol, GRID["origin"], GRID["spacing"], torch.from_numpy(pos).to(dev), torch.from_numpy(nm).to(dev))
    assert_bits(t2.cpu().numpy(), want, "positions and normals as two tensors")
    assert tuple(pv.sample_probes(tvol, GRID["origin"], GRID["spacing"], tp[:0]).shape) == (0, 4)


def test_sample_takes_a_second_trip(pv):
    """(5, 4, 3), n from the card's compute units: the grid-stride loop runs twice for the first threads, once for the last"""
    import torch
    count = (5, 4, 3)
    n = second_trip()
    assert n > cus() * 8 * 256
    d = P.desc(GRID["origin"], GRID["spacing"], count)
    vol = P.fabricated_volume(count, 9)
    pts = P.sample_points(d, n, 7, nonfinite=True)
    want = P.sample(d, vol, pts)
    dev = torch.device("cuda", 0)
    out = torch.full((n + 256, 4), 7.0, dtype=torch.float32, device=dev)
    tvol, tp = torch.from_numpy(vol).to(dev), torch.from_numpy(pts).to(dev)
    torch.cuda.synchronize()
    dd = P.abi_desc(GRID["origin"], GRID["spacing"], count, flags=abi.PROBES_DEVICE_ARRAYS)
    assert device.lib().hj_sample_probes(pv._h, C.byref(dd), tvol.data_ptr(), tp.data_ptr(), n, out.data_ptr()) == abi.HJ_OK
    assert_bits(out[:n].cpu().numpy(), want, f"n = {n}")
    assert (out[n:] == 7.0).all(), "written beyond n"
    finite = np.isfinite(pts[:, 0:3]).all(1)
    got = pv.sample_probes(vol, GRID["origin"], GRID["spacing"], pts[finite])
    assert_bits(got, want[finite], f"n = {int(finite.sum())}, host arrays")


def test_a_refused_call_writes_nothing(pv):
    """With a live context, on the device route: every kind of refusal leaves the tensors as they were; the context's text.  The
    look-up and the points need no scene; the bake without one is a state error."""
    import torch
    L = device.lib()
    dev = torch.device("cuda", 0)
    vol = torch.full((8, 28), 7.0, dtype=torch.float32, device=dev)
    pts = torch.full((64, 8), 7.0, dtype=torch.float32, device=dev)
    out = torch.full((64, 4), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    DEV = abi.PROBES_DEVICE_ARRAYS
    for dkw in (dict(flags=DEV | 2), dict(count=(2, 2, 0), flags=DEV), dict(origin=(0, float("nan"), 0), flags=DEV), dict(spacing=(1, -1, 1), flags=DEV),
                dict(min_distance=-1.0, flags=DEV)):
        dd = P.abi_desc(**dkw)
        for rc in (L.hj_sample_probes(pv._h, C.byref(dd), vol.data_ptr(), pts.data_ptr(), 64, out.data_ptr()),
                   L.hj_probe_points(pv._h, C.byref(dd), pts.data_ptr()), L.hj_bake_probes(pv._h, C.byref(dd), 1, None, vol.data_ptr(), None)):
            assert rc == abi.HJ_ERR_INVALID and b"hj_" in L.hj_last_error(pv._h)
    dd = P.abi_desc(flags=DEV)
    assert L.hj_sample_probes(pv._h, C.byref(dd), vol.data_ptr(), pts.data_ptr() + 4, 63, out.data_ptr()) == abi.HJ_ERR_INVALID
    assert L.hj_sample_probes(pv._h, C.byref(dd), vol.data_ptr(), None, 64, out.data_ptr()) == abi.HJ_ERR_INVALID
    assert L.hj_bake_probes(pv._h, C.byref(dd), 0, None, vol.data_ptr(), None) == abi.HJ_ERR_INVALID
    assert L.hj_sample_probes(pv._h, C.byref(dd), None, None, 0, None) == abi.HJ_OK                 # n == 0: nothing to do
    host = np.full((64, 8), 7.0, F)
    host[5, 3:6] = 0
    hout = np.full((64, 4), 7.0, F)
    hd = P.abi_desc()
    assert L.hj_sample_probes(pv._h, C.byref(hd), np.zeros((8, 28), F).ctypes.data, host.ctypes.data, 64, hout.ctypes.data) == abi.HJ_ERR_INVALID
    assert b"point 5" in L.hj_last_error(pv._h) and (hout == 7.0).all()
    with device.Renderer(0) as r:                                      # no scene
        assert L.hj_bake_probes(r._h, C.byref(dd), 1, None, vol.data_ptr(), None) == abi.HJ_ERR_STATE and b"scene" in L.hj_last_error(r._h)
        good = r.sample_probes(np.ones((1, 1, 1, 28), F), (0, 0, 0), (1, 1, 1), np.array([[0, 0, 0, 0, 0, 1, 0, 0]], F))
        assert good.shape == (1, 4) and good[0, 3] == 1.0
    torch.cuda.synchronize()
    assert (vol == 7.0).all() and (pts == 7.0).all() and (out == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------ end to end

def test_bake_then_sample_end_to_end(pv):
    """cbox: a (5, 4, 3) volume baked at spp 4 and sampled at the gather tests' point set - surface points with their normals, free
    points, scaled and axis normals - equals probe_ref.sample of the GPU's own volume.  (No closeness to the hemisphere gather is
    asserted: order-2 truncation plus 4-spp noise gives no derivable bound.)"""
    cs = R.scene("cbox")
    pv.upload_scene(cs)
    d = P.grid_in_domain(cs, (5, 4, 3), min_distance=0.02)
    vol = pv.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE, min_distance=0.02), spp=4, opts=R.options(40), device=True)
    pts = G.point_set("cbox")
    import torch
    got = pv.sample_probes(vol, d["origin"], d["spacing"], torch.from_numpy(pts.copy()).to(vol.device))
    host_vol = vol.cpu().numpy()
    want = P.sample(d, host_vol, pts)
    assert_bits(got.cpu().numpy(), want, "sample of the baked volume, device arrays")
    assert_bits(pv.sample_probes(host_vol, d["origin"], d["spacing"], pts), want, "sample of the baked volume, host arrays")
    print("irradiance: mean", want[:, 0:3].mean(0).tolist(), "valid weight: min", float(want[:, 3].min()), "zero at", int((want[:, 3] == 0).sum()))
    assert np.isfinite(want).all() and (want[:, 3] > 0).any()
