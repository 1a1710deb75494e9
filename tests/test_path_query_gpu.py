"""hj_trace_paths on the GPU: the radiance along caller-given rays against the oracle bit for bit - all 8 words of every record of
every set (none is skipped), and the statistics against the reference's counts: a block's camera rays against hjo_integrate_block
and hj_debug_samples; arbitrary rays on four scenes and two bounce caps against path_query_ref.compose; pool, workgroup count, chunk
size and prefix length against each other; spp; the light-shaft grid; device arrays; the context's state around a query; a query
after hj_scene_update_shapes."""
import numpy as np
import pytest

import path_query_ref as R
import update_scenes
from refit_scenes import refit_numpy, shape_boxes
from hijiki_amd import abi, device
from oracle import hj_oracle as O

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
COUNTS = ("paths", "closest_rays", "shadow_rays", "hits", "unoccluded_shadow_rays")


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(U)


def assert_samples(got, want, what):
    bad = (bits(got) != bits(want)).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(want)} records differ, first at ray {i}:\n  gpu  {got[i].tolist()}\n  want {want[i].tolist()}")


def assert_counts(stats, counts, what):
    assert {k: stats[k] for k in COUNTS} == {k: counts[k] for k in COUNTS}, what


@pytest.fixture(scope="module")
def pq():
    with device.Renderer(0) as ctx:
        yield ctx


_default = {}


def default_result(pq, name="cbox"):
    """(samples, statistics) of the scene's ray set from the module's context: default switches, host arrays, max_bounces = 40"""
    pq.upload_scene(R.scene(name))
    if name not in _default:
        _default[name] = pq.trace_paths(R.ray_set(name), opts=R.options(40), stats=True)
        _default[name][0].setflags(write=False)
    return _default[name]


@pytest.mark.parametrize("name", ["cbox", "env"])
def test_camera_rays_are_the_integrator(pq, name):
    cs, block, o = R.scene(name), R.camera_block(), R.options(40)
    want, ctr = O.integrate_block(cs, block, o)
    pq.upload_scene(cs)
    got, stats = pq.trace_paths(R.camera_rays(cs, block), opts=o, stats=True)
    assert_samples(got, want.reshape(-1, 8), f"{name}: camera rays against the oracle")
    assert_samples(got, pq.samples(block, o).reshape(-1, 8), f"{name}: camera rays against hj_debug_samples")
    assert (stats["paths"], stats["closest_rays"], stats["shadow_rays"], stats["hits"]) == \
           (ctr["paths"], ctr["closest_calls"], ctr["shadow_calls"], ctr["hits"])
    assert stats["batches"] == 1 and stats["total_ms"] > 0 and stats["bounce_rounds"] == 0 and stats["path_launches"] == 0


@pytest.mark.parametrize("max_bounces", [40, 5])
@pytest.mark.parametrize("name", list(R.SCENES))
def test_arbitrary_rays_match_the_reference(pq, name, max_bounces):
    want, counts, _ = R.expected(name, max_bounces)
    if max_bounces == 40:
        got, stats = default_result(pq, name)
    else:
        pq.upload_scene(R.scene(name))
        got, stats = pq.trace_paths(R.ray_set(name), opts=R.options(max_bounces), stats=True)
    print(f"{name}, max_bounces {max_bounces}: {counts}")
    assert_samples(got, want, f"{name}, max_bounces {max_bounces}")
    assert_counts(stats, counts, f"{name}, max_bounces {max_bounces}")
    assert (got[:, 3] == 1.0).all()


@pytest.mark.parametrize("switch", ["HJ_PATHS_POOL=64 HJ_PATHS_WGS=1", "HJ_PATHS_POOL=128 HJ_PATHS_WGS=3", "HJ_PATHS_CHUNK=1000"])
def test_scheduling_never_shows_in_a_result(pq, monkeypatch, switch):
    """One workgroup of 64 positions (dozens of top-ups, and the one-wave tail), three of 128, launches of 1000 samples: a context
    created under the setting returns the bits of the default one, and the same counts."""
    want, want_stats = default_result(pq)
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(R.scene("cbox"))
        got, stats = r.trace_paths(R.ray_set("cbox"), opts=R.options(40), stats=True)
    assert_samples(got, want, switch)
    assert_counts(stats, want_stats, switch)
    assert stats["batches"] == (4 if "CHUNK" in switch else 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_prefixes(pq, n):
    want, _ = default_result(pq)
    got = pq.trace_paths(R.ray_set("cbox")[:n], opts=R.options(40))
    assert_samples(got, want[:n], f"n = {n}")


def test_state_regrows_on_a_live_context(monkeypatch):
    """One context, six queries whose path state differs in what it must hold; every result is the reference's prefix word for word
    (record k depends on ray k alone: its own seed).  cbox, all rays: the positions, no miss bin, no ext[].  env (environment and
    tinted glass), 64 rays: fewer positions, but the miss bin and ext[] - "positions suffice" must still reallocate.  cbox, 65 rays:
    the larger layout is kept.  One workgroup of 128 positions, then two of 64: the same positions, another workgroup count.  env, all
    rays, with the counts.  Last, beyond HJ_PATHS_WGS of every earlier step: the per-workgroup arrays regrow."""
    want = {name: R.expected(name, 40)[0] for name in ("cbox", "env")}
    o = R.options(40)
    with device.Renderer(0) as r:
        def query(name, n, what, switches=""):
            for kv in switches.split():
                monkeypatch.setenv(*kv.split("="))
            r.upload_scene(R.scene(name))                                                  # (an upload re-reads the switches)
            got, stats = r.trace_paths(R.ray_set(name)[:n], opts=o, stats=True)
            assert_samples(got, want[name][:n], what)
            return stats
        stats = query("cbox", R.N_RAYS, "cbox, all rays")
        assert_counts(stats, R.expected("cbox", 40)[1], "cbox, all rays")
        query("env", 64, "env[:64] after cbox: miss bin and ext[] on fewer positions")
        query("cbox", 65, "cbox[:65] in the larger layout")
        query("cbox", 200, "one workgroup of 128 positions", "HJ_PATHS_WGS=1 HJ_PATHS_POOL=128")
        query("cbox", 200, "two workgroups of 64 positions", "HJ_PATHS_WGS=2 HJ_PATHS_POOL=64")
        stats = query("env", R.N_RAYS, "env, all rays")
        assert_counts(stats, R.expected("env", 40)[1], "env, all rays")
        query("cbox", 200, "more workgroups allowed than ever allocated for", "HJ_PATHS_WGS=4096 HJ_PATHS_POOL=64")


def test_samples_per_ray(pq):
    """500 rays at spp = 4: the reference's sum, and the in-order float32 sum of four spp = 1 calls with seeds + k (the ray seeded
    0xFFFFFFFE wraps); word 3 is 4.0."""
    cs, rays, o = R.scene("cbox"), R.ray_set("cbox")[:500], R.options(40)
    assert rays.view(U)[1, 6] == 0xFFFFFFFE
    pq.upload_scene(cs)
    want, counts = R.compose(cs, rays, 4, o)
    got, stats = pq.trace_paths(rays, spp=4, opts=o, stats=True)
    assert_samples(got, want, "spp = 4")
    assert_counts(stats, counts, "spp = 4")
    assert stats["paths"] == 2000 and (got[:, 3] == 4.0).all()
    seeds = rays.view(U)[:, 6].copy()
    total = np.zeros((500, 3), F)
    for k in range(4):
        one = pq.trace_paths(rays, seeds=seeds + U(k), opts=o)
        total = total + one[:, 0:3]
        assert (bits(one[:, 4:8]) == bits(got[:, 4:8])).all()
    assert (bits(total) == bits(got[:, 0:3])).all()
    assert (rays.view(U)[:, 6] == seeds).all()


def test_light_grid_changes_no_bit(pq):
    """On the cbox the default and HJ_RENDER_NO_LIGHT_GRID give the same bits; the grid answers some next-event samples, and the
    other counts are equal."""
    with_grid, s1 = default_result(pq)
    without, s0 = pq.trace_paths(R.ray_set("cbox"), opts=R.options(40, grid=False), stats=True)
    assert_samples(without, with_grid, "HJ_RENDER_NO_LIGHT_GRID")
    assert s1["shadow_rays_proven_free"] > 0 and s0["shadow_rays_proven_free"] == 0
    assert_counts(s0, s1, "counts with and without the grid")


def test_device_arrays(pq):
    import torch
    want, want_stats = default_result(pq, "rich")
    rays = R.ray_set("rich")
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(rays.copy()).to(dev)
    keep = t.clone()
    got, stats = pq.trace_paths(t, opts=R.options(40), stats=True)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.shape == (len(rays), 8)
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the ray tensor changed"
    assert_samples(got.cpu().numpy(), want, "device arrays")
    assert_counts(stats, want_stats, "device arrays")
    seeds = torch.from_numpy(rays.view(np.int32)[:, 6].copy()).to(dev)
    zeroed = t.clone()
    zeroed.view(torch.int32)[:, 6] = 0
    zkeep = zeroed.clone()
    got2 = pq.trace_paths(zeroed, seeds=seeds, opts=R.options(40))
    assert torch.equal(zeroed.view(torch.int32), zkeep.view(torch.int32)), "seeds were written into the caller's tensor"
    assert_samples(got2.cpu().numpy(), want, "device arrays with seeds")
    bad = [t.cpu(), t.double(), t[::2], t[:, :7].contiguous(), t.reshape(-1)]
    for b in bad:
        with pytest.raises(ValueError):
            pq.trace_paths(b)
    with pytest.raises(ValueError):
        pq.trace_paths(t, seeds=seeds.cpu())
    assert tuple(pq.trace_paths(t[:0]).shape) == (0, 8)


def test_state_around_a_query():
    """No scene and a frame in flight are HJ_ERR_STATE; a frame rendered before and after a query is the same frame - the query
    borrows nothing of the batch slots and leaves the framebuffer alone -; hj_trace_rays still answers as before."""
    cs, rays = R.scene("cbox"), R.ray_set("cbox")
    want, _, _ = R.expected("cbox", 40)
    W, H = 96, 64
    L = device.lib()
    with device.Renderer(0) as r:
        out = np.zeros((64, 8), F)
        assert L.hj_trace_paths(r._h, rays.ctypes.data, 64, 1, None, 0, out.ctypes.data, None) == abi.HJ_ERR_STATE     # no scene yet
        assert b"scene" in L.hj_last_error(r._h) and (out == 0).all()
        r.upload_scene(cs)
        r.create_framebuffer(W, H)
        probe = rays.copy()
        probe[:, 6], probe[:, 7] = 1e-4, np.inf
        hits_before = r.trace_rays(probe, surface=True)
        r.render_frame(2, 9)
        first = r.read().copy()
        got = r.trace_paths(rays, opts=R.options(40))
        assert_samples(got, want, "between two frames")
        assert (bits(r.read()) == bits(first)).all(), "the query touched the framebuffer"
        r.clear()
        r.render_frame(2, 9)
        assert (bits(r.read()) == bits(first)).all(), "a frame after a query differs from the frame before it"
        hits_after = r.trace_rays(probe, surface=True)
        for a, b in zip(hits_before, hits_after):
            assert (bits(a) == bits(b)).all()
        r.clear()
        r.render_frame_async(2, 9)
        rc = L.hj_trace_paths(r._h, rays.ctypes.data, 64, 1, None, 0, out.ctypes.data, None)
        text = L.hj_last_error(r._h)
        r.sync()
        assert rc == abi.HJ_ERR_STATE and b"asynchronous" in text and (out == 0).all()
        assert (bits(r.read()) == bits(first)).all()
        assert L.hj_trace_paths(r._h, None, 0, 1, None, 0, None, None) == abi.HJ_OK                                      # n == 0: nothing to do


def test_after_an_update_with_moved_shapes(pq):
    rest, moved = update_scenes.light_show(triangles=150), update_scenes.light_show(moved=True, triangles=150)
    moved.set_bvh(refit_numpy(rest.bvh.copy(), shape_boxes(moved)))
    rng = np.random.default_rng(4)
    lo, hi = R.domain(moved)
    lo, hi = np.maximum(lo, [-1.2, 0.0, -1.2]), np.minimum(hi, [1.2, 2.0, 1.2])           # (inside the scene's box of quads)
    n = 1000
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays.view(U)[:, 6] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    o = R.options(40)
    want, counts = R.compose(moved, rays, 1, o)
    assert counts["hits"] > 1000 and counts["unoccluded_shadow_rays"] > 100
    pq.upload_scene(rest)
    before = pq.trace_paths(rays, opts=o)
    pq.update_shapes(moved)
    got, stats = pq.trace_paths(rays, opts=o, stats=True)
    assert (bits(got) != bits(before)).any()
    assert_samples(got, want, "moved shapes")
    assert_counts(stats, counts, "moved shapes")
