"""hj_trace_paths_adaptive on the GPU: all 8 words of every record, every n_i, the moments and the counts against
path_adaptive_ref.expected bit for bit on four scenes (no ray is skipped); the headline invariant on the GPU alone - a ray's record
is hj_trace_paths' for that ray at spp = n_i; the two ends of rel_error; pool, workgroup count, chunk size, ray order and prefix
length against each other; a short last round; device tensors; the context's state around a query; a query after
hj_scene_update_shapes."""
import numpy as np
import pytest

import path_adaptive_ref as A
import path_query_ref as R
import update_scenes
from refit_scenes import refit_numpy, shape_boxes
from hijiki_amd import device
from test_path_query_gpu import assert_counts, assert_samples, bits

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
KW = A.aopts()                                     # 4 / +4 / 16, rel_error 0.5, floor 0.01: test_path_adaptive_host.py proves the spread


@pytest.fixture(scope="module")
def pa():
    with device.Renderer(0) as ctx:
        yield ctx


_default = {}


def default_result(pa, name="cbox"):
    """(samples, moments, statistics) of the scene's ray set from the module's context: default switches, host arrays, KW"""
    pa.upload_scene(R.scene(name))
    if name not in _default:
        _default[name] = pa.trace_paths_adaptive(R.ray_set(name), opts=R.options(40), stats=True, moments=True, **KW)
        _default[name][0].setflags(write=False)
        _default[name][1].setflags(write=False)
    return _default[name]


def assert_moments(got, want, what):
    bad = (bits(got) != want).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(want)} moment records differ, first at ray {i}:\n  gpu  {bits(got)[i].tolist()}\n  want {want[i].tolist()}")


def assert_result(got, e, what):
    samples, moments, stats = got
    print(f"{what}: n_i {np.bincount(e['n']).nonzero()[0].tolist()} x {np.bincount(e['n'])[np.bincount(e['n']).nonzero()[0]].tolist()}, rounds {e['rounds']}, {e['counts']}")
    assert (samples[:, 3] == e["n"]).all(), (what, int((samples[:, 3] != e["n"]).sum()))
    assert_samples(samples, e["samples"], what)
    assert_moments(moments, e["moments"], what)
    assert_counts(stats, e["counts"], what)
    assert stats["paths"] == int(e["n"].sum()) and stats["bounce_rounds"] == e["rounds"]
    assert stats["batches"] >= e["rounds"] and stats["total_ms"] > 0 and stats["path_launches"] == 0


@pytest.mark.parametrize("name", list(R.SCENES))
def test_every_record_matches_the_reference(pa, name):
    assert_result(default_result(pa, name), A.expected_for(name), name)


def test_a_record_is_the_fixed_spp_query_of_its_ray(pa):
    """The headline invariant on the GPU alone: the rays grouped by n_i, trace_paths(spp = n_i) of each group gives the group's
    records, all 8 words."""
    samples, moments, _ = default_result(pa)
    rays, o = R.ray_set("cbox"), R.options(40)
    n_i = bits(moments)[:, 3]
    assert set(n_i.tolist()) == {4, 8, 12, 16}
    for m in (4, 8, 12, 16):
        idx = np.flatnonzero(n_i == m)
        fixed = pa.trace_paths(rays[idx], spp=m, opts=o)
        assert_samples(samples[idx], fixed, f"the {len(idx)} rays of n_i = {m}")


def test_the_two_ends_of_rel_error(pa):
    """A huge rel_error stops every ray after the first round: trace_paths(spp = spp_min), record for record.  rel_error = 0 stops
    a ray before spp_max only when its samples so far have no variance at all (sem2 <= 0: the rays that leave the scene, which see
    nothing); every other ray gets spp_max samples and trace_paths(spp = spp_max)'s record, and the rays without variance their
    trace_paths(spp = n_i) record.  (That the stop rule as written lets a ray of zero variance go at rel_error = 0 follows from its
    `<=`; a ray is compared with the spp_max query exactly when its last sem2 is above 0.)"""
    rays, o = R.ray_set("cbox"), R.options(40)
    default_result(pa)
    lo, hi = pa.trace_paths(rays, spp=4, opts=o), pa.trace_paths(rays, spp=16, opts=o)
    got, stats = pa.trace_paths_adaptive(rays, opts=o, stats=True, **dict(KW, rel_error=1e18))
    assert_samples(got, lo, "rel_error 1e18")
    assert stats["bounce_rounds"] == 1 and stats["paths"] == 4 * len(rays)
    got, mom, stats = pa.trace_paths_adaptive(rays, opts=o, stats=True, moments=True, **dict(KW, rel_error=0.0))
    n_i, sem2 = bits(mom)[:, 3], mom[:, 2]
    full = n_i == 16
    e0 = A.expected_for("cbox", rel_error=0.0)
    print(f"rel_error 0: {int(full.sum())} rays at spp_max, {int((~full).sum())} without variance")
    assert (n_i == e0["n"]).all() and (sem2[~full] == 0).all() and (n_i[-200:] == 4).all() and full.any()
    assert_samples(got[full], hi[full], "rel_error 0, rays with variance")
    for m in sorted(set(n_i[~full].tolist())):
        idx = np.flatnonzero(n_i == m)
        assert_samples(got[idx], pa.trace_paths(rays[idx], spp=m, opts=o), f"rel_error 0, {len(idx)} rays without variance at n_i = {m}")
    assert stats["bounce_rounds"] == 4 and stats["paths"] == int(n_i.sum())


def test_rays_that_leave_the_scene_stop_at_spp_min(pa):
    samples, moments, _ = default_result(pa)
    assert (samples[-200:, 3] == 4.0).all() and (bits(moments)[-200:, 3] == 4).all()
    assert (bits(samples[-200:, 0:3]) == 0).all() and (bits(moments)[-200:, 0:3] == 0).all()


@pytest.mark.parametrize("switch", ["HJ_PATHS_POOL=64 HJ_PATHS_WGS=1", "HJ_PATHS_POOL=128 HJ_PATHS_WGS=3", "HJ_PATHS_CHUNK=1000"])
def test_scheduling_never_shows_in_a_result(pa, monkeypatch, switch):
    """A context created under the setting returns the bits of the default one, the same moments and the same counts.  Launches of
    1000 samples are launches of 250 rays in every round (4 samples a ray): one per 250 rays of each round's list."""
    want, want_mom, want_stats = default_result(pa)
    for kv in switch.split():
        monkeypatch.setenv(*kv.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(R.scene("cbox"))
        got, mom, stats = r.trace_paths_adaptive(R.ray_set("cbox"), opts=R.options(40), stats=True, moments=True, **KW)
    assert_samples(got, want, switch)
    assert_moments(mom, bits(want_mom), switch)
    assert_counts(stats, want_stats, switch)
    assert stats["bounce_rounds"] == want_stats["bounce_rounds"]
    n_i = A.expected_for("cbox")["n"]
    chunked = sum(-(-int((n_i > m).sum()) // 250) for m in (0, 4, 8, 12))
    assert stats["batches"] == (chunked if "CHUNK" in switch else 4)


def test_a_permutation_of_the_rays_permutes_the_result(pa):
    want, want_mom, _ = default_result(pa)
    perm = np.random.default_rng(11).permutation(R.N_RAYS)
    got, mom = pa.trace_paths_adaptive(R.ray_set("cbox")[perm], opts=R.options(40), moments=True, **KW)
    assert_samples(got, want[perm], "permuted rays")
    assert_moments(mom, bits(want_mom)[perm], "permuted rays")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_prefixes(pa, n):
    """the compaction's wave and workgroup edges"""
    want, want_mom, _ = default_result(pa)
    got, mom = pa.trace_paths_adaptive(R.ray_set("cbox")[:n], opts=R.options(40), moments=True, **KW)
    assert_samples(got, want[:n], f"n = {n}")
    assert_moments(mom, bits(want_mom)[:n], f"n = {n}")


def test_a_short_last_round(pa):
    """4 / +5 / 16: rounds of 4, 5, 5 and 2 samples"""
    e = A.expected_for("cbox", 4, 5, 16)
    assert set(e["n"].tolist()) == {4, 9, 14, 16} and e["rounds"] == 4
    pa.upload_scene(R.scene("cbox"))
    got = pa.trace_paths_adaptive(R.ray_set("cbox"), opts=R.options(40), stats=True, moments=True, **A.aopts(4, 5, 16))
    assert_result(got, e, "cbox, 4 / +5 / 16")


def test_device_arrays(pa):
    import torch
    want, want_mom, want_stats = default_result(pa, "rich")
    rays = R.ray_set("rich")
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(rays.copy()).to(dev)
    keep = t.clone()
    got, mom, stats = pa.trace_paths_adaptive(t, opts=R.options(40), stats=True, moments=True, **KW)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.shape == (len(rays), 8) and mom.shape == (len(rays), 4)
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the ray tensor changed"
    assert_samples(got.cpu().numpy(), want, "device arrays")
    assert_moments(mom.cpu().numpy(), bits(want_mom), "device arrays")
    assert_counts(stats, want_stats, "device arrays")
    seeds = torch.from_numpy(rays.view(np.int32)[:, 6].copy()).to(dev)
    zeroed = t.clone()
    zeroed.view(torch.int32)[:, 6] = 0
    zkeep = zeroed.clone()
    got2 = pa.trace_paths_adaptive(zeroed, seeds=seeds, opts=R.options(40), **KW)          # (no moments: NULL)
    assert torch.equal(zeroed.view(torch.int32), zkeep.view(torch.int32)), "seeds were written into the caller's tensor"
    assert_samples(got2.cpu().numpy(), want, "device arrays with seeds, no moments")
    for b in [t.cpu(), t.double(), t[::2], t[:, :7].contiguous(), t.reshape(-1)]:
        with pytest.raises(ValueError):
            pa.trace_paths_adaptive(b)
    assert tuple(pa.trace_paths_adaptive(t[:0]).shape) == (0, 8)


def test_state_around_a_query():
    """A frame rendered before and after a query is the same frame - the query leaves the batch slots and the framebuffer alone -,
    and hj_trace_paths still answers as before."""
    cs, rays = R.scene("cbox"), R.ray_set("cbox")
    e = A.expected_for("cbox")
    W, H = 96, 64
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        r.create_framebuffer(W, H)
        fixed_before = r.trace_paths(rays[:500], spp=2, opts=R.options(40))
        r.render_frame(2, 9)
        first = r.read().copy()
        got = r.trace_paths_adaptive(rays, opts=R.options(40), **KW)
        assert_samples(got, e["samples"], "between two frames")
        assert (bits(r.read()) == bits(first)).all(), "the query touched the framebuffer"
        r.clear()
        r.render_frame(2, 9)
        assert (bits(r.read()) == bits(first)).all(), "a frame after a query differs from the frame before it"
        assert_samples(r.trace_paths(rays[:500], spp=2, opts=R.options(40)), fixed_before, "trace_paths after an adaptive query")


def test_after_an_update_with_moved_shapes(pa):
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
    e = A.expected(moved, rays, KW, o)
    assert len(set(e["n"].tolist())) >= 2
    pa.upload_scene(rest)
    before = pa.trace_paths_adaptive(rays, opts=o, **KW)
    pa.update_shapes(moved)
    got = pa.trace_paths_adaptive(rays, opts=o, stats=True, moments=True, **KW)
    assert (bits(got[0]) != bits(before)).any()
    assert_result(got, e, "moved shapes")
