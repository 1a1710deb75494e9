"""hj_trace_rays on the GPU: caller-given rays through the uploaded tree, against the oracle bit for bit - ids, the bits of t, u, v
and the 14 floats of the populated intersection - on every ray of each set (none is skipped); any-hit against the oracle's boolean;
sizes, segment sizes, chunk sizes and the two kernel forms against each other; device arrays against host arrays; the routes into an
upload; the context's state around a query."""
import ctypes as C
import functools

import numpy as np
import pytest

import scenes
import update_scenes as U
from refit_scenes import refit_numpy, shape_boxes
from hijiki_amd import abi, device, host
from oracle import hj_oracle as O

pytestmark = pytest.mark.gpu

C_FLOAT_P = C.POINTER(C.c_float)


def bits(a):
    """the words of a float32 (or int32) array"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(np.uint32)


def _cbox():
    return host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=1280).compile()


SCENES = {"cbox": _cbox, "rich": lambda: scenes.rich_scene(7), "cluster": lambda: scenes.random_cluster_scene(77),
          "nasty": lambda: scenes.nasty_scene(3)}


# master seed of the logged frames: the first one (of 0, 1, 2, ...) at which the 32 x 32, 2 spp frame of the cluster scene holds a ray
# outside general position (found with the oracle alone; check_case asserts it)
FRAME_SEED = 16


def ray_set(cs, seed=5):
    """Every ray the oracle logs for one 32 x 32, 2 spp frame of `cs` (all bounces, shadow windows, the directions the reference's
    arithmetic leaves: not unit vectors), 20 000 seeded random rays with shadow-style windows, and the edge cases: rays that miss
    everything, NaN directions, and for 64 rays of the set that hit: tMin == tMax == t of the hit, and tMax one float short of it."""
    log = O.logged_rays(cs, host.make_blocks(32, 32, 2, FRAME_SEED))
    r = np.random.default_rng(seed)
    n = 20000
    rnd = np.zeros((n, 8), np.float32)
    rnd[:, 0:3] = np.stack([r.uniform(-0.95, 0.95, n), r.uniform(0.05, 1.5, n), r.uniform(-1.0, 0.95, n)], 1)
    d = r.normal(size=(n, 3))
    rnd[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rnd[:, 6], rnd[:, 7] = 2e-4, r.uniform(0.1, 3.0, n)
    base = np.ascontiguousarray(np.concatenate([log[:, 0:8], rnd]))
    away = np.zeros((8, 8), np.float32)                               # from far outside, pointing away
    away[:, 0:3] = [1.0e4, 2.0e4, -3.0e4]
    away[:, 3:6] = r.uniform(0.1, 1.0, (8, 3)) * [1, 1, -1]
    away[:, 6], away[:, 7] = 1e-4, np.inf
    nan = base[:4].copy()
    nan[0, 3], nan[1, 4], nan[2, 5], nan[3, 3:6] = np.nan, np.nan, np.nan, np.nan
    oi, ot, _, _ = O.intersect(cs, base)
    hit = np.nonzero((oi >= 0) & np.isfinite(ot))[0][:: max(1, int((oi >= 0).sum()) // 64)][:64]
    pinned = base[hit].copy()
    pinned[:, 6] = pinned[:, 7] = ot[hit]
    short = base[hit].copy()
    short[:, 7] = np.nextafter(ot[hit], np.float32(-np.inf))
    return np.ascontiguousarray(np.concatenate([base, away, nan, pinned, short])), len(log)


@functools.lru_cache(maxsize=None)
def case(name):
    """(compiled scene, rays, the oracle's (ids, t, u, v, full) for them, number of logged rays): computed once, never written to"""
    cs = SCENES[name]()
    rays, n_log = ray_set(cs)
    want = O.intersect(cs, rays, full=True)
    for a in (rays,) + want:
        a.setflags(write=False)
    return cs, rays, want, n_log


def kinds(cs, ids):
    """hits per shape kind (spheres, quads, triangles) and misses"""
    ns, nq = len(cs.spheres), len(cs.quads)
    return (int(((ids >= 0) & (ids < ns)).sum()), int(((ids >= ns) & (ids < ns + nq)).sum()), int((ids >= ns + nq).sum()),
            int((ids < 0).sum()))


def assert_covers(cs, ids):
    """every shape kind the scene has is hit, and something is missed"""
    sph, quad, tri, miss = kinds(cs, ids)
    assert (sph > 0) == (len(cs.spheres) > 0) and (quad > 0) == (len(cs.quads) > 0) and (tri > 0) == (len(cs.triangles) > 0), (sph, quad, tri)
    assert sph + quad + tri > 1000 and miss > 100
    return sph, quad, tri, miss


def assert_hits(got, want, what):
    gi, gt, gu, gv = got[:4]
    oi, ot, ou, ov = want[:4]
    bad = (gi != oi) | (bits(gt) != bits(ot)) | (bits(gu) != bits(ou)) | (bits(gv) != bits(ov))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(oi)} hit records differ, first at ray {int(np.argmax(bad))}"


def assert_surface(cs, got, want, what):
    """the 14 floats of the oracle's full record as uint32, the material word, the last word; a miss: 16 zero words"""
    ids, surf, full = want[0], bits(got[4]), bits(want[4])
    bad = (surf[:, :14] != full[:, :14]).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(ids)} surface records differ, first at ray {int(np.argmax(bad))}"
    hit = ids >= 0
    assert (surf[hit, 14] == cs.materials[ids[hit]]).all(), f"{what}: material words"
    assert (surf[:, 15] == 0).all() and (surf[~hit] == 0).all(), f"{what}: words that must be 0"


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as ctx:
        yield ctx


_default = {}


def default_results(rq, name):
    """closest hit + surface and any-hit records of case `name` from the module's context (default switches, host arrays)"""
    if name not in _default:
        cs, rays, _, _ = case(name)
        rq.upload_scene(cs)
        _default[name] = (rq.trace_rays(rays, surface=True), rq.trace_rays(rays, any_hit=True))
    else:
        rq.upload_scene(case(name)[0])
    return _default[name]


def check_case(name):
    """the set exercises what it claims, by the oracle's own answers: every shape kind the scene has is hit, something is missed, the
    edge cases do what they say"""
    cs, rays, want, n_log = case(name)
    oi = want[0]
    sph, quad, tri, miss = assert_covers(cs, oi)
    assert np.isfinite(rays[:n_log, 7]).sum() > 500                            # shadow windows among the logged rays
    if name in ("rich", "cluster"):                                            # ... and directions the reference never re-normalised
        assert (np.abs(np.linalg.norm(rays[:n_log, 3:6].astype(np.float64), axis=1) - 1.0) > 0.01).any()
    base = len(rays) - 8 - 4 - 128
    assert (oi[base:base + 8] == -1).all()                                     # the rays that leave the scene
    assert np.isnan(rays[base + 8:base + 12, 3:6]).any(axis=1).all()
    assert (oi[base + 12:base + 76] >= 0).sum() > 0                            # tMin == tMax == t still finds a hit
    if name == "cluster":                                                      # a ray outside general position: the second tree is walked
        assert (rays[:n_log, 3:6] == 0).any(), "no logged ray of the cluster scene has an exact-zero direction component"
    return sph, quad, tri, miss


@pytest.mark.parametrize("name", list(SCENES))
def test_every_ray_matches_the_oracle(rq, name):
    cs, rays, want, n_log = case(name)
    oi = want[0]
    sph, quad, tri, miss = check_case(name)
    closest, anyhit = default_results(rq, name)
    print(f"{name}: {len(rays)} rays ({n_log} logged), hits on spheres / quads / triangles {sph} / {quad} / {tri}, {miss} misses")
    assert_hits(closest, want, name)
    assert_surface(cs, closest, want, name)
    ai, at, au, av = anyhit
    assert ((ai >= 0) == (oi >= 0)).all(), f"{name}: any-hit booleans"
    assert (ai[ai < 0] == -1).all() and (bits(at)[ai < 0] == 0).all() and (bits(au)[ai < 0] == 0).all() and (bits(av)[ai < 0] == 0).all()


def test_surface_with_any_hit_is_refused(rq):
    cs, rays, _, _ = case("cbox")
    rq.upload_scene(cs)
    with pytest.raises(ValueError):
        rq.trace_rays(rays[:8], any_hit=True, surface=True)
    hits, surf = np.zeros((8, 4), np.float32), np.zeros((8, 16), np.float32)
    L = device.lib()
    assert L.hj_trace_rays(rq._h, rays.ctypes.data, 8, abi.TRACE_ANY_HIT, hits.ctypes.data, surf.ctypes.data) == abi.HJ_ERR_INVALID
    assert b"surface" in L.hj_last_error(rq._h)
    assert L.hj_trace_rays(rq._h, rays.ctypes.data, 0, 0, None, None) == abi.HJ_OK       # n == 0: nothing to do


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_sizes(rq, n):
    cs, rays, want, _ = case("cbox")
    rq.upload_scene(cs)
    got = rq.trace_rays(rays[:n], surface=True)
    cut = tuple(a[:n] for a in want)
    assert_hits(got, cut, f"n = {n}")
    assert_surface(cs, got, cut, f"n = {n}")
    ai, *_ = rq.trace_rays(rays[:n], any_hit=True)
    assert ((ai >= 0) == (cut[0] >= 0)).all()


@pytest.mark.parametrize("name", ["cbox", "cluster"])
@pytest.mark.parametrize("switch", ["HJ_TRACE_WG_RAYS=64", "HJ_TRACE_WG_RAYS=100", "HJ_TRACE_PERSISTENT=0", "HJ_TRACE_CHUNK=1000"])
def test_scheduling_never_shows_in_a_result(rq, monkeypatch, name, switch):
    """Segments of 64 and of 100 rays (many workgroups, ragged last segments, segments that are no multiple of a wave), launches of
    1000 rays, and the plain kernel form: a context created under the setting returns the bits of the default one in all four hit
    arrays - any-hit records included - and in the surface records."""
    cs, rays, _, _ = case(name)
    closest, anyhit = default_results(rq, name)
    monkeypatch.setenv(*switch.split("="))
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        got, got_any = r.trace_rays(rays, surface=True), r.trace_rays(rays, any_hit=True)
    for k in range(4):
        assert (bits(got[k]) == bits(closest[k])).all(), (switch, "closest", k)
        assert (bits(got_any[k]) == bits(anyhit[k])).all(), (switch, "any-hit", k)
    assert (bits(got[4]) == bits(closest[4])).all(), (switch, "surface")


def test_device_arrays(rq):
    import torch
    cs, rays, _, _ = case("rich")
    closest, anyhit = default_results(rq, "rich")
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(rays.copy()).to(dev)
    keep = t.clone()
    got, got_any = rq.trace_rays(t, surface=True), rq.trace_rays(t, any_hit=True)
    assert all(isinstance(a, torch.Tensor) and a.device == dev for a in got + got_any)
    assert got[0].dtype == torch.int32 and got[4].shape == (len(rays), 16)
    assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), "the ray tensor changed"
    for k in range(5):
        assert (bits(got[k].cpu().numpy()) == bits(closest[k])).all(), ("closest", k)
    for k in range(4):
        assert (bits(got_any[k].cpu().numpy()) == bits(anyhit[k])).all(), ("any-hit", k)
    assert (got[0].cpu().numpy() == closest[0]).all()
    # refused before any launch: the host, another GPU, another dtype, a tensor with gaps, another shape
    bad = [t.cpu(), t.double(), t[::2], t[:, :7].contiguous(), t.reshape(-1)]
    if torch.cuda.device_count() > 1:
        bad.append(t.to(torch.device("cuda", 1)))
    for b in bad:
        with pytest.raises(ValueError):
            rq.trace_rays(b)
    empty = rq.trace_rays(t[:0], surface=True)
    assert [tuple(a.shape) for a in empty] == [(0,), (0,), (0,), (0,), (0, 16)]


def test_tree_built_on_the_device_and_left_there(rq):
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile()
    rays = case("cbox")[1]
    rq.build_bvh(cs, keep_on_device=True)
    cs.set_bvh(rq.read_device_bvh())                                          # the oracle walks the same tree
    rq.upload_scene(cs, device_tree=True)
    want = O.intersect(cs, rays, full=True)
    assert_covers(cs, want[0])
    got = rq.trace_rays(rays, surface=True)
    assert_hits(got, want, "device-built tree")
    assert_surface(cs, got, want, "device-built tree")
    ai, *_ = rq.trace_rays(rays, any_hit=True)
    assert ((ai >= 0) == (want[0] >= 0)).all()


def test_after_an_update_with_moved_shapes(rq):
    rest, moved = U.light_show(), U.light_show(moved=True)
    moved.set_bvh(refit_numpy(rest.bvh.copy(), shape_boxes(moved)))
    rays, _ = ray_set(moved)
    want = O.intersect(moved, rays, full=True)
    assert min(assert_covers(moved, want[0])) > 0                             # (spheres, quads and triangles)
    rq.upload_scene(rest)
    before = rq.trace_rays(rays)
    rq.update_shapes(moved)
    got = rq.trace_rays(rays, surface=True)
    assert (got[0] != before[0]).any()
    assert_hits(got, want, "moved shapes")
    assert_surface(moved, got, want, "moved shapes")
    ai, *_ = rq.trace_rays(rays, any_hit=True)
    assert ((ai >= 0) == (want[0] >= 0)).all()


def test_state_around_a_query():
    """Refused with the probes' status while a frame submitted with HJ_RENDER_NO_DRAIN is in flight, fine after hj_pipeline_wait; a
    frame rendered before and after a query is the same frame: the query leaves nothing behind."""
    cs, rays, want, _ = case("cbox")
    W, H = 96, 64
    L = device.lib()
    with device.Renderer(0) as r:
        hits = np.zeros((64, 4), np.float32)
        assert L.hj_trace_rays(r._h, rays.ctypes.data, 64, 0, hits.ctypes.data, None) == abi.HJ_ERR_STATE      # no scene yet
        assert b"scene" in L.hj_last_error(r._h)
        r.upload_scene(cs)
        r.create_framebuffer(W, H)
        r.render_frame(2, 9)
        first = r.read().copy()
        r.clear()
        r.submit_frame(2, 9)
        assert L.hj_trace_rays(r._h, rays.ctypes.data, 64, 0, hits.ctypes.data, None) == abi.HJ_ERR_STATE
        assert b"NO_DRAIN" in L.hj_last_error(r._h) and (hits == 0).all()
        assert L.hj_debug_trace(r._h, rays.ctypes.data_as(C_FLOAT_P), 64, 1, 0, hits.ctypes.data_as(C_FLOAT_P)) == abi.HJ_ERR_STATE
        r.pipeline_wait(keep=0)
        assert (bits(r.read()) == bits(first)).all()
        got = r.trace_rays(rays[:4097], surface=True)
        assert_hits(got, tuple(a[:4097] for a in want), "after the drain")
        r.clear()
        r.render_frame(2, 9)
        assert (bits(r.read()) == bits(first)).all(), "a frame after a query differs from the frame before it"


def test_agrees_with_the_probe(rq):
    cs, rays, _, _ = case("cbox")
    closest, anyhit = default_results(rq, "cbox")
    probe, probe_any = rq.trace(rays), rq.trace(rays, any_hit=True)
    for k in range(4):
        assert (bits(probe[k]) == bits(closest[k])).all(), ("closest", k)
        assert (bits(probe_any[k]) == bits(anyhit[k])).all(), ("any-hit", k)

