"""hj_scene_update_shapes on the GPU: an uploaded scene's shapes moved in place.  Records against the numpy refit and the numpy guard
formula word for word (Renderer.scene_tree()), frames against the oracle walking the refitted tree (0 differing bits, equal
counters) and against the old route - refit + upload on a second context."""
import ctypes as C
import time

import numpy as np
import pytest

import fuzz_cases as FZ
import scenes
import update_scenes as U
from refit_scenes import Deformation, refit_numpy, sa_cost, shape_boxes
from hijiki_amd import abi, device, host
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

W, H = 160, 96


@pytest.fixture
def r():
    with device.Renderer(0) as ctx:
        yield ctx


@pytest.fixture
def r2():
    with device.Renderer(0) as ctx:
        yield ctx


def _blocks():
    return host.make_blocks(W, H, 3, 23)


def _frame(r, blocks, opts=None):
    r.create_framebuffer(W, H)
    st = r.render_blocks(blocks, opts)
    return r.read().copy(), st


COUNTERS = ("closest_rays", "shadow_rays", "hits", "unoccluded_shadow_rays", "shadow_rays_proven_free")


def _small(kind=host.SYNTH_CBOX_SPHERES):
    return host.Scene.synthetic(kind, mesh_triangles=1280).compile()


def _mesh_150k(r):
    cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=150000).compile(with_tree=False)
    cs.set_bvh(r.build_bvh(cs))
    return cs


@pytest.mark.parametrize("tree", ["host-compiled", "device-built"])
@pytest.mark.parametrize("route", ["0", "1"])
@pytest.mark.parametrize("kind", [host.SYNTH_CBOX, host.SYNTH_CBOX_SPHERES])
def test_unmoved_update_is_the_identity(r, monkeypatch, kind, route, tree):
    monkeypatch.setenv("HJ_UPLOAD_DEVICE", route)
    cs = _small(kind)
    if tree == "device-built":
        cs.set_bvh(r.build_bvh(cs))
    r.upload_scene(cs)
    before = r.scene_tree()
    mapped, guarded, _ = U.check_records(before, cs, cs.bvh)               # both routes make guards: the numpy formula is the upload's
    assert guarded > 0
    blocks = _blocks()
    f0, st0 = _frame(r, blocks)
    r.update_shapes(cs)
    after = r.scene_tree()
    assert (after["records"] == before["records"]).all() and (after["map"] == before["map"]).all()
    assert all(after[k] == before[k] for k in ("num_nodes", "root", "root2", "num_hot"))
    f1, st1 = _frame(r, blocks)
    assert_same(f1, f0, "unmoved update")
    assert all(st1[k] == st0[k] for k in COUNTERS)


@pytest.mark.parametrize("route", ["0", "1"])
def test_there_and_back(r, monkeypatch, route):
    monkeypatch.setenv("HJ_UPLOAD_DEVICE", route)
    cs = _small()
    r.upload_scene(cs)
    first = r.scene_tree()["records"].copy()
    d = Deformation(cs, seed=5)
    d.apply(0.03, t=0.3)
    r.update_shapes(cs)
    assert (r.scene_tree()["records"] != first).any()
    d.restore()
    r.update_shapes(cs)
    assert (r.scene_tree()["records"] == first).all()


@pytest.mark.parametrize("case", ["small", "mesh-150k", "resident"])
def test_records_after_a_deformation(r, case):
    """resident: the tree a device build left on the device, uploaded with bvh == NULL - the third route into an upload"""
    cs = _mesh_150k(r) if case == "mesh-150k" else _small()
    if case == "resident":
        r.build_bvh(cs, keep_on_device=True)
        topo = r.read_device_bvh().copy()
        r.upload_scene(cs, device_tree=True)
    else:
        topo = cs.bvh.copy()
        r.upload_scene(cs)
    before = r.scene_tree()
    d = Deformation(cs, seed=7)
    for step, amp in enumerate((0.01, 0.03)):
        d.apply(amp, t=0.7 * step)
        cost = r.update_shapes(cs, cost=True)
        tree = r.scene_tree()
        want = refit_numpy(topo, shape_boxes(cs))
        mapped, guarded, widened = U.check_records(tree, cs, want)
        assert (U.links_of(tree["records"]) == U.links_of(before["records"])).all(), "a link word changed"
        assert (tree["map"] == before["map"]).all()
        assert (U.boxes_of(tree["records"]) != U.boxes_of(before["records"])).any()
        assert abs(cost - sa_cost(want)) / sa_cost(want) < 1e-9
        print(f"{case}, step {step}: {len(want)} nodes, {mapped} mapped, {guarded} guarded, {widened} of them with their parent's box")
    if case == "small":
        assert guarded > 0                                                 # host route: guards (and a light-shaft grid)
    elif case == "mesh-150k":
        assert mapped < len(topo) and tree["root2"] > mapped               # device route: collapsed nodes, pair leaves, padding
        # pair nodes: an inner node whose record has the pair mark and whose two leaves have no record; their triangles were
        # gathered again - the frames of test_frames_150k_triangle_mesh walk them
        pair = (tree["records"][tree["map"][:, 0][tree["map"][:, 0] != U.NONE], 3] >> 30) == 3
        assert pair.sum() > 1000, f"{pair.sum()} pair nodes"
    d.restore()


def _animate(r, r2, oracle, cs, amps, seed, flags=0, use_bvh=1, monkeypatch=None):
    """upload once; then per step deform -> update_shapes -> render, against the oracle on the numpy-refitted tree and against refit +
    upload on a second context"""
    topo = cs.bvh.copy()
    blocks = _blocks()
    r.upload_scene(cs)
    d = Deformation(cs, seed=seed)
    o = device.default_opts()
    o.flags = flags
    o.use_bvh = use_bvh
    for step, amp in enumerate(amps):
        d.apply(amp, t=0.9 * step)
        r.update_shapes(cs)
        got, st = _frame(r, blocks, o)
        cs.set_bvh(refit_numpy(topo, shape_boxes(cs)))
        want, ctr, _ = oracle.render_blocks(cs, blocks, W, H, o)
        assert_same(got, want, f"updated scene, step {step}")
        assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"] and st["hits"] == ctr["hits"]
        r2.refit_bvh(cs, topology=topo if step == 0 else None, keep_on_device=True)
        r2.upload_scene(cs, device_tree=True)
        old, st_old = _frame(r2, blocks, o)
        assert_same(got, old, f"update against refit + upload, step {step}")
        assert st["shadow_rays_proven_free"] == st_old["shadow_rays_proven_free"]
    cs.set_bvh(topo)
    d.restore()


@pytest.mark.parametrize("mode", ["default", "split", "no-light-grid", "linear-scan"])
def test_frames_small_scene(r, r2, oracle, mode):
    flags = {"split": abi.RENDER_SPLIT_KERNELS, "no-light-grid": abi.RENDER_NO_LIGHT_GRID}.get(mode, 0)
    _animate(r, r2, oracle, _small(), (0.01, 0.02, 0.03), seed=2, flags=flags, use_bvh=0 if mode == "linear-scan" else 1)


def test_frames_150k_triangle_mesh(r, r2, oracle):
    _animate(r, r2, oracle, _mesh_150k(r), (0.005, 0.01, 0.02), seed=4)


def test_frames_textured_scene_under_an_environment(r, r2, oracle):
    """textures and sky survive the update: the oracle renders the compiled scene with both"""
    import env_scenes
    _animate(r, r2, oracle, env_scenes.mixed_scene(), (0.01, 0.02, 0.03), seed=6)


def test_every_logged_ray_of_an_updated_frame(r, oracle):
    """the oracle's ray log of the deformed cluster scene (rays outside general position: the second copy is walked) through hj_debug_trace"""
    from oracle import hj_oracle as O
    cs = scenes.random_cluster_scene(FZ.source_seed() % 100000)
    topo = cs.bvh.copy()
    r.upload_scene(cs)
    d = Deformation(cs, seed=9)
    d.apply(0.02, t=0.1)
    r.update_shapes(cs)
    cs.set_bvh(refit_numpy(topo, shape_boxes(cs)))
    log = O.logged_rays(cs, host.make_blocks(96, 64, 2, 3))
    rays = np.ascontiguousarray(np.concatenate([log[:, 0:8], FZ.degenerate_rays(np.random.default_rng(1), 20000)]))
    oi, ot, _, _ = O.intersect(cs, rays)
    ids, t, _, _ = r.trace(rays)
    anyhit, *_ = r.trace(rays, any_hit=True)
    bad = int((ids != oi).sum()) + int((t.view(np.uint32) != ot.view(np.uint32))[oi >= 0].sum()) + int(((anyhit >= 0) != (oi >= 0)).sum())
    assert bad == 0, f"{bad} of {len(rays)} rays differ"
    d.restore()


def test_a_guard_that_leaves_its_collapsed_parent_takes_the_parent_s_box(r, monkeypatch):
    """The upload collapses a node only while both children's boxes lie inside its own - a guard's padded box included.  A leaf that
    its sibling covers at rest and that sticks out after the move bounds the refitted parent itself: the padded box is wider than
    the parent's by the padding.  The guard then holds the parent's box, so its test is the test the reference makes of the parent;
    every logged ray of a frame and rays grazing the moved leaf's faces agree with the oracle."""
    from oracle import hj_oracle as O
    monkeypatch.setenv("HJ_UPLOAD_DEVICE", "0")
    rest, moved = U.covered_leaf_scene(), U.covered_leaf_scene(0.9)
    r.upload_scene(rest)
    before = r.scene_tree()
    P, L = 1, 2
    assert before["map"][P, 0] == U.NONE and before["map"][L, 1] != U.NONE, "the case is not built: P kept, or L without a guard"
    assert U.check_records(before, rest, rest.bvh)[2] == 0                  # at rest: the formula's box
    r.update_shapes(moved)
    tree = r.scene_tree()
    assert U.check_records(tree, moved, moved.bvh)[2] == 1
    guard = tree["records"][tree["map"][L, 1]]
    assert (U.boxes_of(guard[None]) == U.boxes_of(moved.bvh[P:P + 1])).all()
    assert moved.bvh_f32[P, 4] == moved.bvh_f32[L, 4] > 1.0                 # ... which ends where L ends, outside S
    log = O.logged_rays(moved, host.make_blocks(96, 64, 2, 3))
    rng = np.random.default_rng(5)
    lo, hi = moved.bvh_f32[L, 0:3], moved.bvh_f32[L, 4:7]
    graze = np.zeros((20000, 8), np.float32)                                # through points on and a float either side of L's box faces
    on = rng.uniform(lo, hi, (len(graze), 3)).astype(np.float32)
    k, side = rng.integers(0, 3, len(graze)), rng.integers(0, 2, len(graze))
    face = np.where(side == 1, hi[k], lo[k]).astype(np.float32)
    step = rng.integers(-1, 2, len(graze))
    face = np.where(step < 0, np.nextafter(face, np.float32(-np.inf)), np.where(step > 0, np.nextafter(face, np.float32(np.inf)), face))
    on[np.arange(len(graze)), k] = face
    org = rng.uniform([-0.9, 0.1, -0.9], [3.0, 1.9, 0.9], (len(graze), 3)).astype(np.float32)
    graze[:, 0:3], graze[:, 3:6] = org, on - org                          # o, d, tMin, tMax
    graze[:, 6], graze[:, 7] = 1e-4, 1e30
    rays = np.ascontiguousarray(np.concatenate([log[:, 0:8], graze]))
    oi, ot, _, _ = O.intersect(moved, rays)
    ids, t, _, _ = r.trace(rays)
    bad = int((ids != oi).sum()) + int((t.view(np.uint32) != ot.view(np.uint32))[oi >= 0].sum())
    assert bad == 0, f"{bad} of {len(rays)} rays differ"
    assert (oi == 2).sum() > 100                                           # the moved leaf is hit at all
    r.update_shapes(rest)                                                  # and back: the formula's box again
    assert (r.scene_tree()["records"] == before["records"]).all()


@pytest.mark.parametrize("arrays", ["host", "device"])
def test_moved_lights_and_a_moved_camera(r, r2, oracle, monkeypatch, arrays):
    """An emissive quad, sphere and triangle moved and rescaled (emitter pdf and cdf with them), the camera 70 units away behind a
    narrow lens: emitters, emit_rec, camera and tan_half_fov are replaced, and the guards' absolute padding follows the new extent
    of root box and camera.  Frame and counters against the oracle and against a fresh upload of the moved scene, records against
    the numpy formula."""
    monkeypatch.setenv("HJ_UPLOAD_DEVICE", "0")
    rest, moved = U.light_show(), U.light_show(moved=True)
    topo = rest.bvh.copy()
    assert (moved.emitters[:, 0] == rest.emitters[:, 0]).all() and (moved.emitters[:, 1] != rest.emitters[:, 1]).all()
    moved.set_bvh(refit_numpy(topo, shape_boxes(moved)))
    f = moved.bvh_f32
    cam = np.array(list(moved.desc.camera.position)[0:3], np.float32)
    assert np.float32(4e-6) * (np.maximum(f[0, 4:7], cam) - np.minimum(f[0, 0:3], cam)).max() > np.float32(2.5e-4)
    blocks = _blocks()
    r.upload_scene(rest)
    f_rest, _ = _frame(r, blocks)
    if arrays == "device":
        import torch
        dev = torch.device("cuda", 0)
        r.update_shapes(moved, device_arrays={k: torch.from_numpy(getattr(moved, k).copy()).to(dev) for k in ("vertices", "spheres", "quads")})
    else:
        r.update_shapes(moved)
    mapped, guarded, _ = U.check_records(r.scene_tree(), moved, moved.bvh)
    assert guarded > 100
    got, st = _frame(r, blocks)
    assert (got != f_rest).any()
    want, ctr, _ = oracle.render_blocks(moved, blocks, W, H)
    assert_same(got, want, "moved lights and camera against the oracle")
    assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"] and st["hits"] == ctr["hits"]
    r2.upload_scene(moved)
    fresh, st_fresh = _frame(r2, blocks)
    assert_same(got, fresh, "moved lights and camera against a fresh upload")
    assert all(st[k] == st_fresh[k] for k in COUNTERS)


@pytest.mark.parametrize("light_grid", [True, False])
def test_device_arrays(r, r2, light_grid):
    import torch
    cs = _small()
    blocks = _blocks()
    r.upload_scene(cs)
    r2.upload_scene(cs)
    d = Deformation(cs, seed=11)
    d.apply(0.03, t=0.4)
    r2.update_shapes(cs)                                                   # host arrays
    want, st_want = _frame(r2, blocks)
    dev = torch.device("cuda", 0)
    arrays = {"vertices": torch.from_numpy(cs.vertices.copy()).to(dev), "spheres": torch.from_numpy(cs.spheres.copy()).to(dev),
              "quads": torch.from_numpy(cs.quads.copy()).to(dev)}
    moved = (cs.vertices.copy(), cs.spheres.copy(), cs.quads.copy())
    d.restore()                                                            # the host arrays are NOT what the update may read
    r.update_shapes(cs, device_arrays=arrays, light_grid=light_grid)
    got, st = _frame(r, blocks)
    assert_same(got, want, "device arrays against host arrays")
    assert all(st[k] == st_want[k] for k in COUNTERS[:4])
    if light_grid:
        assert st["shadow_rays_proven_free"] == st_want["shadow_rays_proven_free"] > 0
    else:
        assert st["shadow_rays_proven_free"] == 0
    assert (r.scene_tree()["records"] == r2.scene_tree()["records"]).all()
    assert all((a.cpu().numpy() == m).all() for a, m in zip((arrays["vertices"], arrays["spheres"], arrays["quads"]), moved))


def test_refusals_leave_the_scene_alone(r):
    cs = _small()
    with pytest.raises(abi.HijikiError) as e:
        r.update_shapes(cs)
    assert e.value.status == abi.HJ_ERR_STATE
    r.upload_scene(cs)
    blocks = _blocks()
    f0, st0 = _frame(r, blocks)
    tree0 = r.scene_tree()["records"].copy()

    def refused(call, status=abi.HJ_ERR_INVALID):
        with pytest.raises(abi.HijikiError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert (r.scene_tree()["records"] == tree0).all()
        f, st = _frame(r, blocks)
        assert_same(f, f0, "after a refused update")
        assert all(st[k] == st0[k] for k in COUNTERS)

    fewer = abi.SceneDesc()
    C.memmove(C.byref(fewer), C.byref(cs.desc), C.sizeof(abi.SceneDesc))
    fewer.num_vertices -= 1
    refused(lambda: r._check(device.lib().hj_scene_update_shapes(r._h, C.byref(fewer), 0, None)))
    refused(lambda: r._check(device.lib().hj_scene_update_shapes(r._h, C.byref(cs.desc), 4, None)))       # unknown flag bit
    d = Deformation(cs, seed=1)
    d.apply(0.02)
    keep = cs.vertices[len(cs.vertices) // 2, 1]
    cs.vertices[len(cs.vertices) // 2, 1] = np.nan
    refused(lambda: r.update_shapes(cs))
    cs.vertices[len(cs.vertices) // 2, 1] = keep
    keep = cs.spheres[0, 3]
    cs.spheres[0, 3] = np.inf
    refused(lambda: r.update_shapes(cs))
    cs.spheres[0, 3] = keep
    d.restore()
    r.submit_frame(2, 1)                                                   # a frame in flight: the upload's busy status
    with pytest.raises(abi.HijikiError) as e:
        r.update_shapes(cs)
    assert e.value.status == abi.HJ_ERR_STATE
    with pytest.raises(abi.HijikiError) as e2:
        r.upload_scene(cs)
    assert e2.value.status == e.value.status
    r.pipeline_wait(0)
    r.update_shapes(cs)
    assert (r.scene_tree()["records"] == tree0).all()


def test_the_refit_s_tree_and_links_are_untouched(r):
    cs = _small()
    other = _small(host.SYNTH_CBOX)
    r.upload_scene(other)
    topo = cs.bvh.copy()
    first = r.refit_bvh(cs, topology=topo)                                 # kept links + a tree on the device
    d = Deformation(other, seed=2)
    d.apply(0.02)
    r.update_shapes(other)
    assert (r.read_device_bvh() == first).all()
    d2 = Deformation(cs, seed=3)
    d2.apply(0.02)
    assert (r.refit_bvh(cs) == refit_numpy(topo, shape_boxes(cs))).all()   # the kept links still are cs's topology
    built = r.build_bvh(cs, keep_on_device=True)
    tree = r.read_device_bvh()
    r.update_shapes(other)
    assert len(tree) == built and (r.read_device_bvh() == tree).all()
    d.restore(); d2.restore()


def test_a_small_fuzz(r, r2, oracle):
    """40 scenes of tests/scenes.py (random, clustered, degenerate, smooth mesh), seeds from a hash of the sources: each deformed
    once and updated, frame and counters against the oracle on the tree hj_refit_bvh_device makes of the same shapes on a second
    context (the numpy restatement does not order the box of a sphere with a negative radius, which the degenerate scenes hold)"""
    seed = FZ.source_seed()
    rng = np.random.default_rng(seed + 7)
    gens = (scenes.random_scene, scenes.random_cluster_scene, scenes.nasty_scene, scenes.smooth_mesh_scene)
    t0 = time.time()
    for k in range(40):
        s = int(rng.integers(0, 1_000_000))
        cs = gens[k % 4](s)
        what = f"HJ_FUZZ_SEED={seed}: scene {k} ({gens[k % 4].__name__}({s}))"
        topo = cs.bvh.copy()
        blocks = host.make_blocks(96, 64, 2, s)
        r.upload_scene(cs)
        d = Deformation(cs, seed=s)
        d.apply(float(rng.choice([0.005, 0.02, 0.05])), t=float(rng.random()))
        r.update_shapes(cs)
        r.create_framebuffer(96, 64)
        st = r.render_blocks(blocks)
        got = r.read().copy()
        cs.set_bvh(r2.refit_bvh(cs, topology=topo))
        want, ctr, _ = oracle.render_blocks(cs, blocks, 96, 64)
        assert_same(got, want, what)
        assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"] and st["hits"] == ctr["hits"], what
    print(f"update fuzz: seed {seed}, 40 scenes, {time.time() - t0:.1f} s")
