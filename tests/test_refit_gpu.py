"""hj_refit_bvh_device on the GPU: the boxes of a flattened tree recomputed on the device for shapes that have moved, against a
restatement in numpy float32 (bit for bit) and, frame by frame, against the oracle walking the refitted tree (0 differing bits)."""
import numpy as np
import pytest

import refit_scenes
from refit_scenes import Deformation, refit_numpy, sa_cost
from hijiki_amd import abi, device, host
from test_gpu_parity import _check_skip_link_tree, _shape_boxes, assert_same, render

pytestmark = pytest.mark.gpu


@pytest.fixture
def r():
    """A context of its own: no tree and no kept links of an earlier test on it."""
    with device.Renderer(0) as ctx:
        yield ctx


def _same_links(nodes, topo):
    return (nodes[:, 3] == topo[:, 3]).all() and (nodes[:, 7] == topo[:, 7]).all()


@pytest.mark.parametrize("kind", [host.SYNTH_CBOX, host.SYNTH_CBOX_SPHERES])
def test_unmoved_refit_of_a_device_built_tree_is_that_tree(r, kind):
    cs = host.Scene.synthetic(kind, mesh_triangles=1280).compile()
    nodes = r.build_bvh(cs)
    again = r.refit_bvh(cs, topology=nodes)
    assert (again == nodes).all(), f"{int((again != nodes).any(axis=1).sum())} of {len(nodes)} records differ"
    assert (r.refit_bvh(cs, topology=nodes) == nodes).all()
    assert (r.refit_bvh(cs) == nodes).all()                                # ... and over the kept links
    assert (r.read_device_bvh() == nodes).all()


def _cases():
    return ["device-built", "host-compiled", "chain"]


@pytest.mark.parametrize("case", _cases())
def test_refit_equals_the_numpy_restatement(r, case):
    """(a) the device-built tree, (b) the host-compiled one (tuned SAH topology), (c) a chain over 3000 small spheres, each after a
    deformation: the device's records equal the numpy refit in all 8 words, are a valid tree over the moved shapes, keep the links."""
    if case == "chain":
        cs = refit_scenes.sphere_chain_scene(3000)
        topo = refit_scenes.chain_topology(3000)
    else:
        cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile()
        topo = r.build_bvh(cs) if case == "device-built" else cs.bvh.copy()
    if case == "host-compiled":
        unmoved = r.refit_bvh(cs, topology=topo)
        same = bool((unmoved == topo).all())
        print(f"refit of the UNMOVED scene reproduces Scene::compile's boxes: {same}"
              + ("" if same else f" ({int((unmoved != topo).any(axis=1).sum())} of {len(topo)} records differ)"))
        assert same                # (the synthetic scenes: the host's boxes are the same chain of min / max - DESIGN.md 4, "Refit")
    d = Deformation(cs, seed=7)
    for step, amp in enumerate((0.01, 0.03)):
        d.apply(amp, t=0.7 * step)
        boxes = _shape_boxes(cs)
        got = r.refit_bvh(cs, topology=topo if step == 0 else None)
        want = refit_numpy(topo, boxes)
        assert (got == want).all(), f"{case}, step {step}: {int((got != want).any(axis=1).sum())} of {len(want)} records differ"
        _check_skip_link_tree(got, boxes)
        assert _same_links(got, topo)
    d.restore()


@pytest.mark.parametrize("case", ["mesh", "chain"])
def test_both_kernel_forms_give_the_same_records(r, monkeypatch, case):
    """HJ_REFIT_TILED = 1 (subtrees inside a run of records finished in LDS) and 0 (the plain climb): the same records, which are
    the numpy restatement's - on a tree of 300 k records (runs of 1024 records: most subtrees inside one, hundreds straddling) and
    on the chain, where NO inner node's subtree lies inside a run but the last ones."""
    if case == "chain":
        cs = refit_scenes.sphere_chain_scene(3000)
        topo = refit_scenes.chain_topology(3000)
    else:
        cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=150000).compile(with_tree=False)
        topo = r.build_bvh(cs)
    d = Deformation(cs, seed=8)
    d.apply(0.02, t=0.2)
    want = refit_numpy(topo, _shape_boxes(cs))
    for tiled in ("1", "0", "1"):
        monkeypatch.setenv("HJ_REFIT_TILED", tiled)
        got = r.refit_bvh(cs, topology=topo if tiled == "1" else None)
        assert (got == want).all(), f"HJ_REFIT_TILED={tiled}: {int((got != want).any(axis=1).sum())} of {len(want)} records differ"
        assert (r.refit_bvh(cs) == want).all()                            # (the counters were left zero)
    d.restore()


def _animate(r, oracle, cs, topo, W, H, amps, seed):
    """Three steps deform -> refit (tree stays on the device) -> upload(bvh = NULL) -> render, each against the oracle on the
    read-back copy and against the same tree through the host."""
    blocks = host.make_blocks(W, H, 3, 23)
    d = Deformation(cs, seed=seed)
    for step, amp in enumerate(amps):
        d.apply(amp, t=0.9 * step)
        n = r.refit_bvh(cs, topology=topo if step == 0 else None, keep_on_device=True)
        assert n == 2 * cs.num_shapes - 1
        nodes = r.read_device_bvh()
        assert _same_links(nodes, topo)
        r.upload_scene(cs, device_tree=True)
        r.create_framebuffer(W, H)
        st = r.render_blocks(blocks)
        got = r.read().copy()
        with pytest.raises(abi.HijikiError):                              # the upload consumed the tree (not the links)
            r.read_device_bvh()
        cs.set_bvh(nodes)
        want, ctr, _ = oracle.render_blocks(cs, blocks, W, H)
        assert_same(got, want, f"refitted tree, step {step}")
        assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"] and st["hits"] == ctr["hits"]
        through_host = r.refit_bvh(cs)                                    # the same tree through the host: kept links
        assert (through_host == nodes).all()
        cs.set_bvh(through_host)
        host_frame, st2 = render(r, cs, W, H, blocks)
        assert_same(host_frame, got, f"host route against the device route, step {step}")
        assert st2["shadow_rays_proven_free"] == st["shadow_rays_proven_free"]
    d.restore()


@pytest.mark.parametrize("case", ["device-built", "host-compiled"])
def test_animation_frames_small_scene(r, oracle, case):
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile()
    topo = r.build_bvh(cs) if case == "device-built" else cs.bvh.copy()
    _animate(r, oracle, cs, topo, 160, 96, (0.01, 0.02, 0.03), seed=2)


def test_animation_frames_150k_triangle_mesh(r, oracle):
    cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=150000).compile(with_tree=False)
    topo = r.build_bvh(cs)
    _animate(r, oracle, cs, topo, 160, 96, (0.005, 0.01, 0.02), seed=4)


@pytest.mark.parametrize("kind,amp", [(host.SYNTH_CBOX_SPHERES, 0.03), (host.SYNTH_CBOX, 0.005)])
def test_light_grid_of_the_upload_is_the_deformed_scene_s(r, kind, amp):
    """The light-shaft grid is rebuilt by the upload from the arrays it is given: with HJ_RENDER_NO_LIGHT_GRID (every shadow ray
    walked) the deformed scene renders the same frame as with the grid's proofs."""
    cs = host.Scene.synthetic(kind, mesh_triangles=1280).compile()
    topo = cs.bvh.copy()
    d = Deformation(cs, seed=9)
    d.apply(amp, t=0.4)
    W, H = 160, 96
    blocks = host.make_blocks(W, H, 3, 23)
    frames = []
    for flags in (0, abi.RENDER_NO_LIGHT_GRID):
        r.refit_bvh(cs, topology=topo, keep_on_device=True)
        r.upload_scene(cs, device_tree=True)
        r.create_framebuffer(W, H)
        o = device.default_opts()
        o.flags = flags
        st = r.render_blocks(blocks, o)
        frames.append((r.read().copy(), st))
    assert_same(frames[1][0], frames[0][0], "no light grid against the grid, deformed scene")
    print("shadow rays the grid proved free:", frames[0][1]["shadow_rays_proven_free"], "of", frames[0][1]["shadow_rays"])
    d.restore()


def test_kept_links(r):
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile()
    with pytest.raises(abi.HijikiError) as e:                             # a fresh context keeps nothing
        r.refit_bvh(cs)
    assert e.value.status == abi.HJ_ERR_STATE
    topo = cs.bvh.copy()
    first = r.refit_bvh(cs, topology=topo)
    r.upload_scene(cs, device_tree=True)                                  # consumes the tree ...
    built = r.build_bvh(cs)                                               # ... a build of the same scene in between ...
    assert not _same_links(built, topo)
    assert (r.read_device_bvh() == built).all()
    d = Deformation(cs, seed=3)
    d.apply(0.02)
    got = r.refit_bvh(cs)                                                 # ... and the kept links are still the first topology
    assert _same_links(got, topo) and (got == refit_numpy(topo, _shape_boxes(cs))).all()
    d.restore()
    assert (r.refit_bvh(cs) == first).all()
    other = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=320).compile()
    assert other.num_shapes != cs.num_shapes
    with pytest.raises(abi.HijikiError) as e:                             # kept links of another shape count
        r.refit_bvh(other)
    assert e.value.status == abi.HJ_ERR_INVALID
    assert (r.read_device_bvh() == first).all()                           # refused before the tree on the device was touched


def test_refusals_leave_the_tree_and_the_links(r):
    cs = host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=1280).compile()
    topo = cs.bvh.copy()
    good = r.refit_bvh(cs, topology=topo)

    def refused(topology, undo=None):
        with pytest.raises(abi.HijikiError) as e:
            r.refit_bvh(cs, topology=topology)
        if undo:
            undo()
        assert e.value.status == abi.HJ_ERR_INVALID, str(e.value)
        assert (r.read_device_bvh() == good).all()                        # the tree that was there before
        assert (r.refit_bvh(cs) == good).all()                            # the kept links still work
        return str(e.value)

    bad = topo.copy()                                                     # one exit moved (the edit test_gpu_parity.py makes)
    i = int(np.nonzero(bad[:, 3] == 0xFFFFFFFF)[0][5])
    right = int(bad[i + 1, 7])
    assert int(bad[right, 7]) < len(bad) - 1
    bad[right, 7] = int(bad[right, 7]) + 1
    assert "not a pre-order skip-link tree" in refused(bad)
    bad = topo.copy()                                                     # a leaf's shape index duplicated
    leaves = np.nonzero(bad[:, 3] != 0xFFFFFFFF)[0]
    bad[leaves[3], 3] = bad[leaves[10], 3]
    assert "two leaves" in refused(bad)
    assert "records" in refused(topo[:-2])                                # N != 2 * shapes - 1
    tri = cs.triangles
    keep = int(tri[7, 1])
    tri[7, 1] = len(cs.vertices)                                          # a triangle with a vertex index out of range

    def put_back():
        tri[7, 1] = keep
    assert "unknown vertex" in refused(topo, undo=put_back)
    assert (r.refit_bvh(cs, topology=topo) == good).all()


def test_surface_area_cost(r):
    """out_cost against the same sum in numpy float64 over the returned records.  Bound: 1e-9 relative (a double sum of at most
    2^25 positive terms is off by at most 2^25 x 2^-53 = 4e-9 relative in the worst case and far less in practice)."""
    cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=150000).compile(with_tree=False)
    built = r.build_bvh(cs)
    nodes, cost = r.refit_bvh(cs, topology=built, cost=True)
    assert (nodes == built).all()
    want = sa_cost(nodes)
    rel = abs(cost - want) / want
    print(f"cost {cost!r} against numpy {want!r}: relative difference {rel:.3e} (bound 1e-9)")
    assert rel < 1e-9
    nodes2, cost2 = r.refit_bvh(cs, cost=True)                            # unmoved, kept links: the same tree, exactly the same double
    assert (nodes2 == built).all() and cost2 == cost
    n3, cost3 = r.refit_bvh(cs, keep_on_device=True, cost=True)
    assert n3 == len(built) and cost3 == cost
    d = Deformation(cs, seed=6)
    d.apply(0.02)
    moved, cost_moved = r.refit_bvh(cs, cost=True)
    want = sa_cost(moved)
    rel = abs(cost_moved - want) / want
    print(f"deformed: cost {cost_moved!r} against numpy {want!r}: relative difference {rel:.3e}; refitted / unmoved {cost_moved / cost:.4f}")
    assert rel < 1e-9
    d.restore()
