"""The tree level on the GPU: the node array hj_scene_upload derives, read back with Renderer.scene_tree(), against
tests/relayout_check.py on every route into an upload - the host's re-layout, the device's, the tree a device build left resident -
and under the switches that change the derivation; the two routes against each other in canonical form; one ray per shape against
the oracle bit for bit; the links across hj_scene_update_shapes."""
import numpy as np
import pytest

import relayout_check as RC
import relayout_scenes as RS
import update_scenes as U
from refit_scenes import Deformation, refit_numpy, shape_boxes
from hijiki_amd import device
from oracle import hj_oracle as O
from test_ray_query_gpu import assert_hits, assert_surface

pytestmark = pytest.mark.gpu

ROUTES = ("0", "1")                                   # HJ_UPLOAD_DEVICE
SWITCHES = ("HJ_PAIR_LEAVES=0", "HJ_NODE_ORDER=0", "HJ_NODE_ORDER=1", "HJ_COLLAPSE_PCT=0", "HJ_COLLAPSE_PCT=1000",
            "HJ_LEAF_GUARDS=0", "HJ_LEAF_GUARDS=1", "HJ_LEAF_GUARDS=2", "HJ_LEAF_GUARDS=3")
CASES = [(name, "") for name in RS.BUILDERS] + [(name, sw) for name in RS.SWITCHED for sw in SWITCHES]
COUNTED = ("guards", "pairs", "dropped", "padding")


@pytest.fixture(scope="module")
def r():
    with device.Renderer(0) as ctx:
        yield ctx


_resident_nodes = []
_uploads = {}


def resident_nodes(r):
    """the tree a device build leaves for the shapes of the resident scene, built once"""
    if not _resident_nodes:
        r.build_bvh(RS.scene("resident"), keep_on_device=True)
        nodes = r.read_device_bvh().copy()
        nodes.setflags(write=False)
        _resident_nodes.append(nodes)
    return _resident_nodes[0]


def upload(r, monkeypatch, name, route, switch):
    """`name` goes up through `route` under `switch`; returns the compiled scene and the uploaded skip-link array.  The resident
    scene's device route is the tree left on the device (bvh == NULL), its host route the same nodes handed over through the host."""
    monkeypatch.setenv("HJ_UPLOAD_DEVICE", route)
    if switch:
        monkeypatch.setenv(*switch.split("="))
    cs = RS.scene(name)
    if name == "resident":
        nodes = resident_nodes(r)
        cs.set_bvh(nodes)                                                    # (the oracle walks the same tree)
        if route == "1":
            r.build_bvh(cs, keep_on_device=True)
            assert (r.read_device_bvh() == nodes).all(), "the device build is not repeatable"
            r.upload_scene(cs, device_tree=True)
            return cs, nodes
    r.upload_scene(cs)
    return cs, cs.bvh.copy()


def uploaded(r, monkeypatch, name, route, switch):
    """(scene_tree(), uploaded nodes, compiled scene) of an upload, made once per case of the matrix and never written to"""
    key = (name, route, switch)
    if key not in _uploads:
        cs, nodes = upload(r, monkeypatch, name, route, switch)
        tree = r.scene_tree()
        for a in (tree["records"], tree["map"], nodes):
            a.setflags(write=False)
        _uploads[key] = (tree, nodes, cs)
    return _uploads[key]


_counts = {}


def checked(r, monkeypatch, name, route, switch):
    key = (name, route, switch)
    if key not in _counts:
        tree, nodes, cs = uploaded(r, monkeypatch, name, route, switch)
        _counts[key] = RC.check_tree(tree, nodes, len(cs.spheres), len(cs.quads), switch != "HJ_PAIR_LEAVES=0", cs=cs)
    return _counts[key]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name,switch", CASES)
def test_tree_is_the_uploaded_tree(r, monkeypatch, name, switch, route):
    counts = checked(r, monkeypatch, name, route, switch)
    print(f"{name}, HJ_UPLOAD_DEVICE={route} {switch}: {counts}")


@pytest.mark.parametrize("name,switch", CASES)
def test_routes_agree(r, monkeypatch, name, switch):
    """Which route a scene takes depends on its size alone: both must derive the same walk.  (What this found: the device route made
    no leaf guards - the box's walk had 1299 records through the host and 1179 through the device, the mesh's 20825 and 18593; 24 of
    the 31 cases differed.  DESIGN.md 5, "Tree level".)"""
    host_tree, host_nodes, _ = uploaded(r, monkeypatch, name, "0", switch)
    dev_tree, dev_nodes, _ = uploaded(r, monkeypatch, name, "1", switch)
    assert (host_nodes == dev_nodes).all()
    a, b = RC.canonical(host_tree, host_nodes), RC.canonical(dev_tree, dev_nodes)
    assert a.shape == b.shape, f"{name} {switch}: the host route's walk has {len(a)} records, the device route's {len(b)}"
    assert (a == b).all(), f"{name} {switch}: the walks differ first at position {int(np.argmax((a != b).any(axis=1)))}"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(RS.BUILDERS))
def test_every_shape_is_found(r, monkeypatch, name, route):
    """One ray per shape (its premise: tests/test_relayout_host.py), and the same rays along the plain normals - on axis-aligned
    shapes those are outside general position and walk the second copy: ids and the bits of t, u, v and of the surface record on
    every ray, the boolean for any-hit."""
    cs, _ = upload(r, monkeypatch, name, route, "")
    rays = np.concatenate([RS.shape_rays(cs), RS.shape_rays(cs, tilt=0.0)])
    want = O.intersect(cs, rays, full=True)
    got = r.trace_rays(rays, surface=True)
    own = int((want[0][:cs.num_shapes] == np.arange(cs.num_shapes)).sum())
    print(f"{name}, HJ_UPLOAD_DEVICE={route}: {len(rays)} rays, {own} of {cs.num_shapes} shapes found by their own ray, {int((want[0] < 0).sum())} misses")
    assert_hits(got, want, name)
    assert_surface(cs, got, want, name)
    ai, *_ = r.trace_rays(rays, any_hit=True)
    assert ((ai >= 0) == (want[0] >= 0)).all(), f"{name}: any-hit booleans"


@pytest.mark.parametrize("route", ROUTES)
def test_an_update_keeps_the_links(r, monkeypatch, route):
    """hj_scene_update_shapes moves boxes, never records: words 3 and 7 of every record stay, and the tree passes against the
    refitted boxes (the hot set is the one chosen on the boxes of the upload)."""
    cs, nodes = upload(r, monkeypatch, "cbox", route, "")
    before = r.scene_tree()
    RC.check_tree(before, nodes, len(cs.spheres), len(cs.quads), True, cs=cs)
    d = Deformation(cs, seed=7)
    try:
        d.apply(0.03, t=0.7)
        r.update_shapes(cs)
        after = r.scene_tree()
        want = refit_numpy(nodes, shape_boxes(cs))
        assert (U.links_of(after["records"]) == U.links_of(before["records"])).all(), "a link word changed"
        assert (after["map"] == before["map"]).all() and all(after[k] == before[k] for k in ("num_nodes", "root", "root2", "num_hot"))
        assert (U.boxes_of(after["records"]) != U.boxes_of(before["records"])).any()
        counts = RC.check_tree(after, want, len(cs.spheres), len(cs.quads), True, cs=cs, placed_on=before["records"])
        print(f"HJ_UPLOAD_DEVICE={route}: after the update {counts}")
    finally:
        d.restore()


def test_the_matrix_exercises_every_feature(r, monkeypatch):
    """guards, pairs, dropped inner nodes, padding records and more reachable records than the hot set holds: each somewhere"""
    seen = {k: 0 for k in COUNTED + ("cold",)}
    for name, switch in CASES:
        for route in ROUTES:
            with monkeypatch.context() as m:
                c = checked(r, m, name, route, switch)
            for k in COUNTED:
                seen[k] += c[k] > 0
            seen["cold"] += c["reachable"] > RC.HOT_NODES
    print(f"cases of {2 * len(CASES)} with a non-zero count: {seen}")
    assert all(v > 0 for v in seen.values()), seen
