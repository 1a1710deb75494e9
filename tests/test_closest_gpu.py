"""hj_closest_points and hj_distance_field on the GPU against closest_ref - brute force over all shapes - bit for bit on all eight
words: a single sphere under a hand-written one-record tree, and four scenes through the three routes into an upload, five point counts, the radius cases, moved shapes from host and device
arrays, device tensors against host arrays, the statistics, launches cut by HJ_TRACE_CHUNK, the field."""
import ctypes as C
import functools

import numpy as np
import pytest

import closest_ref as R
import scenes
from refit_scenes import refit_numpy, shape_boxes
from hijiki_amd import abi, device, host

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
COUNTS = (1, 63, 64, 65, 4097)
ROUTES = ("host_tree", "device_tree", "optimized")


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


class OneSphere:
    """A scene of ONE sphere under a one-record tree whose root is a leaf, as a bare hj_scene_desc: host.Scene.compile and
    hj_build_bvh_device refuse fewer than two shapes ("root would be a leaf"), hj_scene_upload takes a hand-written tree.  The
    arrays are those of a compiled two-sphere scene with the counts cut to one shape; the attributes are what closest_ref and
    shape_boxes read of a compiled scene."""

    def __init__(self):
        s = host.Scene()
        s.set_camera((0, 0, 5), (0, 0, 0, 1), 40.0)
        m = s.add_diffuse((0.5, 0.5, 0.5))
        s.add_sphere((0.5, -0.25, 1.0), 0.75, m)
        s.add_sphere((9.0, 9.0, 9.0), 0.5, m)
        self._two = s.compile()                                          # (keeps the arrays alive)
        self.spheres = self._two.spheres[:1]
        self.quads, self.triangles, self.vertices = np.zeros((0, 12), F), np.zeros((0, 3), U), np.zeros((0, 8), F)
        lo, hi = shape_boxes(self)
        self._node = (abi.BvhNode * 1)()
        self._node[0].aabb_min[:], self._node[0].aabb_max[:] = lo[0].tolist(), hi[0].tolist()
        self._node[0].shape_index, self._node[0].exit_index = 0, 1       # a leaf over shape 0 that leaves the tree
        self.desc = abi.SceneDesc()
        C.memmove(C.byref(self.desc), C.byref(self._two.desc), C.sizeof(abi.SceneDesc))
        self.desc.bvh, self.desc.num_bvh_nodes = self._node, 1
        self.desc.num_spheres, self.desc.num_materials, self.desc.num_emitters = 1, 1, 0


def _two_triangles():
    s = host.Scene()
    s.set_camera((0, 0, 5), (0, 0, 0, 1), 40.0)
    m = s.add_diffuse((0.5, 0.5, 0.5))
    b = s.add_vertices(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], F), np.tile(F([0, 0, 1]), (4, 1)))
    s.add_triangle(b, b + 1, b + 2, m)
    s.add_triangle(b + 1, b + 3, b + 2, m)
    return s.compile()


def _mesh():
    return scenes.smooth_mesh_scene(11)                                  # 1 sphere, 1 quad, 1244 triangles


def _mesh_far():
    """the mesh translated by +1000 on every axis, its tree refitted in numpy: the slack's worst case"""
    cs = _mesh()
    cs.vertices[:, 0:3] += F(1000)
    cs.quads[:, 0:3] += F(1000)
    cs.spheres[:, 0:3] += F(1000)
    cs.set_bvh(refit_numpy(cs.bvh, shape_boxes(cs)))
    return cs


SCENES = {"sphere": OneSphere, "two_triangles": _two_triangles, "cbox": lambda: host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=200).compile(),
          "mesh": _mesh, "mesh_far": _mesh_far}


def _ulps(p, n, k):
    """p moved k floats along the sign of n per axis (k < 0: against it)"""
    out = p.copy()
    for _ in range(abs(k)):
        out = np.where(n == 0, out, np.nextafter(out, np.where((n > 0) == (k > 0), F(np.inf), F(-np.inf)))).astype(F)
    return out


def point_set(cs, sh, seed=3):
    """4097 points (p, r): on the shapes - vertices, edge midpoints, centroids of triangles and quads (shared edges and corners: ties) -,
    the same pushed 1 and 2 floats along +-normal, sphere centres and points inside spheres, points 1e6 away, a random cloud in 1.5
    times the scene's box; r = +inf, but for stated slices 0, NaN, negative, and - filled in by case() - the reference's distance and
    one float below it."""
    rng = np.random.default_rng(seed)
    lo, hi = shape_boxes(cs)
    lo, hi = lo.min(0), hi.max(0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5 + 1e-3
    on, nrm = [], []
    for t in (sh["triangles"], sh["quads"]):
        if len(t):
            pick = t[rng.permutation(len(t))[:200]]
            a, e1, e2 = pick[:, 0], pick[:, 1], pick[:, 2]
            n = np.cross(e1, e2)
            for wu, wv in ((0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (1 / 3, 1 / 3), (1, 1)):
                on.append((a + e1 * F(wu) + e2 * F(wv)).astype(F))
                nrm.append(n)
    parts = []
    if on:
        on, nrm = np.concatenate(on), np.concatenate(nrm)
        keep = rng.permutation(len(on))[:600]
        on, nrm = on[keep], nrm[keep]
        parts += [on] + [_ulps(on, nrm, k) for k in (1, 2, -1, -2)]
    s = sh["spheres"]
    if len(s):
        d = rng.normal(size=(len(s) * 8, 3))
        inside = np.repeat(s[:, 0:3], 8, 0) + d / np.linalg.norm(d, axis=1, keepdims=True) * np.repeat(s[:, 3:4], 8, 0) * rng.uniform(0, 1, (len(d), 1))
        onsurf = np.repeat(s[:, 0:3], 8, 0) + d / np.linalg.norm(d, axis=1, keepdims=True) * np.repeat(s[:, 3:4], 8, 0)
        parts += [s[:, 0:3], inside.astype(F), onsurf.astype(F)]
    far = (rng.normal(size=(16, 3)) * 1e6 + mid).astype(F)
    parts.append(far)
    have = sum(len(x) for x in parts)
    cloud = (mid + rng.uniform(-1, 1, (4097 - have, 3)) * half).astype(F)
    p = np.concatenate(parts + [cloud]).astype(F)
    p = p[rng.permutation(len(p))]                                       # (every prefix holds every kind)
    assert len(p) == 4097
    pts = np.concatenate([p, np.full((4097, 1), np.inf, F)], 1).astype(F)
    pts[5::64, 3] = 0.0
    pts[6::64, 3] = np.nan
    pts[7::64, 3] = -1.0
    return pts


EXACT, BELOW = slice(8, None, 64), slice(9, None, 64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(compiled scene, its shape records, 4097 points, the reference's records): computed once, never written to"""
    cs = SCENES[name]()
    sh = R.shapes_of(cs)
    pts = point_set(cs, sh)
    first = R.closest(sh, pts)
    pts[EXACT, 3] = first[EXACT, 1]
    pts[BELOW, 3] = np.nextafter(first[BELOW, 1], F(-np.inf))
    want = R.closest(sh, pts)
    pts.setflags(write=False)
    want.setflags(write=False)
    return cs, sh, pts, want


def upload(r, cs, route):
    if route == "host_tree":
        r.upload_scene(cs)
        return
    r.build_bvh(cs, keep_on_device=True)
    if route == "optimized":
        r.optimize_bvh_device(cs, passes=4)
    r.upload_scene(cs, device_tree=True)


def assert_records(got, want, what):
    bad = (bits(got) != bits(want)).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(want)} records differ, first at point {int(np.argmax(bad))}: {got[np.argmax(bad)]} != {want[np.argmax(bad)]}"


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as r:
        yield r


# (the single sphere goes up under its hand-written tree alone: hj_build_bvh_device refuses fewer than two shapes - shown below)
@pytest.mark.parametrize("name,route", [(n, r) for n in SCENES for r in ROUTES if n != "sphere" or r == "host_tree"])
def test_records_equal_brute_force_on_bits(rq, name, route):
    cs, sh, pts, want = case(name)
    upload(rq, cs, route)
    ids = R.ids(want)
    assert (ids >= 0).sum() > 3000 and (ids < 0).sum() >= 3 * 64 and (set(np.unique(ids)) == {-1, 0} if name == "sphere" else len(np.unique(ids)) > 2)
    assert (want[EXACT, 0].view(np.int32) >= 0).mean() > 0.3            # (r = the distance: r * r may round below d2 - the reference decides)
    for n in COUNTS:
        assert_records(rq.closest_points(pts[:n]), want[:n], f"{name} / {route} / {n} points")


def test_the_device_build_refuses_a_single_shape(rq):
    """why the single sphere has one route: the build needs two shapes (the host compiler says the same, and compile() raises)"""
    one = OneSphere()
    with pytest.raises(abi.HijikiError, match="at least 2 shapes"):
        rq.build_bvh(one, keep_on_device=True)
    s = host.Scene()
    s.add_sphere((0, 0, 0), 1.0, s.add_diffuse((0.5, 0.5, 0.5)))
    with pytest.raises(abi.HijikiError, match="at least 2 shapes"):
        s.compile()


@functools.lru_cache(maxsize=None)
def vertex_case():
    """EVERY vertex, edge midpoint and face centroid of the mesh scene's triangles and quads, and every vertex pushed one float along
    +-normal (the 4097-point sets hold a sample of all of these pushed 1 and 2 floats), unbounded radius; the reference's records and,
    per point, how many shapes share the minimal key."""
    cs, sh, _, _ = case("mesh")
    t = np.concatenate([sh["quads"], sh["triangles"]])
    a, e1, e2 = t[:, 0], t[:, 1], t[:, 2]
    n = np.cross(e1, e2)
    on = np.concatenate([(a + e1 * F(wu) + e2 * F(wv)).astype(F) for wu, wv in ((0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (1 / 3, 1 / 3))])
    p = np.concatenate([on, _ulps(a, n, 1), _ulps(a, n, -1)])
    pts = np.concatenate([p, np.full((len(p), 1), np.inf, F)], 1).astype(F)
    want, ties = R.closest(sh, pts, ties=True)
    pts.setflags(write=False)
    want.setflags(write=False)
    return pts, want, ties


def test_every_vertex_edge_midpoint_and_centroid_of_the_mesh(rq):
    cs, sh, _, _ = case("mesh")
    pts, want, ties = vertex_case()
    assert len(pts) == 9 * (len(sh["quads"]) + len(sh["triangles"]))
    # real ties: points where two or more shapes have the minimal d2 bits - shared vertices and edges - and the lower index wins
    assert (ties >= 2).sum() > 1000 and (ties >= 4).sum() > 100, ((ties >= 2).sum(), (ties >= 4).sum())
    rq.upload_scene(cs)
    assert_records(rq.closest_points(np.array(pts)), want, "every vertex, edge midpoint and centroid")


def test_both_forms_of_the_walk_give_the_same_bits(rq, monkeypatch):
    """HJ_CLOSEST_ORDERED=0, the stackless walk alone, against the default (nearer child first): the records bit for bit on every
    scene; the statistics differ, and each form's are its own function of the points and the tree."""
    ordered = {}
    for name in SCENES:                                                   # (an upload reads the switches: the default form first)
        cs, sh, pts, want = case(name)
        rq.upload_scene(cs)
        ordered[name] = rq.closest_points(pts, stats=True)[1]
    monkeypatch.setenv("HJ_CLOSEST_ORDERED", "0")
    with device.Renderer(0) as r:
        for name in SCENES:
            cs, sh, pts, want = case(name)
            r.upload_scene(cs)
            got, st = r.closest_points(pts, stats=True)
            assert_records(got, want, f"{name} / stackless")
            print(f"{name}: stackless {st}, ordered {ordered[name]}")
            if name == "mesh":
                assert ordered[name]["shapes_tested"] < st["shapes_tested"]


def test_a_tree_deeper_than_the_stack_falls_back(rq):
    """A chain: 40 spheres along a line under a tree that is one long right spine given in far-to-near order for points at the near
    end, so the ordered walk has more than its 32 stack entries pending and takes the stackless walk for those points."""
    n = 40
    s = host.Scene()
    s.set_camera((0, 0, 5), (0, 0, 0, 1), 40.0)
    m = s.add_diffuse((0.5, 0.5, 0.5))
    for k in range(n):
        s.add_sphere((float(k), 0.0, 0.0), 0.25, m)
    cs = s.compile()
    lo, hi = shape_boxes(cs)
    # pre-order spine: inner, leaf k, inner, leaf k + 1, ..., the last two leaves; every inner node's left child is a leaf
    nodes = np.zeros((2 * n - 1, 8), U)
    nodes[0:2 * n - 2:2, 3] = abi.BVH_INNER
    nodes[1:2 * n - 2:2, 3] = np.arange(n - 1)
    nodes[2 * n - 2, 3] = n - 1
    nodes[1:2 * n - 2:2, 7] = np.arange(2, 2 * n, 2)
    nodes[0:2 * n - 2:2, 7] = 2 * n - 1
    nodes[2 * n - 2, 7] = 2 * n - 1
    cs.set_bvh(refit_numpy(nodes, (lo, hi)))
    rq.upload_scene(cs)
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform([-3, -1, -1], [n + 2, 1, 1], (513, 3)), np.full((513, 1), np.inf)], 1).astype(F)
    pts[:64, 0] = n + 1 + pts[:64, 0] * 0.01                           # beyond the far end: every left leaf is the farther child
    assert_records(rq.closest_points(pts), R.closest(R.shapes_of(cs), pts), "spine of 40")


def test_points_as_n_by_3_with_radii(rq):
    cs, sh, pts, want = case("two_triangles")
    rq.upload_scene(cs)
    assert_records(rq.closest_points(np.ascontiguousarray(pts[:65, 0:3]), radius=pts[:65, 3]), want[:65], "per-point radius")
    inf = np.concatenate([pts[:65, 0:3], np.full((65, 1), np.inf, F)], 1)
    assert_records(rq.closest_points(np.ascontiguousarray(pts[:65, 0:3])), R.closest(sh, inf), "scalar radius")


def test_device_tensors_in_place_and_statistics(rq):
    import torch
    cs, sh, pts, want = case("mesh")
    rq.upload_scene(cs)
    host_out, st1 = rq.closest_points(pts, stats=True)
    t = torch.from_numpy(np.array(pts)).to(f"cuda:{rq.device}")
    dev_out, st2 = rq.closest_points(t, stats=True, device=True)
    assert_records(host_out, want, "host arrays")
    assert_records(dev_out.cpu().numpy(), want, "device tensors")
    assert st1 == st2 and st1["nodes_visited"] > 0
    # the walk skips something: with unbounded radius fewer shape tests than brute force
    unbounded = np.array(pts)
    unbounded[:, 3] = np.inf
    _, st = rq.closest_points(unbounded, stats=True)
    n, N = len(pts), R.count(sh)
    print(f"mesh, {n} points, {N} shapes, unbounded: {st['shapes_tested']} shapes tested ({st['shapes_tested'] / (n * N):.4f} of n * N), {st['nodes_visited']} nodes visited")
    assert 0 < st["shapes_tested"] < n * N
    # stats as a device pointer is refused before anything runs
    word = torch.zeros(2, dtype=torch.int64, device=t.device)
    out = torch.full((len(pts), 8), 7.0, device=t.device)
    rc = device.lib().hj_closest_points(rq._h, t.data_ptr(), len(pts), abi.CLOSEST_DEVICE_ARRAYS, out.data_ptr(), C.cast(word.data_ptr(), C.POINTER(C.c_uint64)))
    assert rc == abi.HJ_ERR_INVALID and (out == 7.0).all().item()


def test_chunks_give_the_same_bits_and_the_same_statistics(rq, monkeypatch):
    """HJ_TRACE_CHUNK=1000 cuts the 4097 points into five launches, the last of 97: the records on bits, and the statistics - counted
    per point in its own lane, summed per workgroup and read back per launch - equal to the one launch's, from host arrays and from
    device tensors."""
    import torch
    cs, sh, pts, want = case("mesh")
    assert len(pts) >= 2001 and len(pts) % 1000 and len(pts) % 256
    rq.upload_scene(cs)
    whole, st_whole = rq.closest_points(pts, stats=True)
    assert st_whole["nodes_visited"] > 0 and st_whole["shapes_tested"] > 0
    monkeypatch.setenv("HJ_TRACE_CHUNK", "1000")
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        got, st = r.closest_points(pts, stats=True)
        assert_records(got, whole, "host arrays in chunks of 1000")
        assert st == st_whole
        t = torch.from_numpy(np.array(pts)).to(f"cuda:{r.device}")
        got, st = r.closest_points(t, stats=True, device=True)
        assert_records(got.cpu().numpy(), whole, "device tensors in chunks of 1000")
        assert st == st_whole


@pytest.mark.parametrize("from_device", [False, True])
def test_moved_shapes_answer_for_the_moved_scene(rq, from_device):
    cs = _mesh()
    rq.upload_scene(cs)
    pts = np.array(case("mesh")[2][:513])
    cs.vertices[:, 0:3] = (cs.vertices[:, 0:3] * F(1.03) + F([0.05, -0.02, 0.01])).astype(F)
    cs.spheres[:, 0:3] += F(0.1)
    cs.quads[:, 0:3] -= F(0.05)
    if from_device:
        import torch
        dev = f"cuda:{rq.device}"
        arrays = dict(spheres=torch.from_numpy(np.array(cs.spheres)).to(dev), quads=torch.from_numpy(np.array(cs.quads)).to(dev),
                      vertices=torch.from_numpy(np.array(cs.vertices)).to(dev))
        rq.update_shapes(cs, device_arrays=arrays)
    else:
        rq.update_shapes(cs)
    assert_records(rq.closest_points(pts), R.closest(R.shapes_of(cs), pts), "after update_shapes")


@pytest.mark.parametrize("signed", [True, False])
def test_distance_field_on_a_grid_with_misses(rq, signed):
    cs, sh, _, _ = case("cbox")
    rq.upload_scene(cs)
    lo, hi = shape_boxes(cs)
    lo, hi = lo.min(0), hi.max(0)
    origin, spacing, count = lo - (hi - lo) * F(0.2), (hi - lo) * F(1.4) / F([4, 3, 2]), (5, 4, 3)
    md = float((hi - lo).min()) * 0.15
    want = R.distance_field(sh, origin, spacing, count, md, signed)
    assert want.shape == (3, 4, 5) and 0 < (want == F(md)).sum() < want.size
    got = rq.distance_field(origin, spacing, count, max_distance=md, signed=signed)
    assert got.shape == want.shape and (bits(got) == bits(want)).all()
    dev = rq.distance_field(origin, spacing, count, max_distance=md, signed=signed, device=True)
    assert (bits(dev.cpu().numpy()) == bits(want)).all()
