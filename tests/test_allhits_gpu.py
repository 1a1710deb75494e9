"""hj_trace_rays_all and hj_points_inside on the GPU against allhits_ref - the contract restated in numpy - bit for bit on every word:
the cbox with its spheres, the smooth mesh and the hand-built scenes under their hand-written trees, through every route into an
upload, at K = 0, 1, 3, 8, in chunks, from device tensors, after moved shapes; containment on a cube, a flipped cube and a sphere.
The reference is fed with the tree actually uploaded: the compiled scene's node array, hj_bvh_device_read's after a device build -
each checked against the device's own second copy of the tree - and that copy itself after hj_scene_update_shapes."""
import functools

import numpy as np
import pytest

import allhits_cases as cases
import allhits_ref as A
from hijiki_amd import device

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
KS = (0, 1, 3, 8)
ROUTES = ("host_tree", "device_tree", "optimized")


def differing(got, want):
    """how many words differ, counts and crossings and hit records together"""
    return sum(int((np.ascontiguousarray(g).view(U) != np.ascontiguousarray(w).view(U)).sum()) for g, w in zip(got, want))


def assert_same(got, want, what):
    assert all(np.asarray(g).shape == np.asarray(w).shape for g, w in zip(got, want)), what
    bad = differing(got, want)
    if bad:
        rows = np.nonzero((got[0] != want[0]) | (got[1] != want[1]) | (got[2].view(U) != want[2].view(U)).any((1, 2)))[0]
        i = int(rows[0])
        raise AssertionError(f"{what}: {bad} words differ on {len(rows)} rays, first ray {i}: counts {got[0][i]} / {want[0][i]}, crossings "
                             f"{got[1][i]} / {want[1][i]}, hits {got[2][i].tolist()} / {want[2][i].tolist()}")


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as r:
        yield r


def upload(r, cs, route):
    """-> the node array the walk reads, in the uploaded layout"""
    if route == "host_tree":
        r.upload_scene(cs)
        fed = np.array(cs.bvh, U)
    else:
        r.build_bvh(cs, keep_on_device=True)
        if route == "optimized":
            r.optimize_bvh_device(cs, passes=4)
        fed = r.read_device_bvh()
        r.upload_scene(cs, device_tree=True)
    assert A.same_walk(fed, A.nodes_of_device(r.scene_tree())), route        # (the second copy is the uploaded array verbatim)
    return fed


@functools.lru_cache(maxsize=None)
def reference(name, route, nodes_key):
    """the reference at K = 8 under the nodes of a route (the host tree's is cases.want)"""
    cs, sh, rays = cases.case(name)
    return A.all_hits(sh, np.frombuffer(nodes_key, U).reshape(-1, 8), rays, 8)


def head(want, K):
    return want[0], want[1], np.ascontiguousarray(want[2][:, :K])


@pytest.mark.parametrize("name", ["cbox", "mesh"])
def test_every_word_equals_the_reference_at_every_k(rq, name):
    cs, sh, rays = cases.case(name)
    want = cases.want(name)
    assert len(rays) % 64 != 0 and len(rays) % 256 != 0 and (want[0] > 8).any() and (want[0] == 0).any()
    upload(rq, cs, "host_tree")
    for K in KS:
        # (the first min(count, K) records for K < count are the head of the K = 8 list: the reference's slice IS that head)
        assert_same(rq.trace_rays_all(np.array(rays), K), head(want, K), f"{name} / K = {K}")
    for n in (1, 63, 64, 65, 257):
        assert_same(rq.trace_rays_all(np.array(rays[:n]), 8), tuple(x[:n] for x in want), f"{name} / {n} rays")
    c0, x0, h0 = rq.trace_rays_all(np.array(rays), 0)
    c8, x8, _ = rq.trace_rays_all(np.array(rays), 8)
    assert h0.shape == (len(rays), 0, 4) and (c0 == c8).all() and (x0 == x8).all()


@pytest.mark.parametrize("name", ["stack", "coincident"])
def test_hand_built_scenes_under_hand_written_trees(rq, name):
    cs, sh, rays = cases.case(name)
    want = cases.want(name)
    upload(rq, cs, "host_tree")
    for K in KS:
        got = rq.trace_rays_all(np.array(rays), K)
        assert_same(got, head(want, K), f"{name} / K = {K}")
    got = rq.trace_rays_all(np.array(rays), 8)
    for i, (_, ray, n, cross, ids) in enumerate(h for h in cases.HAND if h[0] == name):
        assert (int(got[0][i]), int(got[1][i])) == (n, cross), (name, ray)
        assert got[2][i, :, 0].view(np.int32).tolist() == list(ids[:8]) + [-1] * (8 - min(n, 8)), (name, ray)


@pytest.mark.parametrize("route", ROUTES[1:])
@pytest.mark.parametrize("name", ["cbox", "mesh"])
def test_device_built_trees(rq, name, route):
    cs, sh, rays = cases.case(name)
    fed = upload(rq, cs, route)
    want = reference(name, route, fed.tobytes())
    for K in (0, 3, 8):
        assert_same(rq.trace_rays_all(np.array(rays), K), head(want, K), f"{name} / {route} / K = {K}")


def test_moved_shapes_answer_for_the_moved_scene(rq):
    cs = cases.SCENES["mesh"]()
    rays = np.array(cases.case("mesh")[2][:1025])
    rq.upload_scene(cs)
    cs.vertices[:, 0:3] = (cs.vertices[:, 0:3] * F(1.03) + F([0.05, -0.02, 0.01])).astype(F)
    cs.spheres[:, 0:3] += F(0.1)
    cs.quads[:, 0:3] -= F(0.05)
    rq.update_shapes(cs)
    nodes = A.nodes_of_device(rq.scene_tree())                              # the refitted boxes, as the walk reads them
    assert not A.same_walk(nodes, cs.bvh)
    want = A.all_hits(A.shapes_of(cs), nodes, rays, 8)
    assert (want[0] > 0).sum() > 300
    assert_same(rq.trace_rays_all(rays, 8), want, "after update_shapes")


def test_chunks_and_device_tensors_give_the_same_bits(rq, monkeypatch):
    import torch
    cs, sh, rays = cases.case("mesh")
    want = cases.want("mesh")
    rq.upload_scene(cs)
    t = torch.from_numpy(np.array(rays)).to(f"cuda:{rq.device}")
    for K in (0, 8):
        c, x, h = rq.trace_rays_all(t, K)
        assert c.dtype == torch.int32 and h.shape == (len(rays), K, 4)
        assert_same((c.cpu().numpy().view(U), x.cpu().numpy(), h.cpu().numpy()), head(want, K), f"device tensors / K = {K}")
    monkeypatch.setenv("HJ_TRACE_CHUNK", "1000")
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        assert_same(r.trace_rays_all(np.array(rays), 8), want, "chunks of 1000")
        c, x, h = r.trace_rays_all(t, 3)
        assert_same((c.cpu().numpy().view(U), x.cpu().numpy(), h.cpu().numpy()), head(want, 3), "device tensors in chunks of 1000")
        pts = cases.cube_points()[0]
        r.upload_scene(cases.cube_scene())
        chunked = r.points_inside(np.array(pts))
    rq.upload_scene(cases.cube_scene())
    whole = rq.points_inside(np.array(pts))
    assert all((a == b).all() for a, b in zip(chunked, whole))


@pytest.mark.parametrize("flipped", [False, True])
def test_points_inside_a_cube_a_flipped_cube_and_a_sphere(rq, flipped):
    import torch
    pts, inside, outside = cases.cube_points()
    cs = cases.cube_scene(flipped)
    sh = A.shapes_of(cs)
    fed = upload(rq, cs, "host_tree")
    in_cube = inside & (np.abs(pts[:, 0:3]).max(1) <= 0.95)
    assert in_cube.sum() > 100 and outside.sum() > 100 and (~inside & ~outside).sum() > 100     # (the last: within 1e-3 of a face, among others)
    for parity in (False, True):
        want = A.points_inside(sh, fed, pts, parity)
        got = rq.points_inside(np.array(pts), parity)
        assert got[0].dtype == U and (got[0] == want[0]).all() and (got[1] == want[1]).all(), (flipped, parity, int((got[1] != want[1]).sum()))
        dev = rq.points_inside(torch.from_numpy(np.array(pts)).to(f"cuda:{rq.device}"), parity)
        assert (dev[0].cpu().numpy().view(U) == want[0]).all() and (dev[1].cpu().numpy().view(U) == want[1]).all()
        assert (got[0][outside] == 0).all()
        if parity:
            assert (got[0][inside] == 1).all()
        elif flipped:
            assert (got[0][in_cube] == 0).all() and (got[0][inside & ~in_cube] == 1).all()     # (the sphere keeps its orientation)
        else:
            assert (got[0][inside] == 1).all()
    # the three rays of a point through hj_trace_rays_all give the kernel's votes
    c, x, _ = rq.trace_rays_all(A.point_rays(pts), 0)
    assert all((a == b).all() for a, b in zip(A.vote(c, x), rq.points_inside(np.array(pts))))
