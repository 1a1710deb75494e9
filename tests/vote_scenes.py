"""Shared by tests/test_vote_host.py and tests/test_vote_gpu.py: the scenes, rays, trees and gains of the vote's tests.  numpy, the
host library and tests/vote_ref.py only: no GPU, and every choice made here is made from the float64 reference alone."""
import functools
import os

import numpy as np

import lbvh_edges as E
import refit_scenes
import vote_ref as V
from hijiki_amd import abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_RAYS = 4096


# ---------------------------------------------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def cluster(emitters=True, shift=2.0):
    """257 spheres of radius 0.05 ... 0.12 in a 1.8-cube (they overlap: origins lie inside some), with the host's tree.  shift = 2:
    the cube lies in the positive octant, every box bound is positive (see `case`); shift = 0: in front of the Cornell camera.
    emitters=False: the same spheres, none of them a light."""
    s = host.Scene()
    s.set_camera_cbox()
    m, e = s.add_diffuse((0.6, 0.6, 0.6)), s.add_emissive((9, 9, 9))
    rng = np.random.default_rng(23)
    for k in range(257):
        c = rng.uniform(-0.9, 0.9, 3) + (0.13 + shift, 1.07 + shift, 0.21 + shift)
        s.add_sphere(tuple(c), 0.05 + 0.07 * rng.random(), e if (emitters and k % 64 == 0) else m)
    return s.compile()


@functools.lru_cache(maxsize=None)
def cbox():
    """The 1280-triangle Cornell box (host.SYNTH_CBOX_MESH: 1292 triangles with its walls) moved into the positive octant, so that
    every box bound is positive on every axis (see `case`), with the host's tree over the moved mesh."""
    src = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=1280).compile()
    assert len(src.triangles) == 1292 and len(src.spheres) == 0 and len(src.quads) == 0
    s = host.Scene()
    s.set_camera_cbox()
    white, light = s.add_diffuse((0.7, 0.7, 0.7)), s.add_emissive((9, 9, 9))
    v = src.vertices
    base = s.add_vertices(v[:, 0:3] + np.float32([2.1234, 1.0567, 2.0321]), v[:, 4:7], np.stack([v[:, 3], v[:, 7]], axis=1))
    emissive = (src.materials >> abi.MATERIAL_TAG_SHIFT) == abi.MAT_EMISSIVE
    for k, (a, b, c) in enumerate(src.triangles.tolist()):
        s.add_triangle(base + a, base + b, base + c, light if emissive[k] else white)
    cs = s.compile()
    assert len(cs.bvh) == 2583
    return cs


def leaf_positions(nodes, shapes):
    """per shape id (-1: none) the array position of its leaf, V.MISS for none"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    leaf = np.nonzero(nodes[:, 3] != V.INNER)[0]
    where = np.full(len(leaf), V.MISS, np.int64)
    where[nodes[leaf, 3]] = leaf
    shapes = np.asarray(shapes, np.int64)
    return np.where(shapes >= 0, where[np.maximum(shapes, 0)], V.MISS)


# ---------------------------------------------------------------------------------------------------------------- rays
def _candidates(cs, n, seed):
    """n rays from origins inside the scene's box, in blocks of 16: 11 of any direction, 2 shadow-style (tMin 2e-4, tMax 0.3 ... 1.5),
    1 with one exact-zero direction component, 1 along an axis (two zeros), 1 shadow-style with one zero.  Directions are unit vectors
    rounded to float32."""
    rng = np.random.default_rng(seed)
    f = cs.bvh_f32
    lo, hi = f[0, 0:3].astype(np.float64), f[0, 4:7].astype(np.float64)
    rays = np.zeros((n, 8), np.float32)
    o = lo + (hi - lo) * rng.uniform(0.03, 0.97, (n, 3))
    d = rng.normal(size=(n, 3))
    kind = np.arange(n) % 16
    axis, other = rng.integers(0, 3, n), rng.integers(1, 3, n)
    one = (kind == 13) | (kind == 15)
    d[one, axis[one]] = 0.0
    two = kind == 14
    d[two, axis[two]] = 0.0
    d[two, (axis[two] + other[two]) % 3] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 0:3], rays[:, 3:6] = o, d
    rays[:, 6], rays[:, 7] = 1e-4, np.inf
    window = (kind == 11) | (kind == 12) | (kind == 15)
    rays[window, 6], rays[window, 7] = 2e-4, rng.uniform(0.3, 1.5, int(window.sum()))
    assert ((rays[:, 3:6] == 0).sum(axis=1)[two] == 2).all() and ((rays[:, 3:6] == 0).sum(axis=1)[one] == 1).all()
    return rays


def _clear(ref):
    """the rays a choice keeps: ten times further from every tie than vote_ref.ambiguous asks, and no sphere passed within |r^2 - d^2|
    < 1e-5 (float32 forms that difference from terms near 1 - an error of some 1e-7)"""
    t, t2 = ref["t"], ref["t2"]
    with np.errstate(invalid="ignore"):
        second = np.isfinite(t) & (np.abs(t2 - t) <= 1e-3 * np.maximum(1.0, np.abs(t)))
    return ~(second | (ref["window"] <= 1e-3) | (ref["edge"] <= 1e-3) | (ref["graze"] <= 1e-5))


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, NUM_RAYS rays, closest_f64 of them) for "cluster" and "cbox": per kind of ray (k % 16) the first 256 candidates the
    reference calls clear.
    Scene and origins lie in the positive octant.  On an axis its direction has an exact zero on, the slab test (the reference's,
    shader/scene.glsl:120-131: lo * (1 / d) - o * (1 / d)) forms inf - inf = NaN from a bound and an origin of one sign, which
    minNum / maxNum drop - the axis does not cull -, and -inf from a bound of the other sign: a box that straddles zero on that axis
    is never entered, wherever the origin is.  The counting is compared exactly either way; what `closest` finds is comparable with
    a brute force over the shapes only where every bound has the origin's sign."""
    cs = {"cluster": cluster, "cbox": cbox}[name]()
    cand = _candidates(cs, 5120 * 2, {"cluster": 101, "cbox": 202}[name])
    ref = V.closest_f64(cs, cand)
    ok = _clear(ref)
    # ray k of the set: the first clear candidate of kind k % 16 not used yet
    pick = np.zeros(NUM_RAYS, np.int64)
    for kind in range(16):
        have = np.nonzero(ok & (np.arange(len(cand)) % 16 == kind))[0]
        assert len(have) >= NUM_RAYS // 16, (name, kind, len(have))
        pick[kind::16] = have[:NUM_RAYS // 16]
    return cs, np.ascontiguousarray(cand[pick]), {k: v[pick] for k, v in ref.items()}


@functools.lru_cache(maxsize=None)
def cluster_rays(n):
    """n rays of any direction through the cluster and their closest_f64"""
    rays = _candidates(cluster(), 16 * n, 77)[0::16][:n]
    return rays, V.closest_f64(cluster(), rays)


def missing_rays(cs, n=256):
    """rays that start outside the scene's box and point away from it"""
    f = cs.bvh_f32
    rays = np.zeros((n, 8), np.float32)
    rng = np.random.default_rng(9)
    rays[:, 0:3] = f[0, 4:7] + rng.uniform(0.5, 1.0, (n, 3)).astype(np.float32)
    d = rng.uniform(0.1, 1.0, (n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6], rays[:, 7] = 1e-4, np.inf
    return rays


# ---------------------------------------------------------------------------------------------------------------- trees and gains
def inner_levels(nodes):
    """deepest level that holds an inner node, plus one (0: a single leaf)"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    depth = np.zeros(len(nodes), np.int64)
    levels = 0
    for i in np.nonzero(nodes[:, 3] == V.INNER)[0].tolist():            # pre-order: a parent comes before its children
        depth[i + 1] = depth[int(nodes[i + 1, 7])] = depth[i] + 1
        levels = max(levels, int(depth[i]) + 1)
    return levels


def right_spine(n):
    """every inner node's LEFT child is a leaf: inner nodes at the levels 0 ... n - 2"""
    return refit_scenes.chain_topology(n)


def root_exit_n(nodes):
    """the same tree in the other root-exit convention: the right spine leaves through N"""
    out = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8).copy()
    assert out[0, 7] == abi.BVH_ROOT_EXIT and len(out) < abi.BVH_ROOT_EXIT
    out[out[:, 7] == abi.BVH_ROOT_EXIT, 7] = len(out)
    return out


def root_exit_constant(nodes):
    out = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8).copy()
    out[out[:, 7] == len(out), 7] = abi.BVH_ROOT_EXIT
    return out


def random_gains(rng, nodes):
    """Python integers below 2^40, equal on both sides at every third record"""
    N = len(nodes)
    gl = [int(x) for x in rng.integers(0, 1 << 40, N)]
    gr = [int(x) for x in rng.integers(0, 1 << 40, N)]
    for k in range(0, N, 3):
        gr[k] = gl[k]
    return gl, gr


GAIN_SETS = ("zero", "ones", "random", "left 2^32", "right 2^32", "near 2^63")


def gains(kind, nodes, seed=0):
    N = len(nodes)
    if kind == "zero":
        return [0] * N, [0] * N
    if kind == "ones":
        return [0] * N, [1] * N
    if kind == "random":
        return random_gains(np.random.default_rng(100 + seed), nodes)
    if kind == "left 2^32":                                               # (a compare of the low words alone would exchange every node)
        return [1 << 32] * N, [1] * N
    if kind == "right 2^32":                                              # (... and here none)
        return [1] * N, [1 << 32] * N
    rng = np.random.default_rng(200 + seed)                              # near 2^63: the top bit set on one side or both, low words at odds
    top = rng.integers(0, 4, N)
    gl = [((1 << 63) if t & 1 else (1 << 63) - (1 << 32)) + int(x) for t, x in zip(top, rng.integers(0, 1 << 31, N))]
    gr = [((1 << 63) if t & 2 else (1 << 63) - (1 << 32)) + int(x) for t, x in zip(top, rng.integers(0, 1 << 31, N))]
    return gl, gr
