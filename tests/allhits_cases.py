"""Shared by tests/test_allhits_host.py and tests/test_allhits_gpu.py: the scenes, the hand-built scenes with their hand-written trees
and expected counts, the ray sets and the containment fixtures.  Everything is computed once and never written to."""
import functools

import numpy as np

import allhits_ref as A
import scenes
from refit_scenes import chain_topology, refit_numpy, shape_boxes
from hijiki_amd import host

U, F = np.uint32, np.float32
INF, NAN = float("inf"), float("nan")
N_RAYS = 3001                                            # a multiple of neither 64 nor 256


def _new_scene():
    s = host.Scene()
    s.set_camera((0, 0, 5), (0, 0, 0, 1), 40.0)
    return s, s.add_diffuse((0.5, 0.5, 0.5))


def _chained(s):
    """compiled, under a hand-written tree: one long right spine over the shapes in index order, boxes refitted in numpy"""
    cs = s.compile()
    n = len(cs.spheres) + len(cs.quads) + len(cs.triangles)
    cs.set_bvh(refit_numpy(chain_topology(n), shape_boxes(cs)))
    return cs


def stack_scene():
    """Two concentric spheres about the origin (shapes 0, 1: radius 1 and 2) and five parallel unit-normal quads across the z axis at
    z = 3 .. 7 (shapes 2 .. 6), the quads at z = 4 and z = 6 turned over (edges exchanged: n_g points to -z)."""
    s, m = _new_scene()
    s.add_sphere((0, 0, 0), 1.0, m)
    s.add_sphere((0, 0, 0), 2.0, m)
    for k, z in enumerate((3.0, 4.0, 5.0, 6.0, 7.0)):
        if k % 2 == 0:
            s.add_quad((-1, -1, z), (2, 0, 0), (0, 2, 0), m)
        else:
            s.add_quad((-1, -1, z), (0, 2, 0), (2, 0, 0), m)
    return _chained(s)


def coincident_scene():
    """the same quad twice (shapes 0 and 1) and a third behind them"""
    s, m = _new_scene()
    s.add_quad((-1, -1, 1), (2, 0, 0), (0, 2, 0), m)
    s.add_quad((-1, -1, 1), (2, 0, 0), (0, 2, 0), m)
    s.add_quad((-1, -1, 2), (2, 0, 0), (0, 2, 0), m)
    return _chained(s)


# (scene, ray, count, crossing sum, shape indices in key order).  Every value below is exact in float32 (o = (0.25, 0.5, .) along
# +-z: l.l, b and the discriminants are dyadic), so the orders are certain.
#   through all:   from z = -5 along +z: outer sphere in (t = 5 - sqrt(4 - 0.3125)), inner in, inner out, outer out, then the five
#                  quads at t = 8 .. 12: 9 candidates; spheres -1 -1 +1 +1, quads +1 -1 +1 -1 +1 (d = +z against n_g = +z, -z, ...): +1
#   between:       from z = -1.5, between the two spheres, along +z with tMax = 4.75 (z <= 3.25): the outer sphere's near root is
#                  behind the origin (t0 < 0 = tMin: no candidate), so inner in (-1), inner out (+1), outer out (+1), the quad at z = 3
#                  (+1): 4 candidates, sum +2 - the ray starts inside ONE closed surface (the outer sphere) and crosses one open sheet
#   backwards:     the same origin along -z, unbounded: only the outer sphere's far root: 1 candidate, sum +1
#   cut:           through all with tMin = 6 and tMax = 10: outer out (t = 5 + sqrt(3.6875) = 6.92), quads at t = 8, 9, 10: 4, sum +1 +1 -1 +1
HAND = (
    ("stack", (0.25, 0.5, -5, 0, 0, 1, 0, INF), 9, 1, (1, 0, 0, 1, 2, 3, 4, 5, 6)),
    ("stack", (0.25, 0.5, -1.5, 0, 0, 1, 0, 4.75), 4, 2, (0, 0, 1, 2)),
    ("stack", (0.25, 0.5, -1.5, 0, 0, -1, 0, INF), 1, 1, (1,)),
    ("stack", (0.25, 0.5, -5, 0, 0, 1, 6, 10), 4, 2, (1, 2, 3, 4)),
    # two coincident quads tie on t and order by index; the third follows; from behind they come the other way round, the tie as before
    ("coincident", (0.25, 0.5, 0, 0, 0, 1, 0, INF), 3, 3, (0, 1, 2)),
    ("coincident", (0.25, 0.5, 3, 0, 0, -1, 0, INF), 3, -3, (2, 0, 1)),
)


def cube_scene(flipped=False, with_sphere=True):
    """A closed cube [-1, 1]^3 of 12 triangles, oriented outward (flipped: every triangle turned over), and a sphere of radius 0.5 at
    (3, 0, 0) beside it."""
    s, m = _new_scene()
    corners = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], F)
    b = s.add_vertices(corners, np.tile(F([0, 0, 1]), (8, 1)))
    quads = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))          # each counter-clockwise seen from outside
    tris = []
    for q in quads:
        for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
            tris.append((t[0], t[2], t[1]) if flipped else t)
    s.add_triangles(np.array(tris, U) + b, m)
    if with_sphere:
        s.add_sphere((3, 0, 0), 0.5, m)
    return s.compile()


def cube_points():
    """grid points inside, outside and within 1e-3 of the faces of the cube, and in and about the sphere -> (n, 4); masks: strictly
    interior by at least 0.05, exterior by at least 0.05 (of the cube and the sphere both)"""
    ax = np.array([-1.5, -1.001, -0.9995, -0.95, -0.5, 0.0, 0.3, 0.95, 0.9995, 1.001, 1.5], F)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(9)
    ball = (F([3, 0, 0]) + rng.uniform(-0.8, 0.8, (200, 3))).astype(F)
    p = np.concatenate([g, ball]).astype(F)
    cheb = np.abs(p).max(1)
    rad = np.linalg.norm(p.astype(np.float64) - [3, 0, 0], axis=1)
    inside = (cheb <= 0.95) | (rad <= 0.45)
    outside = (cheb >= 1.05) & (rad >= 0.55)
    pts = np.concatenate([p, np.zeros((len(p), 1), F)], 1).astype(F)
    return pts, inside, outside


def _surface_points(rng, sh, m):
    t = np.concatenate([sh["quads"], sh["triangles"]])
    pick = t[rng.integers(0, len(t), m)]
    u, v = rng.uniform(0, 1, (m, 1)), rng.uniform(0, 1, (m, 1))
    fold = (u + v) > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)                  # (inside the triangle, and inside the quad)
    return (pick[:, 0] + pick[:, 1] * u + pick[:, 2] * v).astype(F)


def ray_set(cs, sh, seed=5):
    """N_RAYS rays of every kind, shuffled so that every prefix holds every kind: camera rays (one origin outside, a grid of unit
    directions), rays between random surface points (unit directions), axis-parallel rays with exact zeros through surface points,
    rays with tMin > 0 and a finite tMax that cuts the list, zero-length and NaN directions, NaN origins, infinite components."""
    rng = np.random.default_rng(seed)
    lo, hi = shape_boxes(cs)
    lo, hi = lo.min(0), hi.max(0)
    mid, ext = (lo + hi) / 2, (hi - lo)
    unit = lambda d: d / np.linalg.norm(d, axis=1, keepdims=True)              # noqa: E731
    rays = np.zeros((N_RAYS, 8), F)
    rays[:, 7] = INF
    # camera rays
    k = 1000
    eye = mid + ext * [0.1, 0.2, 1.4]
    target = mid + rng.uniform(-0.6, 0.6, (k, 3)) * ext
    rays[:k, 0:3], rays[:k, 3:6] = eye, unit(target - eye)
    # between surface points, starting before the first and running on
    a, b = _surface_points(rng, sh, 1200), _surface_points(rng, sh, 1200)
    d = unit(b - a + 1e-9)
    rays[k:k + 1200, 0:3], rays[k:k + 1200, 3:6] = a - d * 0.37 * np.linalg.norm(ext), d
    k += 1200
    # axis-parallel with exact zeros, through surface points and through box corners of the scene
    p = _surface_points(rng, sh, 400)
    axis = rng.integers(0, 3, 400)
    sign = rng.choice([-1.0, 1.0], 400)
    d = np.zeros((400, 3))
    d[np.arange(400), axis] = sign
    o = p - d * ext.max() * 1.5
    o[:40] = np.where(d[:40] != 0, o[:40], lo)                                 # (on the scene box's own planes: 0 * inf in the box test)
    rays[k:k + 400, 0:3], rays[k:k + 400, 3:6] = o, d
    rays[k:k + 400:7, 3:6] *= np.where(d[::7] == 0, -1.0, 1.0)                 # (negative zeros)
    k += 400
    # a window [tMin, tMax] inside the scene
    a, b = _surface_points(rng, sh, 300), _surface_points(rng, sh, 300)
    d = unit(b - a + 1e-9)
    L = np.linalg.norm(ext)
    rays[k:k + 300, 0:3], rays[k:k + 300, 3:6] = a - d * L, d
    rays[k:k + 300, 6], rays[k:k + 300, 7] = L * rng.uniform(0.8, 1.1, 300), L * rng.uniform(1.1, 1.6, 300)
    k += 300
    # degenerate: zero-length, NaN and infinite directions, a NaN origin, an empty and a NaN range
    rest = N_RAYS - k
    o = mid + rng.uniform(-0.4, 0.4, (rest, 3)) * ext
    d = unit(rng.normal(size=(rest, 3)))
    rays[k:, 0:3], rays[k:, 3:6] = o, d
    kinds = np.arange(rest) % 8
    rays[k:, 3:6][kinds == 0] = 0.0
    rays[k:, 3:6][kinds == 1] = NAN
    rays[k:, 4][kinds == 2] = NAN
    rays[k:, 5][kinds == 3] = INF
    rays[k:, 0][kinds == 4] = NAN
    rays[k:, 6][kinds == 5], rays[k:, 7][kinds == 5] = 1.0, 0.5
    rays[k:, 7][kinds == 6] = NAN
    rays[k:, 3:6][kinds == 7] = [0.0, -0.0, 0.0]
    rays = rays[rng.permutation(N_RAYS)]
    return np.ascontiguousarray(rays, F)


SCENES = {
    "cbox": lambda: host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=200).compile(),
    "mesh": lambda: scenes.smooth_mesh_scene(11),                         # 1 sphere, 1 quad, 1244 triangles
    "stack": stack_scene,
    "coincident": coincident_scene,
}


@functools.lru_cache(maxsize=None)
def scene(name):
    cs = SCENES[name]()
    return cs, A.shapes_of(cs)


@functools.lru_cache(maxsize=None)
def case(name):
    """(compiled scene, shape records, rays): the big scenes get the N_RAYS set; the hand-built ones their HAND rays first, then a
    small set of the same kinds"""
    cs, sh = scene(name)
    rays = ray_set(cs, sh)
    if name in ("stack", "coincident"):
        hand = np.array([h[1] for h in HAND if h[0] == name], F)
        rays = np.concatenate([hand, rays[:321 - len(hand)]])
    rays.setflags(write=False)
    return cs, sh, rays


@functools.lru_cache(maxsize=None)
def want(name):
    """the reference's (counts, crossings, hits at K = 8) of case(name) under the scene's own host tree"""
    cs, sh, rays = case(name)
    out = A.all_hits(sh, cs.bvh, rays, A.MAX_HITS)
    for x in out:
        x.setflags(write=False)
    return out
