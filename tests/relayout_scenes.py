"""Shared by tests/test_relayout_host.py and tests/test_relayout_gpu.py: the scene matrix of the tree level and one ray per shape."""
import functools

import numpy as np

import refit_scenes
import scenes
from hijiki_amd import host

NONE = 0xFFFFFFFF


def _tiny(kind):
    s = host.Scene()
    s.set_camera_cbox()
    white, light = s.add_diffuse((0.7, 0.7, 0.7)), s.add_emissive((9, 9, 9))
    s.add_quad((-0.3, 1.9, -0.3), (0.6, 0, 0), (0, 0, 0.6), light)
    if kind == "quad+sphere":
        s.add_sphere((0.1, 0.6, 0.2), 0.4, white)
        return s.compile()
    pos = np.array([[-0.8, 0.1, 0.3], [0.7, 0.2, 0.1], [0.0, 1.1, -0.4], [0.6, 1.3, 0.5], [-0.5, 0.9, 0.6], [0.2, 0.4, -0.7]], np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(pos), 1))
    base = s.add_vertices(pos, nrm)
    s.add_triangle(base, base + 1, base + 2, white)
    if kind == "3 shapes":
        s.add_triangle(base + 3, base + 4, base + 5, white)
    return s.compile()


def _cbox():
    return host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=1280).compile()


def _chain():
    """a right spine of 700 spheres (tests/test_gpu_parity.py::test_device_vote_on_a_chain_deeper_than_its_level_loop): depth 699"""
    cs = refit_scenes.sphere_chain_scene(700)
    cs.set_bvh(refit_scenes.refit_numpy(refit_scenes.chain_topology(700), refit_scenes.shape_boxes(cs)))
    return cs


def _shrunk():
    """a third of the inner boxes shrunk to 0.8 (tests/test_gpu_parity.py::test_uploaded_tree_with_inconsistent_boxes): children stick
    out of them"""
    cs = _cbox()
    nodes, f = cs.bvh, cs.bvh_f32
    inner = np.nonzero(nodes[:, 3] == NONE)[0]
    rng = np.random.default_rng(5)
    for i in rng.choice(inner[1:], size=len(inner) // 3, replace=False):
        c = 0.5 * (f[i, 0:3] + f[i, 4:7])
        f[i, 0:3] = c + (f[i, 0:3] - c) * 0.8
        f[i, 4:7] = c + (f[i, 4:7] - c) * 0.8
    return cs


def _resident():
    """shapes only: the tree is built on the device and left there (upload with bvh == NULL)"""
    return host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile(with_tree=False)


BUILDERS = {
    "2 shapes": lambda: _tiny("2 shapes"), "3 shapes": lambda: _tiny("3 shapes"), "quad+sphere": lambda: _tiny("quad+sphere"),
    "cbox": _cbox, "cbox spheres": lambda: host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile(),
    "rich": lambda: scenes.rich_scene(7), "cluster": lambda: scenes.random_cluster_scene(77), "nasty": lambda: scenes.nasty_scene(3),
    "mesh 20k": lambda: host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=20000).compile(),
    "chain 700": _chain, "shrunk": _shrunk, "resident": _resident, "random": lambda: scenes.random_scene(3),
}
# The premise of the per-shape rays (tests/test_relayout_host.py): every shape must be found by its own ray (the others: 99 % of them).
EVERY_SHAPE = ("2 shapes", "3 shapes", "quad+sphere", "cbox", "cbox spheres", "mesh 20k", "chain 700", "shrunk", "resident")
# ... decided by the oracle's linear scan where the tree cannot serve: the resident scene's exists on the device only, and the shrunk
# boxes no longer contain their shapes - the oracle itself, walking them, misses 808 of the 1292 shapes.
PREMISE_BY_SCAN = ("shrunk", "resident")
# ... and asserted on random_scene(3) in place of nasty_scene(3), whose shapes coincide and degenerate on purpose: no ray singles out
# one of two coincident shapes (23 of its 36 shapes are found).  Its rays are sent and compared all the same.
NO_PREMISE = ("nasty",)
SWITCHED = ("cbox", "mesh 20k")                      # the scenes that also go up under the other switches


@functools.lru_cache(maxsize=None)
def scene(name):
    """the compiled scene, built once (tests that move its shapes restore them)"""
    return BUILDERS[name]()


def shape_rays(cs, seed=9, tilt=0.1):
    """One ray per shape, in shape order (spheres, quads, triangles), (shapes, 8) float32.  Triangle and quad: from the centroid plus
    delta times a unit vector w towards the centroid, w = the geometric normal tilted by `tilt` times a seeded unit vector; sphere: from
    centre + (r + delta) d towards the centre, d a seeded unit vector; window [delta / 4, 4 delta], delta = 1e-3 of the shape's largest
    extent and at least 1e-5.  The tilt is what the oracle asked for: along the plain normal of an axis-aligned wall the direction
    has two components of exactly 0, such a ray is outside general position ("two copies of the tree"), and the
    reference's slab test then misses the wall's own box from outside it - 12 wall triangles of the Cornell box were not found.
    tilt = 0 gives those rays: no premise holds for them, they walk the second copy of the tree."""
    rng = np.random.default_rng(seed)
    o, d, delta = [], [], []
    if len(cs.spheres):
        c, r = cs.spheres[:, 0:3].astype(np.float64), np.abs(cs.spheres[:, 3].astype(np.float64))
        u = rng.normal(size=c.shape)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        dl = np.maximum(1e-3 * 2.0 * r, 1e-5)
        o.append(c + (r + dl)[:, None] * u); d.append(-u); delta.append(dl)

    def flat(corners, normal):
        ext = (corners.max(axis=1) - corners.min(axis=1)).max(axis=1)
        length = np.linalg.norm(normal, axis=1, keepdims=True)
        n = np.where(length > 0, normal / np.where(length > 0, length, 1.0), [0.0, 0.0, 1.0])     # (a degenerate shape: any direction)
        g = rng.normal(size=n.shape)
        n = n + tilt * g / np.linalg.norm(g, axis=1, keepdims=True)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        dl = np.maximum(1e-3 * ext, 1e-5)
        o.append(corners.mean(axis=1) + dl[:, None] * n); d.append(-n); delta.append(dl)

    if len(cs.quads):
        q0, e1, e2 = (cs.quads[:, k:k + 3].astype(np.float64) for k in (0, 4, 8))
        flat(np.stack([q0, q0 + e1, q0 + e2, q0 + e1 + e2], axis=1), np.cross(e1, e2))
    if len(cs.triangles):
        tri = cs.vertices[:, 0:3].astype(np.float64)[cs.triangles]
        flat(tri, np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
    rays = np.zeros((sum(len(x) for x in o), 8), np.float32)
    rays[:, 0:3], rays[:, 3:6] = np.concatenate(o), np.concatenate(d)
    dl = np.concatenate(delta)
    rays[:, 6], rays[:, 7] = dl / 4.0, dl * 4.0
    return rays
