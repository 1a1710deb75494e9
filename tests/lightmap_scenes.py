"""Scenes of the light-map tests (tests/test_lightmap_host.py, tests/test_lightmap_gpu.py): seeded and small.  Every triangle has
three vertices of its own, so a triangle's index is its place in the list it was built from."""
import functools

import numpy as np

from hijiki_amd import abi, host

F = np.float32


def _add_mesh(s, uv, pos, nrm, material):
    """uv (n, 3, 2), pos, nrm (n, 3, 3) -> n triangles behind whatever the scene holds already"""
    uv, pos, nrm = np.asarray(uv, F), np.asarray(pos, F), np.asarray(nrm, F)
    base = s.add_vertices(pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2))
    s.add_triangles(base + np.arange(3 * len(uv)).reshape(-1, 3), material)


EDGE_CASES = ("quad lower", "quad upper", "vertex on a centre", "overlap low", "overlap high", "partly outside", "wholly outside", "zero area",
              "collinear", "collinear through centres", "nan uv", "inf uv", "sliver", "zero normals", "cancelling normals")


@functools.lru_cache(maxsize=None)
def edge_scene():
    """About 40 triangles behind 2 spheres and 1 quad (so a triangle's shape index is not its triangle index), laid out for a 64 x 64
    atlas, whose texel centres are the odd multiples of 1/128.  The first len(EDGE_CASES) triangles are those cases, in that order;
    random triangles follow.  Positions are random (the uv footprints say nothing about the geometry); normals random unless the
    case is about them.  -> (compiled scene, index of each case)"""
    rng = np.random.default_rng(41)
    c = lambda x, y: (x / 64.0, y / 64.0)                                  # noqa: E731  texel-corner coordinates
    m = lambda x, y: ((x + 0.5) / 64.0, (y + 0.5) / 64.0)                  # noqa: E731  the centre of texel (x, y)
    uv = [
        [c(8, 8), c(24, 8), c(24, 24)],                                    # a quad's two triangles: the diagonal runs through centres
        [c(8, 8), c(24, 24), c(8, 24)],
        [m(40, 8), m(50, 8), m(40, 20)],                                   # vertices, two edges and the hypotenuse's ends on centres
        [c(30, 30), c(50, 32), c(34, 52)],                                 # two that overlap: the lower index wins
        [c(36, 28), c(56, 40), c(38, 50)],
        [(-0.2, 0.5), (0.1, 0.4), (0.05, 0.7)],
        [(1.2, 1.2), (1.5, 1.3), (1.3, -1.6)],
        [c(5, 40), c(5, 40), c(5, 40)],
        [(0.6, 0.6), (0.7, 0.7), (0.8, 0.8)],
        [m(10, 60), m(20, 60), m(30, 60)],                                 # every edge value is zero on the centres of row 60
        [(np.nan, 0.2), (0.3, 0.2), (0.3, 0.4)],
        [(0.1, 0.1), (np.inf, 0.2), (0.2, 0.3)],
        [(5 / 64.0, 0.8000), (58 / 64.0, 0.8100), (58 / 64.0, 0.8140)],     # under a third of a texel high, 53 columns long
        [c(3, 44), c(14, 45), c(4, 58)],
        [m(36, 40), m(52, 40), m(36, 56)],                                 # hu = i / 16, hv = j / 16 at the centre (36 + i, 40 + j)
    ]
    assert len(uv) == len(EDGE_CASES)
    extra = 26
    centre = rng.uniform(0.0, 1.0, (extra, 1, 2))
    uv = np.concatenate([np.array(uv, np.float64), centre + rng.uniform(-0.12, 0.12, (extra, 3, 2))]).astype(F)
    n = len(uv)
    pos = rng.uniform([-1.0, 0.1, -1.0], [1.0, 1.9, 1.0], (n, 1, 3)) + rng.uniform(-0.3, 0.3, (n, 3, 3))
    nrm = rng.normal(size=(n, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[EDGE_CASES.index("zero normals")] = 0.0
    nrm[EDGE_CASES.index("cancelling normals")] = [[0, 1, 0], [0, -1, 0], [0, 1, 0]]   # (l0 - hu) + hv = 0 exactly where hu = 1/2
    s = host.Scene()
    s.set_camera((0.0, 1.0, 3.3), (0.0, 0.0, 0.0, 1.0), 40.0)
    white = s.add_diffuse((0.7, 0.7, 0.7))
    s.add_sphere((-0.5, 0.4, 0.2), 0.3, white)
    s.add_sphere((0.5, 0.3, -0.2), 0.25, s.add_mirror())
    s.add_quad((-1.3, 0.0, 1.3), (2.6, 0.0, 0.0), (0.0, 0.0, -2.6), white)
    _add_mesh(s, uv, pos, nrm, white)
    cs = s.compile()
    assert len(cs.spheres) == 2 and len(cs.quads) == 1 and len(cs.triangles) == n
    return cs, {name: i for i, name in enumerate(EDGE_CASES)}


def _pair(u0, v0, u1, v1, y=0.0):
    """an upward rectangle (x, z) = (u, v) scaled to [-1, 1] at height y, as two triangles that share the diagonal"""
    q = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
    uv = np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], F)
    pos = np.zeros((2, 3, 3), F)
    pos[:, :, 0], pos[:, :, 1], pos[:, :, 2] = 2 * uv[:, :, 0] - 1, y, 2 * uv[:, :, 1] - 1
    nrm = np.zeros((2, 3, 3), F)
    nrm[:, :, 1] = 1.0
    return uv, pos, nrm


@functools.lru_cache(maxsize=None)
def full_pair_scene():
    """one triangle pair over all of [0, 1]^2"""
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    _add_mesh(s, *_pair(0.0, 0.0, 1.0, 1.0), s.add_diffuse((0.6, 0.6, 0.6)))
    return s.compile()


@functools.lru_cache(maxsize=None)
def tiny_scene(n=20000, side=512):
    """n triangles of under one texel of a side x side atlas each, and a floor quad"""
    rng = np.random.default_rng(43)
    centre = rng.uniform(0.0, 1.0, (n, 1, 2))
    uv = (centre + rng.uniform(-0.45, 0.45, (n, 3, 2)) / side).astype(F)
    pos = np.zeros((n, 3, 3), F)
    pos[:, :, 0], pos[:, :, 2] = 2 * uv[:, :, 0] - 1, 2 * uv[:, :, 1] - 1
    pos[:, :, 1] = rng.uniform(0.1, 1.0, (n, 3))
    nrm = rng.normal(size=(n, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    white = s.add_diffuse((0.7, 0.7, 0.7))
    s.add_quad((-1.3, 0.0, 1.3), (2.6, 0.0, 0.0), (0.0, 0.0, -2.6), white)
    _add_mesh(s, uv, pos, nrm, white)
    return s.compile()


def _box_scene(s, floor):
    """A UV-mapped floor (two triangles, chart [0.02, 0.6] x [0.05, 0.95]) and a UV-mapped box standing on it (top and four sides,
    one chart each in the strip u > 0.64) in `s`."""
    uv, pos, nrm = _pair(0.02, 0.05, 0.6, 0.95)
    pos[:, :, 0], pos[:, :, 2] = 2.4 * (uv[:, :, 0] - 0.02) / 0.58 - 1.2, 2.4 * (uv[:, :, 1] - 0.05) / 0.9 - 1.2
    _add_mesh(s, uv, pos, nrm, floor)
    lo, hi = np.array([-0.5, 0.0, -0.4]), np.array([0.1, 0.7, 0.3])
    faces = [((0, 1, 0), 1, (0, 2)), ((1, 0, 0), 0, (2, 1)), ((-1, 0, 0), 0, (1, 2)), ((0, 0, 1), 2, (0, 1)), ((0, 0, -1), 2, (1, 0))]
    uvs, poss, nrms = [], [], []
    for k, (n, axis, (a, b)) in enumerate(faces):
        u0, v0 = 0.66, 0.03 + 0.19 * k
        quv = np.array([(u0, v0), (u0 + 0.3, v0), (u0 + 0.3, v0 + 0.16), (u0, v0 + 0.16)])
        corner = np.zeros((4, 3))
        corner[:, axis] = hi[axis] if sum(n) > 0 else lo[axis]
        corner[:, a] = [lo[a], hi[a], hi[a], lo[a]]
        corner[:, b] = [lo[b], lo[b], hi[b], hi[b]]
        for tri in ((0, 1, 2), (0, 2, 3)):
            uvs.append(quv[list(tri)]); poss.append(corner[list(tri)]); nrms.append(np.tile(np.array(n, float), (3, 1)))
    _add_mesh(s, np.array(uvs), np.array(poss), np.array(nrms), s.add_diffuse((0.3, 0.5, 0.7)))


@functools.lru_cache(maxsize=None)
def bake_scene(env=False):
    """A Cornell-like box - quad walls and ceiling, an area light - around _box_scene; env: open instead (no walls, no ceiling, no
    light) under a small sky"""
    s = host.Scene()
    s.set_camera_cbox()
    white = s.add_diffuse((0.7, 0.7, 0.7))
    if env:
        import env_scenes
        s.add_sphere((0.6, 0.3, 0.5), 0.3, white)
        s.set_environment(s.add_texture(env_scenes.sky_texels(8, 16), abi.TEX_BILINEAR), 1.5)
    else:
        s.add_quad((-1.2, 0, -1.2), (2.4, 0, 0), (0, 2.0, 0), white)
        s.add_quad((-1.2, 0, 1.2), (0, 0, -2.4), (0, 2.0, 0), s.add_diffuse((0.6, 0.1, 0.1)))
        s.add_quad((1.2, 0, -1.2), (0, 0, 2.4), (0, 2.0, 0), s.add_diffuse((0.1, 0.6, 0.1)))
        s.add_quad((-1.2, 2.0, -1.2), (2.4, 0, 0), (0, 0, 2.4), white)
        s.add_quad((-0.4, 1.99, -0.4), (0.8, 0, 0), (0, 0, 0.8), s.add_emissive((15.0, 14.0, 12.0)))
    _box_scene(s, white)
    return s.compile()


@functools.lru_cache(maxsize=None)
def sky_pair_scene():
    """one upward triangle pair (chart [0.25, 0.75]^2) alone under the constant sky of 0.5"""
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    _add_mesh(s, *_pair(0.25, 0.25, 0.75, 0.75), s.add_diffuse((0.5, 0.5, 0.5)))
    s.set_environment(s.add_texture(np.full((4, 8, 4), 0.5, F), abi.TEX_NEAREST))
    return s.compile()


def moved(cs, seed=7):
    """cs.vertices moved in place: positions jittered, normals turned (uv untouched) -> the arrays before the move"""
    rng = np.random.default_rng(seed)
    v = cs.vertices
    keep = v.copy()
    v[:, 0:3] += rng.uniform(-0.05, 0.05, (len(v), 3)).astype(F)
    n = v[:, 4:7] + rng.uniform(-0.3, 0.3, (len(v), 3)).astype(F)
    live = (keep[:, 4:7] != 0).any(axis=1)
    v[live, 4:7] = n[live]
    return keep
