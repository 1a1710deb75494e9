"""Shared by tests/test_refit_host.py and tests/test_refit_gpu.py: deformations of a compiled scene that leave its emitters alone,
the refit of a flattened tree restated in numpy float32, the tree's surface-area cost in float64, a chain-shaped tree."""
import numpy as np

from hijiki_amd import abi, host

INNER = 0xFFFFFFFF


def shape_boxes(cs):
    """(lo, hi) per shape, float32: tests/test_gpu_parity.py::_shape_boxes (spheres, quads, triangles in global shape order)."""
    tri = cs.vertices[:, 0:3][cs.triangles]                               # (T, 3, 3)
    lo = [cs.spheres[:, 0:3] - cs.spheres[:, 3:4]] if len(cs.spheres) else []
    hi = [cs.spheres[:, 0:3] + cs.spheres[:, 3:4]] if len(cs.spheres) else []
    if len(cs.quads):
        o, e1, e2 = cs.quads[:, 0:3], cs.quads[:, 4:7], cs.quads[:, 8:11]
        corners = np.stack([o, o + e1, o + e2, (o + e1) + e2], axis=1)
        lo.append(corners.min(axis=1)); hi.append(corners.max(axis=1))
    if len(cs.triangles):
        lo.append(tri.min(axis=1)); hi.append(tri.max(axis=1))
    return np.concatenate(lo).astype(np.float32), np.concatenate(hi).astype(np.float32)


def refit_numpy(topology, boxes):
    """The refit restated: words 3 and 7 of `topology` stay, a leaf takes its shape's box, an inner node np.minimum / np.maximum of
    its two children's (left = next record, right = the left one's exit) - a reverse pass over the pre-order array, float32."""
    nodes = np.ascontiguousarray(topology, np.uint32).reshape(-1, 8).copy()
    f = nodes.view(np.float32)
    lo, hi = boxes
    f[:, 0:3] = 0
    f[:, 4:7] = 0
    leaf = nodes[:, 3] != INNER
    f[leaf, 0:3], f[leaf, 4:7] = lo[nodes[leaf, 3]], hi[nodes[leaf, 3]]
    inner = np.nonzero(~leaf)[0]
    right = nodes[inner + 1, 7].astype(np.int64)
    bmin, bmax = f[:, 0:3].copy(), f[:, 4:7].copy()
    for i, r in zip(inner[::-1].tolist(), right[::-1].tolist()):
        bmin[i] = np.minimum(bmin[i + 1], bmin[r])
        bmax[i] = np.maximum(bmax[i + 1], bmax[r])
    f[:, 0:3], f[:, 4:7] = bmin, bmax
    return nodes


def sa_cost(nodes):
    """Sum over inner nodes of area(node) / area(root) in float64 (extents taken in float64 from the float32 boxes)."""
    f = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8).view(np.float32).astype(np.float64)
    d = f[:, 4:7] - f[:, 0:3]
    area = np.where((d >= 0).all(axis=1), d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0], 0.0)
    inner = nodes[:, 3] == INNER
    return float(np.sum(area[inner] / area[0]))


def chain_topology(n):
    """A tree that is one long right spine over shapes 0 .. n-1 (every inner node's left child a leaf): the array
    tests/test_gpu_parity.py::test_device_vote_on_a_chain_deeper_than_its_level_loop builds, links only (boxes zero)."""
    N = 2 * n - 1
    end = max(N, abi.BVH_ROOT_EXIT)
    chain = np.zeros((N, 8), np.uint32)
    k = np.arange(n - 1)
    chain[2 * k, 3], chain[2 * k, 7] = INNER, end
    chain[2 * k + 1, 3], chain[2 * k + 1, 7] = k, 2 * k + 2
    chain[N - 1, 3], chain[N - 1, 7] = n - 1, end
    return chain


def sphere_chain_scene(n, seed=11):
    s = host.Scene()
    s.set_camera_cbox()
    m, e = s.add_diffuse((0.6, 0.6, 0.6)), s.add_emissive((9, 9, 9))
    rng = np.random.default_rng(seed)
    for k in range(n):
        s.add_sphere(tuple(rng.uniform(-0.9, 0.9, 3) + (0, 1, 0)), 0.01 + 0.02 * rng.random(), e if k % 600 == 0 else m)
    return s.compile()


class Deformation:
    """A seeded, smooth displacement of a compiled scene's shapes, written INTO the scene's arrays (`cs.vertices`, `cs.spheres`,
    `cs.quads` are views): vertex positions move by a sum of a few sines of their rest position, spheres are translated the same way
    and rescaled, quads translated.  Only shapes that are not emitters move - an emitter record carries the pdf the compiler
    derived from the shape's area -, shading normals and uv stay."""

    def __init__(self, cs, seed=1):
        self.cs = cs
        self.rest_vertices, self.rest_spheres, self.rest_quads = cs.vertices.copy(), cs.spheres.copy(), cs.quads.copy()
        ns, nq = len(cs.spheres), len(cs.quads)
        emissive = (cs.materials >> abi.MATERIAL_TAG_SHIFT) == abi.MAT_EMISSIVE
        emissive[cs.emitters[:, 0].astype(np.int64)] = True              # (global shape index: spheres, quads, triangles)
        self.emitter_shapes = emissive
        self.free_spheres = np.nonzero(~emissive[:ns])[0]
        self.free_quads = np.nonzero(~emissive[ns:ns + nq])[0]
        pinned = np.zeros(len(cs.vertices), bool)
        if len(cs.triangles):
            pinned[cs.triangles[emissive[ns + nq:]].reshape(-1)] = True  # every vertex of an emitter triangle, shared ones included
        self.pinned_vertices = pinned
        self.free_vertices = np.nonzero(~pinned)[0]
        lo, hi = shape_boxes(cs)
        self.extent = float((hi.max(axis=0) - lo.min(axis=0)).max())
        rng = np.random.default_rng(seed)
        self.freq = rng.uniform(1.0, 4.0, (4, 3)) * (2 * np.pi / self.extent)
        self.phase = rng.uniform(0, 2 * np.pi, 4)
        self.dirs = rng.normal(size=(4, 3))
        self.dirs /= np.linalg.norm(self.dirs, axis=1, keepdims=True)

    def _displacement(self, p, amplitude, t):
        w = np.sin(p.astype(np.float64) @ self.freq.T + self.phase + t)  # (n, 4)
        return ((amplitude * self.extent / 4.0) * (w @ self.dirs)).astype(np.float32)

    def apply(self, amplitude, t=0.0, vertices=None, spheres=None, quads=None):
        """Rest shape + displacement of relative `amplitude` (of the scene's extent) at time `t`.  `vertices` / `spheres` / `quads`:
        the indices that move (default: all that are not part of an emitter); naming one that is raises ValueError."""
        cs = self.cs
        vertices = self.free_vertices if vertices is None else np.asarray(vertices, np.int64)
        spheres = self.free_spheres if spheres is None else np.asarray(spheres, np.int64)
        quads = self.free_quads if quads is None else np.asarray(quads, np.int64)
        ns = len(cs.spheres)
        if self.pinned_vertices[vertices].any():
            raise ValueError("a vertex of an emitter triangle would move")
        if self.emitter_shapes[spheres].any() or self.emitter_shapes[ns + quads].any():
            raise ValueError("an emissive sphere or quad would move")
        v, s, q = cs.vertices, cs.spheres, cs.quads
        v[:], s[:], q[:] = self.rest_vertices, self.rest_spheres, self.rest_quads
        if len(vertices):
            v[vertices, 0:3] = self.rest_vertices[vertices, 0:3] + self._displacement(self.rest_vertices[vertices, 0:3], amplitude, t)
        if len(spheres):
            c = self.rest_spheres[spheres, 0:3]
            s[spheres, 0:3] = c + self._displacement(c, amplitude, t)
            s[spheres, 3] = self.rest_spheres[spheres, 3] * (1.0 + np.float32(5.0 * amplitude) * np.sin(c[:, 0] * 7.0 + np.float32(t))).astype(np.float32)
        if len(quads):
            o = self.rest_quads[quads, 0:3]
            q[quads, 0:3] = o + self._displacement(o, amplitude, t)
        # what the docstring promises, checked on the arrays as they now are
        em = self.emitter_shapes
        assert (v[self.pinned_vertices] == self.rest_vertices[self.pinned_vertices]).all()
        assert (s[em[:ns]] == self.rest_spheres[em[:ns]]).all() and (q[em[ns:ns + len(q)]] == self.rest_quads[em[ns:ns + len(q)]]).all()
        assert (v[:, 3:8] == self.rest_vertices[:, 3:8]).all()             # u, normal, v

    def restore(self):
        self.cs.vertices[:], self.cs.spheres[:], self.cs.quads[:] = self.rest_vertices, self.rest_spheres, self.rest_quads
