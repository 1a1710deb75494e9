"""Shared by tests/test_lbvh_edges_host.py and tests/test_lbvh_edges_gpu.py ("Build level"): what EVERY correct device
build and refit must give, decided exactly - a valid pre-order skip-link tree, every shape in one leaf, each leaf its shape's box
word for word, each inner node the exact union of its two children's boxes - and the scenes that put the build's kernels at their
size and value edges.  The union is the ORDERED minimum / maximum (-0 < +0, the integer keys of kernels/hj_lbvh.h `ordered()`); no
build decision (Morton codes, hierarchy, SAH) is restated here.  numpy and the host library only: no GPU."""
import functools

import numpy as np

import refit_scenes
from hijiki_amd import abi, host

INNER = 0xFFFFFFFF
NEG_ZERO, POS_ZERO = 0x80000000, 0x00000000
BOX = (0, 1, 2, 4, 5, 6)                               # the six box words of a record


# ---------------------------------------------------------------------------------------------------------------- the reference
def ordered(words):
    """kernels/hj_lbvh.h ordered(): the int whose order is the float's, -0 (key -1) below +0 (key 0); `words`: uint32"""
    i = np.asarray(words, np.uint32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF)


def omin(a, b):
    return np.where(ordered(a) <= ordered(b), a, b).astype(np.uint32)


def omax(a, b):
    return np.where(ordered(a) >= ordered(b), a, b).astype(np.uint32)


def _w(f):
    return np.ascontiguousarray(f, np.float32).view(np.uint32)


def shape_box_words(cs):
    """(lo, hi) per shape as uint32 words, (shapes, 3) each, in global shape order (spheres, quads, triangles): the float32
    operations of kernels/hj_lbvh.h shape_box (c - r, c + r; O, O + A, O + B, (O + A) + B; the three vertices), the minimum and maximum
    over a shape's corners taken in the order of the keys."""
    lo, hi = [], []

    def over(corners):                                                    # (shapes, k, 3) float32
        w = _w(corners)
        a, b = w[:, 0], w[:, 0]
        for k in range(1, w.shape[1]):
            a, b = omin(a, w[:, k]), omax(b, w[:, k])
        lo.append(a); hi.append(b)
    if len(cs.spheres):
        c, r = cs.spheres[:, 0:3], cs.spheres[:, 3:4]
        over(np.stack([c - r, c + r], axis=1))
    if len(cs.quads):
        o, e1, e2 = cs.quads[:, 0:3], cs.quads[:, 4:7], cs.quads[:, 8:11]
        over(np.stack([o, o + e1, o + e2, (o + e1) + e2], axis=1))
    if len(cs.triangles):
        over(cs.vertices[:, 0:3][cs.triangles])
    return np.concatenate(lo), np.concatenate(hi)


def _structure(nodes):
    """The structure rules of tests/test_gpu_parity.py::_check_skip_link_tree (src/main.rs:203-231); returns per inner node its right
    child, -1 for leaves."""
    N = len(nodes)
    inner = nodes[:, 3] == INNER
    shapes = nodes[~inner, 3]
    assert N == 2 * len(shapes) - 1, f"structure: {N} records for {len(shapes)} leaves"
    assert sorted(shapes.tolist()) == list(range(len(shapes))), "structure: not every shape sits in exactly one leaf"
    exits = nodes[:, 7].astype(np.int64)
    assert (exits > np.arange(N)).all(), "structure: an exit does not move forward"
    assert exits[0] == max(abi.BVH_ROOT_EXIT, N), "structure: the root's exit"
    size = np.zeros(N, np.int64)
    right = np.full(N, -1, np.int64)
    inner_l, exit_l = inner.tolist(), exits.tolist()
    for i in range(N - 1, -1, -1):                                        # pre-order: left child = next record
        if not inner_l[i]:
            size[i] = 1
            continue
        l = i + 1
        assert l < N, f"structure: inner node {i} is the last record"
        r = l + int(size[l])
        assert r < N and exit_l[l] == r, f"structure: the exit of {l}, left child of {i}, is not its sibling"
        size[i] = 1 + size[l] + size[r]
        end = i + int(size[i])
        assert exit_l[r] == exit_l[i], f"structure: the right child of {i} does not inherit its exit"
        assert exit_l[i] == (end if end < N else exit_l[0]), f"structure: the exit of {i} is not the end of its subtree"
        right[i] = r
    assert size[0] == N, "structure: the root's subtree is not the array"
    return right


def check_built_tree(nodes, cs):
    """`nodes`: (N, 8) uint32, a tree over the shapes of `cs` as they are now.  Structure; words 0-2 and 4-6 of a leaf are its shape's
    box; those of an inner node the ordered minimum / maximum of its two children's words."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    right = _structure(nodes)
    lo, hi = shape_box_words(cs)
    leaf = np.nonzero(nodes[:, 3] != INNER)[0]
    bad = (nodes[leaf, 0:3] != lo[nodes[leaf, 3]]).any(axis=1) | (nodes[leaf, 4:7] != hi[nodes[leaf, 3]]).any(axis=1)
    assert not bad.any(), f"leaf box: record {int(leaf[np.argmax(bad)])} does not hold the box of shape {int(nodes[leaf[np.argmax(bad)], 3])} word for word"
    i = np.nonzero(right >= 0)[0]
    l, r = i + 1, right[i]
    bad = (nodes[i, 0:3] != omin(nodes[l, 0:3], nodes[r, 0:3])).any(axis=1) | (nodes[i, 4:7] != omax(nodes[l, 4:7], nodes[r, 4:7])).any(axis=1)
    if bad.any():
        k = int(i[np.argmax(bad)])
        raise AssertionError(f"inner box: record {k} is not the ordered union of its children {k + 1} and {int(right[k])} "
                             f"({int(bad.sum())} such nodes): {nodes[k, list(BOX)]} against {nodes[k + 1, list(BOX)]} and {nodes[right[k], list(BOX)]}")


def refit_reference(topology, cs):
    """refit_scenes.refit_numpy with the ordered minimum / maximum: the links of `topology` stay, a leaf takes its shape's box, an
    inner node the union of its two children's - a reverse pass over the pre-order array on the integer keys."""
    nodes = np.ascontiguousarray(topology, np.uint32).reshape(-1, 8).copy()
    lo, hi = shape_box_words(cs)
    nodes[:, 0:3] = 0
    nodes[:, 4:7] = 0
    leaf = nodes[:, 3] != INNER
    nodes[leaf, 0:3], nodes[leaf, 4:7] = lo[nodes[leaf, 3]], hi[nodes[leaf, 3]]
    inner = np.nonzero(~leaf)[0]
    right = nodes[inner + 1, 7].astype(np.int64)
    keys = ordered(nodes[:, list(BOX)]).tolist()
    for i, r in zip(inner[::-1].tolist(), right[::-1].tolist()):
        a, b = keys[i + 1], keys[r]
        keys[i] = [min(a[0], b[0]), min(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]), max(a[4], b[4]), max(a[5], b[5])]
    k = np.array(keys, np.int64)
    nodes[:, list(BOX)] = (np.where(k >= 0, k, k ^ 0x7FFFFFFF) & 0xFFFFFFFF).astype(np.uint32)      # ordered() is its own inverse
    return nodes


def record_multiset(nodes):
    """the records' boxes and shapes (words 0-6), sorted: what an exchange of children must keep"""
    rows = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)[:, 0:7]
    return rows[np.lexsort(rows.T[::-1])]


def has_both_zeros(nodes):
    """inner nodes one of whose box words is -0 from one child and +0 from the other"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    i = np.nonzero(nodes[:, 3] == INNER)[0]
    l, r = i + 1, nodes[i + 1, 7].astype(np.int64)
    a, b = nodes[l][:, list(BOX)], nodes[r][:, list(BOX)]
    return int((((a == NEG_ZERO) & (b == POS_ZERO)) | ((a == POS_ZERO) & (b == NEG_ZERO))).any(axis=1).sum())


# ---------------------------------------------------------------------------------------------------------------- topologies
def topology(n, left_leaves):
    """Links (boxes zero) of the tree over shapes 0 .. n-1 in which a node over m >= 2 shapes at `depth` gives its first
    left_leaves(m, depth) shapes to its left child: pre-order, exit = the end of the subtree, or the root's exit where the array ends."""
    N = 2 * n - 1
    end = max(N, abi.BVH_ROOT_EXIT)
    out = np.zeros((N, 8), np.uint32)
    stack = [(0, n, 0, 0)]                                                # first shape, shapes, position, depth
    while stack:
        lo, m, pos, depth = stack.pop()
        stop = pos + 2 * m - 1
        out[pos, 7] = stop if stop < N else end
        if m == 1:
            out[pos, 3] = lo
            continue
        out[pos, 3] = INNER
        k = int(left_leaves(m, depth))
        assert 1 <= k < m
        stack.append((lo + k, m - k, pos + 2 * k, depth + 1))
        stack.append((lo, k, pos + 1, depth + 1))
    return out


def balanced_topology(n):
    return topology(n, lambda m, d: m // 2)


def left_spine_topology(n):
    """every inner node's RIGHT child is a leaf: the inner nodes are records 0 .. n-2, one behind the other"""
    return topology(n, lambda m, d: m - 1)


def boundary_topology(n=1025):
    """the root's left subtree has exactly 1023 records: left child at 1 .. 1023, right child at record 1024, the first of the second run"""
    return topology(n, lambda m, d: 512 if d == 0 else m // 2)


REFIT_SIZES = (512, 513, 1024, 1025)
REFIT_TOPOLOGIES = {"balanced": balanced_topology, "chain": refit_scenes.chain_topology, "left spine": left_spine_topology}


# ---------------------------------------------------------------------------------------------------------------- scenes
def _compile(spheres=(), quads=(), vertices=None, triangles=(), emitter=0):
    """spheres: (x, y, z, r) rows; quads: (origin, edge1, edge2); vertices (V, 3) and index triples.  Shape `emitter` (global index)
    is the light; shapes only, no tree."""
    s = host.Scene()
    s.set_camera_cbox()
    white, light = s.add_diffuse((0.7, 0.7, 0.7)), s.add_emissive((9, 9, 9))
    k = 0
    for sp in spheres:
        s.add_sphere(tuple(float(x) for x in sp[0:3]), float(sp[3]), light if k == emitter else white)
        k += 1
    for o, e1, e2 in quads:
        s.add_quad(o, e1, e2, light if k == emitter else white)
        k += 1
    if len(triangles):
        v = np.asarray(vertices, np.float32).reshape(-1, 3)
        base = s.add_vertices(v, np.tile(np.float32([0, 0, 1]), (len(v), 1)))
        for a, b, c in triangles:
            s.add_triangle(base + a, base + b, base + c, light if k == emitter else white)
            k += 1
    return s.compile(with_tree=False)


STEP = 2.0 ** -18                                      # positions and radii of the degenerate blobs are multiples: sums stay exact


def _blob_positions(gen, a, rng):
    """`a` centroids with x < 0.25 in [0, 1]^3, float64 values that are float32 numbers"""
    if gen == "random":
        p = rng.uniform(0.0, 1.0, (a, 3))
        p[:, 0] = 0.01 + 0.23 * p[:, 0]
    elif gen in ("equal", "line", "plane"):
        p = np.tile([0.125, 0.5, 0.5], (a, 1))
        free = {"equal": 0, "line": 1, "plane": 2}[gen]
        p[:, :free] = rng.integers(1 << 12, 1 << 15, (a, free)) * STEP    # 0.0156 .. 0.125, exact
    elif gen == "exp":
        p = np.tile([0.0, 0.5, 0.5], (a, 1))
        p[:, 0] = 0.2 * 2.0 ** -np.arange(a, dtype=np.float64)
    elif gen == "grid":
        g = int(np.ceil(a ** (1.0 / 3.0)))
        ijk = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)[:a]
        p = (ijk + 1.0) / (g + 1.0) * [0.24, 1.0, 1.0]
    else:
        raise KeyError(gen)
    return p.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def blob_scene(gen, a, b, seed=1):
    """Spheres 0 .. a-1: blob A (generator `gen`, centroids at x < 0.25), spheres a .. a+b-1: blob B (random, x > 0.75); radii about
    1e-3, all different (multiples of 2^-18, so that the degenerate generators' centroids are EXACTLY equal where they say so)."""
    rng = np.random.default_rng(1000 * seed + a)
    pa = _blob_positions(gen, a, rng)
    pb = rng.uniform(0.0, 1.0, (b, 3))
    pb[:, 0] = 0.76 + 0.23 * pb[:, 0]
    r = (256 + (np.arange(a + b) * 7) % 1021) * STEP                      # 0.00098 .. 0.0049
    return _compile(spheres=np.column_stack([np.concatenate([pa, pb]), r]), emitter=a)


# (generator, a, b, cluster limit): every a of the list on random blobs; the degenerate generators where each kernel meets them
BLOB_B = {512: 520, 64: 70}
BLOBS = [("random", a, BLOB_B[512], 512) for a in (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513)] \
    + [("random", a, BLOB_B[64], 64) for a in (1, 2, 3, 63, 64, 65)] \
    + [(g, a, BLOB_B[512], 512) for g in ("equal", "line", "plane", "grid") for a in (65, 128, 512)] \
    + [(g, 64, BLOB_B[64], 64) for g in ("equal", "line", "plane", "grid")] \
    + [("equal", 3, BLOB_B[512], 512), ("equal", 513, BLOB_B[512], 512), ("exp", 48, BLOB_B[64], 64), ("exp", 500, BLOB_B[512], 512)]


def kernel_centroids(cs):
    """the centroids as the kernels form them from the float32 boxes: 0.5f * (lo + hi) (k_shape_boxes, k_morton_keys) and lo + hi
    (the SAH kernels), float32"""
    lo, hi = shape_box_words(cs)
    s = lo.view(np.float32) + hi.view(np.float32)
    return np.float32(0.5) * s, s


BIG_SCENES = ((0, 50), (1, 50), (256, 2), (257, 2), (300, 0), (2, 1))     # (p large spheres of radius 0.3, q tiny ones)


@functools.lru_cache(maxsize=None)
def big_scene(p, q, seed=2):
    rng = np.random.default_rng(seed + 10 * p + q)
    big = np.column_stack([rng.uniform(0.3, 0.7, (p, 3)), np.full(p, 0.3)])
    tiny = np.column_stack([rng.uniform(0.0, 1.0, (q, 3)), 1e-3 * (1.0 + rng.random(q))])
    return _compile(spheres=np.concatenate([big, tiny]), emitter=0)


def big_shape_ratio(cs, pct=2):
    """per shape: area / ((float)pct / 100 * scene area) with k_morton_keys' float32 operations (> 1: the shape is "big")"""
    lo, hi = (x.view(np.float32) for x in shape_box_words(cs))
    d = hi - lo
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    e = hi.max(axis=0) - lo.min(axis=0)
    scene = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
    frac = np.float32(pct) / np.float32(100.0)
    assert area.dtype == np.float32 and np.float32(scene).dtype == np.float32
    return area / (frac * scene)


@functools.lru_cache(maxsize=None)
def count_scene(name):
    """"2", "3", "512", ...: that many tiny spheres; "2 quads"; "sphere+quad+triangle" """
    if name == "2 quads":
        return _compile(quads=[((0.1, 0.2, 0.3), (0.5, 0, 0), (0, 0.4, 0)), ((0.2, 0.7, 0.1), (0, 0, 0.6), (0.3, 0.1, 0))], emitter=0)
    if name == "sphere+quad+triangle":
        return _compile(spheres=[(0.2, 0.3, 0.4, 0.1)], quads=[((0.5, 0.1, 0.1), (0.4, 0, 0), (0, 0.3, 0.2))],
                        vertices=[(0.1, 0.8, 0.2), (0.6, 0.9, 0.3), (0.3, 0.6, 0.9)], triangles=[(0, 1, 2)], emitter=1)
    n = int(name)
    rng = np.random.default_rng(40 + n)
    return _compile(spheres=np.column_stack([rng.uniform(0.0, 1.0, (n, 3)), 1e-3 * (1.0 + rng.random(n))]), emitter=0)


COUNT_SCENES = ("2", "3", "1024", "1025", "2 quads", "sphere+quad+triangle")


def _zero(k):
    return 0.0 if k % 2 == 0 else -0.0


@functools.lru_cache(maxsize=None)
def zero_scene(kind, n=64):
    """n shapes, the first half quads, the second half triangles, coordinates written as literals (sums with a zero of the same
    sign: exact).  Shape k has the zero +0.0 for even k and -0.0 for odd k
      "x"      as its lower x bound; y and z in general position
      "xyz"    as its lower bound on all three axes
      "upper"  as its UPPER x bound (the shape lies in x <= 0)
      "mixed"  like "x", but with BOTH zeros among a shape's own corners (every triangle, every second quad; its box: -0)"""
    quads, verts, tris = [], [], []
    for k in range(n):
        z = _zero(k)
        w, h, d = 0.25 + 0.01 * k, 0.125 + 0.005 * k, 0.0625 + 0.002 * k
        y0, z0 = (z, z) if kind == "xyz" else (0.03125 * (k % 29) + 0.001 * k, 0.015625 * (k % 31) + 0.002 * k)
        other = -z if kind == "mixed" else z                             # (-0.0 + 0.0 = +0.0: a second corner with the other zero)
        sx = -1.0 if kind == "upper" else 1.0
        if k < n // 2:
            # corners: (z, y0, z0), (sx w, y0, z0), (z, y0 + h, z0 + d), (sx w, y0 + h, z0 + d)
            quads.append(((z, y0, z0), (sx * w, z if kind == "xyz" else 0.0, z if kind == "xyz" else 0.0), (other, h, d)))
        else:
            b = len(verts)
            verts += [(z, y0, z0), (sx * w, y0, z0 + d), (other, y0 + h, z0)]
            tris.append((b, b + 1, b + 2))
    return _compile(quads=quads, vertices=verts, triangles=tris, emitter=0)


ZERO_SCENES = (("x", 64), ("xyz", 64), ("upper", 64), ("mixed", 64), ("x", 600))


# one scene per family for "the tree is usable" (one ray per shape, tests/relayout_scenes.py shape_rays), and those that render a frame
USABLE = {"blob random 512": lambda: blob_scene("random", 512, 520), "blob equal 512": lambda: blob_scene("equal", 512, 520),
          "blob exp 500": lambda: blob_scene("exp", 500, 520), "big 257+2": lambda: big_scene(257, 2), "big 1+50": lambda: big_scene(1, 50),
          "count 1025": lambda: count_scene("1025"), "sphere+quad+triangle": lambda: count_scene("sphere+quad+triangle"),
          "zeros x 64": lambda: zero_scene("x", 64)}
# the shapes a ray of their own singles out (by the oracle's linear scan, tests/test_lbvh_edges_host.py): all of them in general
# position; concentric or coincident spheres and overlapping zero-thickness quads are compared with the oracle all the same
EVERY_SHAPE = ("blob random 512", "count 1025", "sphere+quad+triangle", "big 1+50")
FRAMES = ("blob equal 512", "blob exp 500", "big 257+2")


def shape_rays(cs, delta=5e-4):
    """relayout_scenes.shape_rays with the spheres' rays started `delta` above the surface, window [delta / 4, 4 delta]: its own
    1e-3 of a tiny sphere's size is below the intersection test's epsilon"""
    import relayout_scenes
    rays = relayout_scenes.shape_rays(cs)
    ns = len(cs.spheres)
    if ns:
        c, r = cs.spheres[:, 0:3].astype(np.float64), np.abs(cs.spheres[:, 3].astype(np.float64))
        u = -rays[:ns, 3:6].astype(np.float64)
        rays[:ns, 0:3] = c + (r + delta)[:, None] * u
        rays[:ns, 6], rays[:ns, 7] = delta / 4.0, delta * 4.0
    return rays
