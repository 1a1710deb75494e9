"""Shared by tests/test_scene_update_host.py and tests/test_scene_update_gpu.py: the guard-box formula of hj_scene_upload (leaf guards,
api/scene_upload.hip) restated in numpy float32, and small helpers around Renderer.scene_tree()."""
import numpy as np

import refit_scenes

F = np.float32
NONE = 0xFFFFFFFF


def guard_boxes(cs, root_lo, root_hi):
    """(gmin, gmax) per shape, float32: the shape's OWN bounds (spheres: centre -/+ |radius|; quads: the four corners origin + a edge1 +
    b edge2; triangles: the vertices), padded by size / 1000 + pad_abs, one float outward.  size = the largest extent (spheres: at
    least |radius|); pad_abs = max(2e-4, 4e-6 x the largest extent of the root box joined with the camera position)."""
    cam = np.array(list(cs.desc.camera.position)[0:3], F)
    a, b = np.minimum(np.asarray(root_lo, F), cam), np.maximum(np.asarray(root_hi, F), cam)
    pad_abs = max(F(2e-4), F(4e-6) * F((b - a).max()))
    lo, hi, size = [], [], []
    if len(cs.spheres):
        c, r = cs.spheres[:, 0:3].astype(F), np.abs(cs.spheres[:, 3:4].astype(F))
        lo.append(np.minimum(c - r, c + r)); hi.append(np.maximum(c - r, c + r)); size.append(r[:, 0])
    if len(cs.quads):
        o, e1, e2 = cs.quads[:, 0:3].astype(F), cs.quads[:, 4:7].astype(F), cs.quads[:, 8:11].astype(F)
        corners = np.stack([(o + F(x) * e1) + F(y) * e2 for x in (0, 1) for y in (0, 1)], axis=1)
        lo.append(corners.min(axis=1)); hi.append(corners.max(axis=1)); size.append(np.zeros(len(o), F))
    if len(cs.triangles):
        tri = cs.vertices[:, 0:3].astype(F)[cs.triangles]
        lo.append(tri.min(axis=1)); hi.append(tri.max(axis=1)); size.append(np.zeros(len(tri), F))
    lo, hi, size = np.concatenate(lo), np.concatenate(hi), np.concatenate(size)
    size = np.maximum(size, (hi - lo).max(axis=1))
    pad = (size * F(1e-3) + pad_abs).astype(F)[:, None]
    return np.nextafter(lo - pad, F(-np.inf)).astype(F), np.nextafter(hi + pad, F(np.inf)).astype(F)


def refitted(cs, topology):
    return refit_scenes.refit_numpy(topology, refit_scenes.shape_boxes(cs))


def boxes_of(records):
    """the six box words of (n, 8) uint32 records"""
    return records[:, [0, 1, 2, 4, 5, 6]]


def links_of(records):
    return records[:, [3, 7]]


def parents_of(nodes):
    """parent index per record of a pre-order skip-link tree (left child = next record, right child = the left one's exit); the root's is -1"""
    parent = np.full(len(nodes), -1, np.int64)
    inner = np.nonzero(nodes[:, 3] == NONE)[0]
    parent[inner + 1] = inner
    parent[nodes[inner + 1, 7].astype(np.int64)] = inner
    return parent


def expected_guards(where, cs, want):
    """(guarded, lo, hi, widened, parent): the uploaded nodes that have a guard, the box each guard must hold - the formula's, or,
    where the leaf's parent has no record and the padded box is not inside the parent's box, the parent's box -, which of them hold
    their parent's box, and the parents.  `want` = the uploaded (or refitted) tree, `where` = Renderer.scene_tree()["map"]."""
    guarded = np.nonzero(where[:, 1] != NONE)[0]
    f = want.view(F)
    gmin, gmax = guard_boxes(cs, f[0, 0:3], f[0, 4:7])
    shape = want[guarded, 3]
    assert (shape != NONE).all(), "a guard in front of an inner node"
    lo, hi = gmin[shape], gmax[shape]
    p = parents_of(want)[guarded]
    assert (p >= 0).all()
    plo, phi = f[p, 0:3], f[p, 4:7]
    widened = (where[p, 0] == NONE) & ~((lo >= plo).all(axis=1) & (hi <= phi).all(axis=1))
    lo, hi = np.where(widened[:, None], plo, lo), np.where(widened[:, None], phi, hi)
    return guarded, lo, hi, widened, p


def check_records(tree, cs, want):
    """Every assertion of 'Records': `tree` = Renderer.scene_tree() after an update, `want` = the numpy refit of the uploaded topology.
    A guard holds the formula's box - or, where the upload collapsed the leaf's parent and the padded box is no longer inside the
    parent's refitted box, the parent's box: the collapse rests on that containment.  Returns the numbers of mapped records, of guards,
    and of guards that hold their parent's box."""
    rec, where, root2 = tree["records"], tree["map"], tree["root2"]
    n0 = len(want)
    assert len(where) == n0 and tree["num_nodes"] - root2 == n0
    assert (boxes_of(rec[root2:root2 + n0]) == boxes_of(want)).all(), "second copy"
    mapped = np.nonzero(where[:, 0] != NONE)[0]
    assert (boxes_of(rec[where[mapped, 0]]) == boxes_of(want[mapped])).all(), "mapped records"
    if (where[:, 1] != NONE).any():
        f = want.view(F)
        guarded, lo, hi, widened, p = expected_guards(where, cs, want)
        g = rec[where[guarded, 1]].view(F)
        assert (g[:, 0:3].view(np.uint32) == lo.view(np.uint32)).all() and (g[:, 4:7].view(np.uint32) == hi.view(np.uint32)).all(), "guard records"
        # what the collapse needs: every record under a collapsed node lies inside that node's box
        kept = np.nonzero((want[:, 3] == NONE) & (where[:, 0] == NONE))[0]
        kept = kept[np.isin(kept, p)]
        for c in kept.tolist():
            mine = p == c
            assert (g[mine, 0:3] >= f[c, 0:3]).all() and (g[mine, 4:7] <= f[c, 4:7]).all(), "a guard sticks out of its collapsed parent"
        return len(mapped), len(guarded), int(widened.sum())
    return len(mapped), 0, 0



def covered_leaf_scene(shift=0.0):
    """Four quads under a hand-made tree: root -> (P -> (leaf L, S -> (floor, ceiling)), light).  At rest the small quad L lies deep
    inside S's box, so L's padded guard box lies inside P's and the upload collapses P (both children are inner records: L's guard
    and S; P has the root's area).  `shift` moves L along x; from 0.8 on it sticks out of S's box and bounds P's refitted box itself."""
    from hijiki_amd import abi, host
    s = host.Scene()
    s.set_camera((0.0, 1.0, 3.3), (0.0, 0.0, 0.0, 1.0), 40.0)
    white, green, light = s.add_diffuse((0.7, 0.7, 0.7)), s.add_diffuse((0.2, 0.7, 0.2)), s.add_emissive((15, 15, 15))
    s.add_quad((-1, 0, 1), (2, 0, 0), (0, 0, -2), white)                   # shape 0: floor
    s.add_quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), white)                   # shape 1: ceiling
    s.add_quad((-0.2 + shift, 1.0, 0.2), (0.4, 0, 0), (0, 0.1, -0.4), green)   # shape 2: L
    s.add_quad((-0.3, 1.9, -0.3), (0.6, 0, 0), (0, 0, 0.6), light)         # shape 3: the light, inside S's box as well
    cs = s.compile()
    end = max(7, abi.BVH_ROOT_EXIT)
    topo = np.zeros((7, 8), np.uint32)
    topo[:, 3] = [NONE, NONE, 2, NONE, 0, 1, 3]
    topo[:, 7] = [end, 6, 3, 6, 5, 6, end]
    cs.set_bvh(refit_scenes.refit_numpy(topo, refit_scenes.shape_boxes(cs)))
    return cs


def light_show(moved=False, triangles=600, seed=3):
    """A box of quads with an emissive quad, an emissive sphere and an emissive triangle, diffuse spheres and a triangle soup.  moved:
    the same shapes in the same order with the three lights moved AND rescaled (their areas, so the pdf and cdf the compiler gives
    their emitters, change), a few other shapes moved, and the camera 70 units away behind a narrow lens: the extent of root box and
    camera then exceeds 50 units, where the guards' absolute padding starts to grow with it."""
    from hijiki_amd import host
    rng = np.random.default_rng(seed)
    m = 1.0 if moved else 0.0
    s = host.Scene()
    if moved:
        s.set_camera((0.3, 1.2, 70.0), (-0.001, 0.002, 0.0, 0.999997), 2.1)
    else:
        s.set_camera((0.05, 0.9, 3.3), (-0.02, 0.01, 0.0, 0.9997), 38.0)
    white, red, blue = s.add_diffuse((0.7, 0.7, 0.7)), s.add_diffuse((0.6, 0.1, 0.1)), s.add_diffuse((0.1, 0.2, 0.6))
    lq, ls, lt = s.add_emissive((20, 18, 15)), s.add_emissive((9, 12, 14)), s.add_emissive((30, 12, 12))
    s.add_quad((-1.2, 0, 1.2), (2.4, 0, 0), (0, 0, -2.4), white)
    s.add_quad((-1.2, 0, -1.2), (2.4, 0, 0), (0, 2.0, 0), white)
    s.add_quad((-1.2, 0, 1.2), (0, 0, -2.4), (0, 2.0, 0), red)
    s.add_quad((1.2, 0, -1.2), (0, 0, 2.4), (0, 2.0, 0), blue)
    s.add_quad((-0.4 + 0.3 * m, 1.99 - 0.2 * m, -0.4), (0.8 - 0.35 * m, 0, 0), (0, 0, 0.8 + 0.3 * m), lq)
    s.add_sphere((0.55 - 0.2 * m, 1.45 - 0.3 * m, 0.3), 0.12 + 0.07 * m, ls)
    s.add_sphere((-0.55, 0.35 + 0.1 * m, 0.1), 0.35 - 0.05 * m, white)
    s.add_sphere((0.45 + 0.1 * m, 0.3, 0.45), 0.3, blue)
    pos = rng.uniform([-0.9, 0.05, -0.9], [0.9, 1.5, 0.9], (triangles, 1, 3)) + rng.uniform(-0.08, 0.08, (triangles, 3, 3))
    pos = pos.reshape(-1, 3).astype(np.float32)
    pos[3:] += np.float32(0.04 * m) * np.sin(7.0 * pos[3:, ::-1]).astype(np.float32)
    pos[0:3] = np.array([[-0.7, 1.6, -0.2], [-0.3, 1.6, -0.2], [-0.5, 1.6, 0.2]], np.float32) * np.float32(1.0 + 0.5 * m) + np.float32([0.2 * m, -0.9 * m, 0])
    nrm = rng.normal(size=(len(pos), 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    base = s.add_vertices(pos, nrm)
    s.add_triangle(base, base + 1, base + 2, lt)
    s.add_triangles(base + 3 + np.arange(3 * (triangles - 1)).reshape(-1, 3), white)
    cs = s.compile()
    # (the compiler selects lights uniformly; a selection by area instead, so that pdf and cdf move with the shapes as well)
    ns, nq = len(cs.spheres), len(cs.quads)
    area = []
    for sh in cs.emitters[:, 0].tolist():
        if sh < ns:
            area.append(4.0 * np.pi * float(cs.spheres[sh, 3]) ** 2)
        elif sh < ns + nq:
            q = cs.quads[sh - ns].astype(np.float64)
            area.append(float(np.linalg.norm(np.cross(q[4:7], q[8:11]))))
        else:
            a, b, c = cs.vertices[cs.triangles[sh - ns - nq], 0:3].astype(np.float64)
            area.append(0.5 * float(np.linalg.norm(np.cross(b - a, c - a))))
    pdf = (np.array(area) / sum(area)).astype(F)
    e = cs.emitters.view(F)
    e[:, 1], e[:, 2] = pdf, np.cumsum(pdf, dtype=F)
    e[-1, 2] = 1.0
    return cs
