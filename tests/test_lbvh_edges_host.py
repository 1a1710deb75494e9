"""The premises of tests/test_lbvh_edges_gpu.py, proved from numpy alone ("Build level"): the scenes of
tests/lbvh_edges.py hold what they claim - cluster sizes, degenerate centroids as the kernels form them, the count of large shapes,
both zeros on one coordinate, inner nodes on run boundaries - and the checker can fail."""
import numpy as np
import pytest

import lbvh_edges as E
import refit_scenes
from hijiki_amd import abi

K_CLUSTER_MAX, K_WAVE_CLUSTER_MAX, K_RF_TILE = 64, 512, 1024          # kernels/hj_lbvh.h


@pytest.mark.parametrize("gen,a,b,cmax", E.BLOBS)
def test_blob_scenes_force_their_cluster_size(gen, a, b, cmax):
    """The key's top bit is the top bit of x's cell, u = (c - min) / (max - min) < 0.5 or not: blob A is the root's left subtree, a
    cluster exactly when a <= cmax < a + b."""
    cs = E.blob_scene(gen, a, b)
    assert len(cs.spheres) == a + b and len(cs.quads) == 0 and len(cs.triangles) == 0
    c, s = E.kernel_centroids(cs)
    assert c.dtype == np.float32 and s.dtype == np.float32
    x = c[:, 0]
    assert (x[:a] < 0.25).all() and (x[a:] > 0.75).all()
    u = (x - x.min()) / (x.max() - x.min())
    assert (u[:a] < 0.4).all() and (u[a:] > 0.6).all()
    assert a <= cmax < a + b or (a, cmax) in ((513, 512), (65, 64))       # (one more than the limit: A is split further)
    assert cmax in (K_CLUSTER_MAX, K_WAVE_CLUSTER_MAX)
    assert (E.big_shape_ratio(cs, pct=2) < 0.5).all()                     # nothing is "big" at the default either
    lo, hi = E.shape_box_words(cs)
    boxes = np.concatenate([lo[:a], hi[:a]], axis=1)
    for name, arr in (("0.5f * (lo + hi)", c[:a]), ("lo + hi", s[:a])):
        same = [len(np.unique(arr[:, k])) == 1 for k in range(3)]
        if gen == "equal":
            assert same == [True, True, True], name
            assert len(np.unique(boxes, axis=0)) == a                     # ... and the boxes all differ
        elif gen == "line":
            assert same == [False, True, True] or a == 1, name
        elif gen == "plane":
            assert same == [False, False, True] or a == 1, name
        elif gen == "exp":
            coincide = int((arr == arr[-1]).all(axis=1).sum())
            assert coincide >= a - 34 and coincide >= 10, (name, coincide)  # from k = 32 or so on: c - r == -r in float32
            assert len(np.unique(arr[:, 0])) >= 12                        # ... and the first ones do not
        elif a >= 3:
            assert same == [False, False, False], name


def test_blob_scenes_cover_every_targeted_size():
    wave = {a for g, a, b, cmax in E.BLOBS if cmax == 512 and g == "random"}
    thread = {a for g, a, b, cmax in E.BLOBS if cmax == 64 and g == "random"}
    assert wave == {1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513} and thread >= {1, 2, 3, 63, 64, 65}
    for g in ("equal", "line", "plane", "grid"):
        assert {(a, cmax) for gg, a, b, cmax in E.BLOBS if gg == g} >= {(64, 64), (65, 512), (128, 512), (512, 512)}
    assert {(a, cmax) for g, a, b, cmax in E.BLOBS if g == "exp"} == {(48, 64), (500, 512)}
    assert max(a + b for g, a, b, cmax in E.BLOBS) <= 1100


@pytest.mark.parametrize("p,q", E.BIG_SCENES)
def test_big_shape_scenes_hold_their_count(p, q):
    cs = E.big_scene(p, q)
    ratio = E.big_shape_ratio(cs)
    assert ratio.dtype == np.float32 and len(ratio) == p + q
    assert (ratio[:p] > 2.0).all() and (ratio[p:] < 0.5).all()             # a factor 2 from the threshold, on either side
    assert int((ratio > 1.0).sum()) == p
    n = p + q                                                             # api/lbvh_build.hip: the first attempt is kept when ...
    kept = p == 0 or (p <= 256 and n - p >= 2)
    assert kept == ((p, q) in ((0, 50), (1, 50), (256, 2)))
    assert {pp for pp, _ in E.BIG_SCENES} >= {0, 1, 256, 257} and (2, 1) in E.BIG_SCENES


@pytest.mark.parametrize("name", E.COUNT_SCENES + tuple(str(n) for n in E.REFIT_SIZES))
def test_count_scenes(name):
    cs = E.count_scene(name)
    want = {"2 quads": (0, 2, 0), "sphere+quad+triangle": (1, 1, 1)}.get(name) or (int(name), 0, 0)
    assert (len(cs.spheres), len(cs.quads), len(cs.triangles)) == want
    assert len(cs.emitters) == 1
    if name in ("1024", "1025"):                                         # idx_bits steps between them
        bits = lambda n: max(1, int(np.ceil(np.log2(n))))
        assert bits(1024) == 10 and bits(1025) == 11


@pytest.mark.parametrize("kind,n", E.ZERO_SCENES)
def test_signed_zero_scenes_hold_both_zeros(kind, n):
    cs = E.zero_scene(kind, n)
    assert len(cs.quads) == n // 2 and len(cs.triangles) == n - n // 2
    lo, hi = E.shape_box_words(cs)
    side, axes = (hi, (0,)) if kind == "upper" else (lo, (0, 1, 2) if kind == "xyz" else (0,))
    k = np.arange(n)
    for ax in axes:
        w = side[:, ax]
        if kind == "mixed":
            both = (k >= n // 2) | (k % 2 == 1)                          # every triangle, every second quad: the ordered minimum
            assert (w[both] == E.NEG_ZERO).all() and (w[~both] == E.POS_ZERO).all()
        else:
            assert (w[k % 2 == 0] == E.POS_ZERO).all() and (w[k % 2 == 1] == E.NEG_ZERO).all()
    if kind == "mixed":
        tri = cs.vertices[:, 0][cs.triangles].view(np.uint32)
        assert ((tri == E.NEG_ZERO).any(axis=1) & (tri == E.POS_ZERO).any(axis=1)).all()
        return
    # among the shapes of one parent: in the balanced tree over the shapes in order every lowest inner node has one of each; whatever
    # the topology, the root spans both, and the reference gives it -0 for a minimum, +0 for a maximum
    for topo in (E.balanced_topology(n), refit_scenes.chain_topology(n), E.left_spine_topology(n)):
        ref = E.refit_reference(topo, cs)
        assert E.has_both_zeros(ref) >= 1
        E.check_built_tree(ref, cs)
        for ax in axes:
            assert ref[0, ax + (4 if kind == "upper" else 0)] == (E.POS_ZERO if kind == "upper" else E.NEG_ZERO)
    assert E.has_both_zeros(E.refit_reference(E.balanced_topology(n), cs)) >= n // 2 - 1
    if n == 600:
        topo = E.balanced_topology(n)
        assert len(topo) > K_RF_TILE
        inner = np.nonzero(topo[:, 3] == E.INNER)[0]
        assert ((inner + 1 < K_RF_TILE) & (topo[inner + 1, 7] >= K_RF_TILE)).any()     # two siblings in different refit runs


def test_sphere_boxes_never_hold_a_negative_zero():
    """c - r and c + r with c = +-r: x - x is +0 in round-to-nearest, never -0"""
    rng = np.random.default_rng(3)
    r = rng.uniform(1e-3, 1.0, 1000).astype(np.float32)
    for c in (r, -r):
        lo, hi = (c - r).view(np.uint32), (c + r).view(np.uint32)
        assert not (lo == E.NEG_ZERO).any() and not (hi == E.NEG_ZERO).any()
        assert ((lo == E.POS_ZERO) | (hi == E.POS_ZERO)).all()


@pytest.mark.parametrize("n", E.REFIT_SIZES)
def test_refit_topologies_are_valid_and_sit_on_run_boundaries(n):
    cs = E.count_scene(str(n))
    N = 2 * n - 1
    assert N in (1023, 1025, 2047, 2049)
    for name, make in E.REFIT_TOPOLOGIES.items():
        topo = make(n)
        ref = E.refit_reference(topo, cs)
        E.check_built_tree(ref, cs)
        assert (ref[:, 3] == topo[:, 3]).all() and (ref[:, 7] == topo[:, 7]).all()
        # without a -0 the ordered reference and refit_numpy agree
        assert not (ref[:, list(E.BOX)] == E.NEG_ZERO).any()
        assert (ref == refit_scenes.refit_numpy(topo, refit_scenes.shape_boxes(cs))).all(), name
    assert (E.topology(n, lambda m, d: 1) == refit_scenes.chain_topology(n)).all()


def test_run_boundary_cases_occur():
    inner_at_last_slot, subtree_ends_on_boundary = [], []
    for n in E.REFIT_SIZES:
        for name, make in list(E.REFIT_TOPOLOGIES.items()) + ([("boundary", E.boundary_topology)] if n == 1025 else []):
            topo = make(n)
            N = len(topo)
            if N > K_RF_TILE and topo[K_RF_TILE - 1, 3] == E.INNER:       # k_rf_tiled: l = j + 1 >= cnt
                inner_at_last_slot.append((name, n))
            inner = np.nonzero(topo[:-1, 3] == E.INNER)[0]
            left_exit = topo[inner + 1, 7]
            if (left_exit == K_RF_TILE).any():                             # a left subtree that ends exactly where the run does
                subtree_ends_on_boundary.append((name, n))
    print("inner node at record 1023:", inner_at_last_slot, "\nsubtree ending at 1024:", subtree_ends_on_boundary)
    assert ("left spine", 1025) in inner_at_last_slot
    assert ("balanced", 1024) in subtree_ends_on_boundary and ("boundary", 1025) in subtree_ends_on_boundary
    b = E.boundary_topology()
    assert b[0, 3] == E.INNER and int(b[1, 7]) == 1024 and len(b) == 2049
    E.check_built_tree(E.refit_reference(b, E.count_scene("1025")), E.count_scene("1025"))


# ---- the checker must be able to fail
def _seven_records():
    """four shapes of the "x" zero scene under a balanced tree: 0 [1 [2 3] 4 [5 6]]"""
    cs = E.zero_scene("x", 4)
    nodes = E.refit_reference(E.balanced_topology(4), cs)
    assert len(nodes) == 7 and nodes[:, 3].tolist() == [E.INNER, E.INNER, 0, 1, E.INNER, 2, 3]
    assert nodes[:, 7].tolist() == [abi.BVH_ROOT_EXIT, 4, 3, 4, abi.BVH_ROOT_EXIT, 6, abi.BVH_ROOT_EXIT]
    return cs, nodes


def test_hand_built_tree_passes():
    cs, nodes = _seven_records()
    E.check_built_tree(nodes, cs)
    assert nodes[1, 0] == E.NEG_ZERO and nodes[2, 0] == E.POS_ZERO and nodes[3, 0] == E.NEG_ZERO


def _ulp_out(nodes):
    nodes[4, 4] += 1


def _plus_zero(nodes):
    assert nodes[1, 0] == E.NEG_ZERO
    nodes[1, 0] = E.POS_ZERO


def _shapes_exchanged(nodes):
    nodes[2, 3], nodes[5, 3] = nodes[5, 3], nodes[2, 3]


def _exit_one_on(nodes):
    nodes[2, 7] += 1


def _shape_twice(nodes):
    nodes[6, 3] = nodes[5, 3]
    nodes[6, list(E.BOX)] = nodes[5, list(E.BOX)]


@pytest.mark.parametrize("mutate,rule", [(_ulp_out, "inner box"), (_plus_zero, "inner box"), (_shapes_exchanged, "leaf box"),
                                         (_exit_one_on, "structure"), (_shape_twice, "structure")])
def test_checker_rejects_each_mutant(mutate, rule):
    cs, nodes = _seven_records()
    mutate(nodes)
    with pytest.raises(AssertionError, match=rule):
        E.check_built_tree(nodes, cs)


@pytest.mark.parametrize("name", list(E.USABLE))
def test_premise_of_the_per_shape_rays(name):
    """By the oracle alone, walking the reference's boxes on a balanced tree over the shapes in order (the built tree exists on the
    device only; the linear scan gives up above 100 spheres): the ray made for a shape finds that shape."""
    from oracle import hj_oracle as O
    cs = E.USABLE[name]()
    rays = E.shape_rays(cs)
    assert rays.shape == (cs.num_shapes, 8) and np.isfinite(rays).all()
    cs.set_bvh(E.refit_reference(E.balanced_topology(cs.num_shapes), cs))
    ids = O.intersect(cs, rays)[0]
    own = int((ids == np.arange(len(rays))).sum())
    print(f"{name}: {own} of {len(rays)} shapes found by their own ray, {int((ids < 0).sum())} rays find nothing")
    if name in E.EVERY_SHAPE:
        assert own == len(rays)
