"""The tree level without a GPU: tests/relayout_check.py must be able to fail - a records dict made by hand from the second-copy
formula passes, every mutant of it is rejected by the rule it breaks -, and the premise of the per-shape rays of
tests/test_relayout_gpu.py, from the oracle alone."""
import numpy as np
import pytest

import relayout_check as RC
import relayout_scenes as RS
import update_scenes as U
from hijiki_amd import host
from oracle import hj_oracle as O

END = 0x3FFFFFFF                   # kernels/hj_device.h kEndOfWalk


def handmade(nodes, dropped=()):
    """Renderer.scene_tree()'s dict for `nodes`, from the formula of the second copy alone: every node but `dropped` keeps a record
    with its own box, the first min(512, records) by area (ties: array order) go first, the others follow in pre-order; no guards, no
    pairs; a link to a node without a record goes to the next record behind it."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    n0 = len(nodes)
    kept = np.ones(n0, bool)
    kept[list(dropped)] = False
    order = np.nonzero(kept)[0]
    f = nodes.view(np.float32)
    d = f[:, 4:7] - f[:, 0:3]
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    hot = min(RC.HOT_NODES, len(order))
    by_area = order[np.argsort(-area[order], kind="stable")]
    is_hot = np.zeros(n0, bool)
    is_hot[by_area[:hot]] = True
    place = np.full(n0 + 1, END, np.int64)                                   # [n0]: behind the tree
    place[by_area[:hot]] = np.arange(hot)
    cold = order[~is_hot[order]]
    place[cold] = hot + np.arange(len(cold))
    m = len(order)
    nxt = np.full(n0 + 1, n0, np.int64)                                      # first kept node at or behind i
    for i in range(n0 - 1, -1, -1):
        nxt[i] = i if kept[i] else nxt[i + 1]
    rec = np.zeros((m + n0, 8), np.uint32)
    leaf = nodes[:, 3] != RC.NONE
    ex = np.minimum(nodes[:, 7].astype(np.int64), n0)
    for i in order.tolist():
        r = rec[place[i]]
        r[[0, 1, 2, 4, 5, 6]] = nodes[i, [0, 1, 2, 4, 5, 6]]
        r[3] = nodes[i, 3] if leaf[i] else RC.INNER_FLAG | int(place[nxt[i + 1]])
        r[7] = place[nxt[ex[i]]]
    two = rec[m:]
    two[:, [0, 1, 2, 4, 5, 6]] = nodes[:, [0, 1, 2, 4, 5, 6]]
    two[:, 3] = np.where(leaf, nodes[:, 3], RC.INNER_FLAG | (m + np.arange(n0) + 1))
    two[:, 7] = np.where(ex < n0, m + ex, END)
    where = np.full((n0, 2), RC.NONE, np.uint32)
    where[order, 0] = place[order]
    return {"records": rec, "map": where, "num_nodes": m + n0, "root": int(place[nxt[0]]), "root2": m, "num_hot": hot}


@pytest.fixture(scope="module")
def small(cbox_small):
    nodes = cbox_small.bvh.copy()
    nodes.setflags(write=False)
    ns, nq = len(cbox_small.spheres), len(cbox_small.quads)
    return nodes, ns, nq


def _check(tree, nodes, small):
    return RC.check_tree(tree, nodes, small[1], small[2], False)


def _copy(tree):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tree.items()}


def _inner_with_inner_children(nodes):
    """an inner node, not the root, whose two children are inner nodes"""
    for i in range(1, len(nodes) - 1):
        if nodes[i, 3] == RC.NONE and nodes[i + 1, 3] == RC.NONE and nodes[int(nodes[i + 1, 7]), 3] == RC.NONE:
            return i
    raise AssertionError("no such node")


def test_the_handmade_tree_passes(small):
    nodes = small[0]
    tree = handmade(nodes)
    counts = _check(tree, nodes, small)
    assert len(nodes) > RC.HOT_NODES, "the tree is too small to have cold records"
    assert counts == {"reachable": len(nodes), "guards": 0, "pairs": 0, "dropped": 0, "padding": 0}
    assert tree["root"] == 0
    # a dropped node whose children lie inside it is fine, and counted
    i = _inner_with_inner_children(nodes)
    counts = _check(handmade(nodes, dropped=[i]), nodes, small)
    assert counts["dropped"] == 1 and counts["reachable"] == len(nodes) - 1
    c = RC.canonical(tree, nodes)
    assert c.shape == (len(nodes), 10) and (RC.canonical(handmade(nodes), nodes) == c).all()
    assert len(RC.canonical(handmade(nodes, dropped=[i]), nodes)) == len(nodes) - 1


def _mutant_inner_exit_moved_on(nodes, tree):
    S, kind, _, pos = RC.walk(tree, nodes)
    for p in range(1, len(S)):                                               # an inner record whose exit is not the end of the walk
        t = int(tree["records"][S[p], 7])
        if kind[p] == RC.INNER and t < tree["root2"] and pos[t] + 1 < len(S):
            tree["records"][S[p], 7] = S[pos[t] + 1]
            return
    raise AssertionError("no such record")


def _mutant_leaf_exit_moved_on(nodes, tree):
    S, kind, _, pos = RC.walk(tree, nodes)
    p = int(np.nonzero(kind == RC.LEAF)[0][3])
    tree["records"][S[p], 7] = S[p + 2]                                      # (a leaf's exit is the next position of the walk)


def _mutant_exit_backwards(nodes, tree):
    S, kind, _, _ = RC.walk(tree, nodes)
    p = int(np.nonzero(kind == RC.INNER)[0][5])
    tree["records"][S[p], 7] = S[p - 1]


def _mutant_neighbours_shape(nodes, tree):
    S, kind, _, _ = RC.walk(tree, nodes)
    a, b = (int(x) for x in np.nonzero(kind == RC.LEAF)[0][7:9])
    tree["records"][S[a], 3] = tree["records"][S[b], 3]


def _mutant_siblings_exchanged(nodes, tree):
    """node i's children l, r in the other order: still a tree with forward links over the same leaves"""
    rec, where = tree["records"], tree["map"]
    i = _inner_with_inner_children(nodes)
    l, r = i + 1, int(nodes[i + 1, 7])
    end = min(int(nodes[i, 7]), len(nodes))
    out = int(rec[where[i, 0], 7])
    rec[where[i, 0], 3] = RC.INNER_FLAG | int(where[r, 0])
    for k in range(r, end):                                                  # what left the right subtree now enters the left one
        if rec[where[k, 0], 7] == out:
            rec[where[k, 0], 7] = where[l, 0]
    for k in range(l, r):
        if rec[where[k, 0], 7] == where[r, 0]:
            rec[where[k, 0], 7] = out


def _mutant_box_one_ulp(nodes, tree):
    r = tree["records"][tree["map"][11, 0]]
    r[4] = np.nextafter(r[4:5].view(np.float32), np.float32(-np.inf)).view(np.uint32)[0]


def _mutant_link_into_second_copy(nodes, tree):
    S, kind, _, _ = RC.walk(tree, nodes)
    p = int(np.nonzero(kind == RC.INNER)[0][5])
    tree["records"][S[p], 7] = tree["root2"] + int(nodes[int(np.nonzero(tree["map"][:, 0] == S[p])[0][0]), 7])


def _mutant_num_hot(nodes, tree):
    tree["num_hot"] += 1


MUTANTS = {
    "an inner record's exit moved one record on": (_mutant_inner_exit_moved_on, "skip link"),
    "a leaf's exit moved one record on": (_mutant_leaf_exit_moved_on, "order"),
    "an exit pointing backwards": (_mutant_exit_backwards, "skip link: .*forward"),
    "a leaf's shape replaced by its neighbour's": (_mutant_neighbours_shape, "order"),
    "two sibling subtrees exchanged": (_mutant_siblings_exchanged, "order"),
    "a mapped record's max.x one ulp down": (_mutant_box_one_ulp, "boxes: a mapped record"),
    "a first-copy link into the second copy": (_mutant_link_into_second_copy, "first copy: an exit link"),
    "num_hot one too large": (_mutant_num_hot, "hot set: num_hot"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_is_rejected_by_its_rule(small, name):
    nodes = small[0]
    mutate, rule = MUTANTS[name]
    tree = handmade(nodes)
    before = _copy(tree)
    mutate(nodes, tree)
    assert tree["num_hot"] != before["num_hot"] or (tree["records"] != before["records"]).any(), "the mutant changed nothing"
    with pytest.raises(AssertionError, match=rule):
        _check(tree, nodes, small)


def test_a_dropped_node_whose_child_sticks_out_is_rejected(small):
    nodes = small[0].copy()
    i = _inner_with_inner_children(nodes)
    _check(handmade(nodes, dropped=[i]), nodes, small)                       # fine while the children lie inside
    f = nodes.view(np.float32)
    c = 0.5 * (f[i, 0:3] + f[i, 4:7])
    f[i, 0:3], f[i, 4:7] = c + (f[i, 0:3] - c) * 0.8, c + (f[i, 4:7] - c) * 0.8
    _check(handmade(nodes), nodes, small)                                    # the shrunk node kept: fine
    with pytest.raises(AssertionError, match="containment"):
        _check(handmade(nodes, dropped=[i]), nodes, small)


def test_a_cold_record_larger_than_a_hot_one_is_rejected(small):
    nodes = small[0]
    tree = handmade(nodes)
    rec, where = tree["records"], tree["map"]
    a, b = tree["num_hot"] - 1, tree["num_hot"]                              # the smallest hot record and the largest cold one change places
    assert (U.boxes_of(rec[a:a + 1]) != U.boxes_of(rec[b:b + 1])).any()
    rec[[a, b]] = rec[[b, a]]
    for col, mask in ((3, (rec[:, 3] & RC.INNER_FLAG) != 0), (7, np.ones(len(rec), bool))):
        link = rec[:, col] & RC.INDEX_MASK
        flags = rec[:, col] & ~np.uint32(RC.INDEX_MASK) if col == 3 else np.uint32(0)
        first = np.arange(len(rec)) < tree["root2"]
        rec[:, col] = np.where(mask & first & (link == a), flags | b, np.where(mask & first & (link == b), flags | a, rec[:, col]))
    ia, ib = int(np.nonzero(where[:, 0] == a)[0][0]), int(np.nonzero(where[:, 0] == b)[0][0])
    where[ia, 0], where[ib, 0] = b, a
    with pytest.raises(AssertionError, match="hot set: cold record"):
        _check(tree, nodes, small)


@pytest.mark.parametrize("name", list(RS.BUILDERS))
def test_premise_of_the_per_shape_rays(name):
    """By the oracle alone: the ray made for a shape finds that shape - on every shape of the synthetic scenes, on 99 % of the shapes
    of the others (relayout_scenes.EVERY_SHAPE, PREMISE_BY_SCAN, NO_PREMISE say which is which, and why)."""
    cs = RS.scene(name)
    rays = RS.shape_rays(cs)
    assert rays.shape == (cs.num_shapes, 8) and np.isfinite(rays).all()
    ids = O.intersect(cs, rays, use_bvh=name not in RS.PREMISE_BY_SCAN)[0]
    own = int((ids == np.arange(len(rays))).sum())
    print(f"{name}: {own} of {len(rays)} shapes found by their own ray, {int((ids < 0).sum())} rays find nothing")
    if name in RS.NO_PREMISE:
        return
    if name in RS.EVERY_SHAPE:
        assert own == len(rays)
    else:
        assert own >= 0.99 * len(rays)
