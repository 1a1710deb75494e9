"""The tree level: what the walk relies on in the node array hj_scene_upload derives (kernels/hj_device.h,
DeviceScene::nodes), decided exactly from Renderer.scene_tree() and the uploaded skip-link array - no rays, no GPU, no oracle, no
tolerance.  This is NOT a second text of the re-layout: which nodes are dropped and where records are placed is left to the upload;
the rules below only say what must hold of whatever it chose.  Every assertion's message starts with its rule's name."""
import numpy as np

import update_scenes as U

NONE = 0xFFFFFFFF
INNER_FLAG, PAIR_FLAG, INDEX_MASK = 0x80000000, 0x40000000, 0x3FFFFFFF
HOT_NODES = 512                     # kernels/hj_device.h kHotNodes
LEAF, INNER, PAIR = 0, 1, 2         # kind of a record
AREA_MARGIN = 1e-6                  # the float32 area is five rounded operations on non-negative terms: relative error < 3.1e-7


def _tree_of(nodes):
    """per node of the uploaded pre-order skip-link array: is it a leaf, where its subtree ends, how many leaves precede it"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    n0 = len(nodes)
    leaf = nodes[:, 3] != NONE
    exits = nodes[:, 7].astype(np.int64)
    assert (exits > np.arange(n0)).all(), "uploaded tree: an exit does not move forward"
    end = np.minimum(exits, n0)
    before = np.concatenate([[0], np.cumsum(leaf)]).astype(np.int64)      # leaves in front of node i; [n0]: all of them
    return nodes, leaf, end, before


def _pair_eligible(nodes, leaf, first_tri):
    """inner nodes whose two children are the next two records, both triangle leaves"""
    n0 = len(nodes)
    ok = np.zeros(n0, bool)
    i = np.arange(max(n0 - 2, 0))
    if len(i):
        ok[i] = (~leaf[i]) & leaf[i + 1] & leaf[i + 2] & (nodes[i + 1, 7] == i + 2) & (nodes[i + 2, 7] == nodes[i, 7]) \
            & (nodes[i + 1, 3] >= first_tri) & (nodes[i + 2, 3] >= first_tri)
    return ok


def _is_end(link, num_nodes):
    return link >= num_nodes


def check_second_copy(tree, nodes, first_tri, pairs_allowed):
    """Record root2 + i is node i: its box, its shape or `inner | root2 + i + 1` or `inner | pair | index`, root2 + exit or the end
    of the walk; no link of either copy crosses root2.  Returns the pair index per node (-1: none)."""
    nodes, leaf, end, _ = _tree_of(nodes)
    rec, root2, num_nodes = tree["records"], int(tree["root2"]), int(tree["num_nodes"])
    n0 = len(nodes)
    assert len(rec) == num_nodes and num_nodes - root2 == n0 and len(tree["map"]) == n0, "second copy: its size is not the uploaded tree's"
    two = rec[root2:]
    assert (U.boxes_of(two) == U.boxes_of(nodes)).all(), "second copy: a box differs from the uploaded node's"
    w3, w7 = two[:, 3].astype(np.int64), two[:, 7].astype(np.int64)
    assert (w3[leaf] == nodes[leaf, 3]).all(), "second copy: a leaf's shape"
    marked = ~leaf & ((w3 & PAIR_FLAG) != 0)
    assert ((w3[~leaf] & INNER_FLAG) != 0).all(), "second copy: an inner node without the inner mark"
    plain = ~leaf & ~marked
    assert (w3[plain] == (INNER_FLAG | (root2 + np.nonzero(plain)[0] + 1))).all(), "second copy: an inner node's link is not root2 + i + 1"
    assert not (marked & ~_pair_eligible(nodes, leaf, first_tri)).any(), "second copy: a pair mark on a node that is not an inner node over two triangle leaves"
    assert pairs_allowed or not marked.any(), "second copy: pair marks with pair nodes switched off"
    pair = np.full(n0, -1, np.int64)
    pair[marked] = w3[marked] & INDEX_MASK
    assert len(np.unique(pair[marked])) == int(marked.sum()) and (pair[marked] < max(int(marked.sum()), 1)).all(), "second copy: pair indices are not 0 .. pairs - 1, each once"
    inside = end < n0
    assert (w7[inside] == root2 + end[inside]).all(), "second copy: an exit is not root2 + exit"
    assert _is_end(w7[~inside], num_nodes).all(), "second copy: an exit beyond the tree does not end the walk"
    # (the links of the second copy are now known to be root2 + something: none points below root2)
    one = rec[:root2]
    a, b = one[:, 3].astype(np.int64), one[:, 7].astype(np.int64)
    child = a[((a & INNER_FLAG) != 0) & ((a & PAIR_FLAG) == 0)] & INDEX_MASK
    assert ((child < root2) | _is_end(child, num_nodes)).all(), "first copy: a child link into the second copy"
    assert ((b < root2) | _is_end(b, num_nodes)).all(), "first copy: an exit link into the second copy"
    return pair


def walk(tree, nodes):
    """The all-hit walk of the first copy from `root`: word 3's index at an inner record, word 7 at a leaf or pair record, until the
    end of the walk.  Returns S (the records in order), kind per position, shapes (positions, 2; -1: none), and per record of the first
    copy its position (-1: not reached).  A pair record gives the two leaves i + 1, i + 2 of the node that `map` names it for."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    rec, root2, num_nodes, where = tree["records"], int(tree["root2"]), int(tree["num_nodes"]), tree["map"]
    node_of = np.full(root2, -1, np.int64)
    named = np.nonzero(where[:, 0] != NONE)[0]
    assert (where[named, 0] < root2).all(), "map: a record outside the first copy"
    node_of[where[named, 0]] = named
    assert len(np.unique(where[named, 0])) == len(named), "map: two nodes name one record"
    w3, w7 = rec[:root2, 3].tolist(), rec[:root2, 7].tolist()
    pos = np.full(root2, -1, np.int64)
    S, kind, shapes = [], [], []
    r = int(tree["root"])
    while not _is_end(r, num_nodes):
        assert r < root2, f"walk: record {r} is not in the first copy"
        assert pos[r] < 0, f"walk: record {r} is visited twice"
        assert len(S) < root2, "walk: it does not end within root2 steps"
        pos[r] = len(S)
        S.append(r)
        a = w3[r]
        if not a & INNER_FLAG:
            kind.append(LEAF); shapes.append((a, -1)); r = w7[r]
        elif a & PAIR_FLAG:
            i = int(node_of[r])
            assert i >= 0 and i + 2 < len(nodes), f"walk: pair record {r} is no uploaded node's"
            kind.append(PAIR); shapes.append((int(nodes[i + 1, 3]), int(nodes[i + 2, 3]))); r = w7[r]
        else:
            kind.append(INNER); shapes.append((-1, -1)); r = a & INDEX_MASK
    return np.array(S, np.int64), np.array(kind, np.int64), np.array(shapes, np.int64).reshape(-1, 2), pos


def _intervals(tree, S, pos):
    """q per position: where the record's word 7 leads in S (len(S): the end of the walk)"""
    rec, num_nodes, root2 = tree["records"], int(tree["num_nodes"]), int(tree["root2"])
    target = rec[S, 7].astype(np.int64)
    ends = _is_end(target, num_nodes)
    assert (target[~ends] < root2).all(), "skip link: an exit leaves the first copy"
    q = np.full(len(S), len(S), np.int64)
    q[~ends] = pos[target[~ends]]
    assert (q >= 0).all(), f"skip link: the exit of record {int(S[np.argmax(q < 0)])} is a record the walk never reaches"
    p = np.arange(len(S))
    assert (q > p).all(), f"skip link: the exit of record {int(S[np.argmax(q <= p)])} does not move forward"
    return q


def check_tree(tree, nodes, num_spheres, num_quads, pairs_allowed, cs=None, placed_on=None):
    """`tree` = Renderer.scene_tree(), `nodes` = the uploaded (N0, 8) skip-link array (after an update: refitted).  `cs`: the compiled
    scene, needed when the tree has guard records (their boxes are update_scenes.guard_boxes').  `placed_on`: the records whose boxes
    the upload chose the hot set by, when they are no longer the tree's own (hj_scene_update_shapes moves boxes, never records).
    Returns the counts {reachable, guards, pairs, dropped, padding}."""
    nodes, leaf, end, before = _tree_of(nodes)
    rec, where = tree["records"], tree["map"]
    root2, num_nodes, num_hot = int(tree["root2"]), int(tree["num_nodes"]), int(tree["num_hot"])
    n0 = len(nodes)
    pair = check_second_copy(tree, nodes, num_spheres + num_quads, pairs_allowed)

    # ---- the all-hit walk: the uploaded tree's leaves in pre-order, each once
    S, kind, shapes, pos = walk(tree, nodes)
    nshape = (shapes >= 0).sum(axis=1)
    tested = shapes[shapes >= 0]                                              # row-major: left before right
    leaves = nodes[leaf, 3].astype(np.int64)
    assert len(tested) == len(leaves) and (tested == leaves).all(), \
        f"order: the walk tests {len(tested)} shapes, the uploaded tree has {len(leaves)} leaves" if len(tested) != len(leaves) else \
        f"order: shape test {int(np.argmax(tested != leaves))} of the walk is not the uploaded tree's leaf in pre-order"
    tp = np.concatenate([[0], np.cumsum(nshape)]).astype(np.int64)            # shapes tested before position p

    # ---- skip links: forward, laminar, a subtree is left only through its root's exit
    q = _intervals(tree, S, pos)
    open_q = []
    for p_, q_ in enumerate(q.tolist()):
        while open_q and open_q[-1] <= p_:
            open_q.pop()
        assert not open_q or q_ <= open_q[-1], f"skip link: the exit of record {int(S[p_])} leaves the subtree it lies in (not laminar)"
        open_q.append(q_)
    named = np.nonzero(where[:, 0] != NONE)[0]
    guarded = np.nonzero(where[:, 1] != NONE)[0]
    pm = pos[where[named, 0]]
    assert (pm >= 0).all(), "map: a mapped record is not reached by the walk"
    bad = (tp[pm] != before[named]) | (tp[q[pm]] != before[end[named]])
    assert not bad.any(), f"skip link: the record of node {int(named[np.argmax(bad)])} does not span exactly the leaves under that node"
    k = kind[pm]
    assert ((k == LEAF) == leaf[named]).all() and ((k == PAIR) == (pair[named] >= 0)).all(), "map: a record's kind is not its node's"
    assert (rec[where[named, 0], 3][k == PAIR] & INDEX_MASK == pair[named][k == PAIR]).all(), "map: a pair record's index is not its second-copy record's"
    if len(guarded):
        assert (where[guarded, 1] < root2).all() and leaf[guarded].all() and (where[guarded, 0] != NONE).all(), "map: a guard without a leaf record"
        pg = pos[where[guarded, 1]]
        assert (pg >= 0).all(), "map: a guard record is not reached by the walk"
        assert (kind[pg] == INNER).all(), "map: a guard record is not an inner record"
        bad = (tp[pg] != before[guarded]) | (tp[q[pg]] != before[guarded] + 1)
        assert not bad.any(), f"skip link: the guard of node {int(guarded[np.argmax(bad)])} does not span exactly its leaf"
        assert (rec[where[guarded, 1], 7] == rec[where[guarded, 0], 7]).all(), "skip link: a guard's exit is not its leaf record's"
    claimed = np.zeros(root2, bool)
    claimed[where[named, 0]] = True
    claimed[where[guarded, 1]] = True
    assert claimed[S].all(), f"map: the walk reaches record {int(S[np.argmax(~claimed[S])])}, which no uploaded node names"
    # a node without a record is a leaf folded into its parent's pair record, or a dropped inner node
    gone = where[:, 0] == NONE
    parent = U.parents_of(nodes)
    folded = gone & leaf
    assert (pair[parent[folded]] >= 0).all() and (parent[folded] >= 0).all(), "map: a leaf without a record that is not half of a pair"
    dropped = np.nonzero(gone & ~leaf)[0]

    # ---- boxes
    f = nodes.view(np.float32)
    assert (U.boxes_of(rec[where[named, 0]]) == U.boxes_of(nodes[named])).all(), "boxes: a mapped record does not hold its node's box"
    if len(guarded):
        assert cs is not None, "boxes: guard records need the compiled scene"
        g_nodes, lo, hi, _, _ = U.expected_guards(where, cs, nodes)
        g = rec[where[g_nodes, 1]].view(np.float32)
        assert (g[:, 0:3].view(np.uint32) == lo.view(np.uint32)).all() and (g[:, 4:7].view(np.uint32) == hi.view(np.uint32)).all(), "boxes: a guard record does not hold the guard formula's box"
    if len(dropped):
        # the box around the first kept records at or beneath every node (min / max are exact; a NaN bound stays and fails below)
        first = np.where(where[:, 1] != NONE, where[:, 1], where[:, 0]).astype(np.int64)
        rf = rec.view(np.float32)
        lo, hi = np.full((n0, 3), np.inf, np.float32), np.full((n0, 3), -np.inf, np.float32)
        has = first != NONE
        lo[has], hi[has] = rf[first[has], 0:3], rf[first[has], 4:7]
        right = nodes[np.minimum(np.arange(n0) + 1, n0 - 1), 7].astype(np.int64)
        for i in dropped[::-1].tolist():                                      # reverse pre-order: children first
            lo[i] = np.minimum(lo[i + 1], lo[right[i]])
            hi[i] = np.maximum(hi[i + 1], hi[right[i]])
        bad = ~((lo[dropped] >= f[dropped, 0:3]).all(axis=1) & (hi[dropped] <= f[dropped, 4:7]).all(axis=1))
        assert not bad.any(), f"containment: node {int(dropped[np.argmax(bad)])} has no record, and a first kept record beneath it sticks out of its box"

    # ---- hot set
    reachable = len(S)
    assert num_hot == min(HOT_NODES, reachable), f"hot set: num_hot is {num_hot} with {reachable} reachable records"
    assert (pos[:num_hot] >= 0).all(), "hot set: a record below num_hot is padding"
    padding = np.nonzero(pos < 0)[0]
    b = (rec if placed_on is None else placed_on)[:root2].view(np.float32).astype(np.float64)
    d = b[:, 4:7] - b[:, 0:3]
    with np.errstate(invalid="ignore", over="ignore"):
        area = np.where((d >= 0).all(axis=1), d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0], 0.0)
    area[np.isnan(area)] = 0.0
    cold = S[S >= num_hot]
    if len(cold) and num_hot:
        assert area[cold].max() <= area[:num_hot].min() * (1.0 + AREA_MARGIN), \
            f"hot set: cold record {int(cold[np.argmax(area[cold])])} is larger than the smallest hot one"
    return {"reachable": reachable, "guards": int(len(guarded)), "pairs": int((kind == PAIR).sum()), "dropped": int(len(dropped)),
            "padding": int(len(padding))}


def canonical(tree, nodes):
    """Per position of the all-hit walk: the six box words, the kind, the shape or shapes, q - p.  What two uploads of one scene under
    the same switches must share whatever route they took; placement, padding and the hot order are what it forgets."""
    S, kind, shapes, pos = walk(tree, nodes)
    q = _intervals(tree, S, pos)
    out = np.zeros((len(S), 10), np.int64)
    out[:, 0:6] = U.boxes_of(tree["records"][S])
    out[:, 6], out[:, 7:9], out[:, 9] = kind, shapes, q - np.arange(len(S))
    return out
