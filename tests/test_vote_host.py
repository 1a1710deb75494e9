"""The vote's probes and tests/vote_ref.py, the part that needs no GPU ("The vote's two halves, pinned"): the three
entry points are declared, listed and exported, every argument refusal comes before the device and leaves a message, and the
references hold what tests/test_vote_gpu.py leans on - exchange_ref keeps a tree a tree, cast_ref counts what an independent float64
walk counts on rays in general position."""
import ctypes as C

import numpy as np
import pytest

import lbvh_edges as E
import reinsert_scenes
import vote_ref as V
import vote_scenes as S
from hijiki_amd import abi, device
from test_abi import declared_functions

NAMES = ("hj_debug_vote_cast", "hj_debug_vote_exchange", "hj_debug_vote_gains")
u64p, u32p, f32p, nodep = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(abi.BvhNode)


def test_entry_points_are_declared_listed_and_exported():
    declared = declared_functions("hijiki_hip.h")
    for name in NAMES:
        assert name in declared and name in device.EXPORTS and hasattr(device.lib(), name), name
    assert device.lib().hj_version() >= 0x001400
    header = open(S.ROOT + "/include/hijiki_hip.h").read()
    assert "#define HJ_VOTE_MAX_LEVELS 8192u" in header and "#define HJ_VOTE_MAX_RAYS 1048576u" in header
    assert (abi.VOTE_MAX_LEVELS, abi.VOTE_MAX_RAYS, abi.VOTE_MAX_SHADOW, abi.VOTE_MISS) == (8192, 1 << 20, 16, 0xFFFFFFFF)
    for wrapper in ("debug_vote_cast", "debug_vote_exchange", "debug_vote_gains"):
        assert callable(getattr(device.Renderer, wrapper))


def _refused(call, name):
    """the call is refused with HJ_ERR_INVALID and a message of its own, without a context and so without a device"""
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call() == abi.HJ_ERR_INVALID, name
    text = L.hj_last_error(None)
    assert text and text != before, (name, text)
    return text


def test_cast_refusals_come_before_the_device():
    L = device.lib()
    cs = S.cluster()
    N = len(cs.bvh)
    rays = np.zeros((4, 8), np.float32)
    rays[:, 5], rays[:, 7] = 1.0, np.inf
    gl, gr, found = np.full(N, 7, np.uint64), np.full(N, 7, np.uint64), np.full((4, 4), 7, np.uint32)
    leaf = int(np.nonzero(cs.bvh[:, 3] != V.INNER)[0][0])
    inner = int(np.nonzero(cs.bvh[:, 3] == V.INNER)[0][3])

    def given(pos):
        g = np.zeros((4, 2), np.uint32)
        g[:, 0] = leaf
        g[2, 0] = pos
        return g

    def call(scene=cs.desc, r=rays, n=4, w=1, g=None, l=gl, rr=gr, cap=N, f=found):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
        return lambda: L.hj_debug_vote_cast(None, None if scene is None else C.byref(scene), p(r, f32p), n, 0, w, p(g, u32p), p(l, u64p), p(rr, u64p), cap,
                                            p(f, u32p))
    no_tree = abi.SceneDesc()
    C.memmove(C.byref(no_tree), C.byref(cs.desc), C.sizeof(abi.SceneDesc))
    no_tree.bvh, no_tree.num_bvh_nodes = None, 0
    cases = {"null scene": call(scene=None), "null rays": call(r=None), "null gain_l": call(l=None), "null gain_r": call(rr=None),
             "null found": call(f=None), "no rays": call(n=0), "too many rays": call(n=abi.VOTE_MAX_RAYS + 1), "N above capacity": call(cap=N - 1),
             "w_shadow 17": call(w=17), "given position N": call(g=given(N)), "given position far": call(g=given(0xFFFFFFFE)),
             "given position of an inner node": call(g=given(inner)), "given the root": call(g=given(0)), "scene without a tree": call(scene=no_tree)}
    for name, c in cases.items():
        assert b"hj_debug_vote_cast" in _refused(c, name), name
    assert (gl == 7).all() and (gr == 7).all() and (found == 7).all()
    # what is valid passes every check: a miss among the given hits, w_shadow at its ends - and then finds no context
    ok = given(abi.VOTE_MISS)
    for w in (0, 16):
        rc = call(g=ok, w=w)()
        assert rc == (abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID)
        assert (b"no HIP device" if L.hj_device_count() == 0 else b"null context") in L.hj_last_error(None)


def test_exchange_refusals_come_before_the_device():
    L = device.lib()
    nodes = E.balanced_topology(4)
    N = len(nodes)
    gl, gr, out, info = np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.full((N, 8), 7, np.uint32), (C.c_uint32 * 4)()
    broken = nodes.copy()
    broken[4, 7] = 6                                                     # (the root's right child leaves through another exit than the root)

    def call(nd=nodes, n=N, l=gl, r=gr, o=out, cap=N, i=info):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
        return lambda: L.hj_debug_vote_exchange(None, p(nd, nodep), n, p(l, u64p), p(r, u64p), p(o, nodep), cap, i)
    cases = {"null nodes": call(nd=None), "null gain_l": call(l=None), "null gain_r": call(r=None), "null out": call(o=None), "null info": call(i=None),
             "no records": call(n=0), "too many records": call(n=0x7FFFFFFF), "N above capacity": call(cap=N - 1)}
    for name, c in cases.items():
        assert b"hj_debug_vote_exchange" in _refused(c, name), name
    assert b"not a pre-order skip-link tree" in _refused(call(nd=broken), "broken link")
    assert b"bvh node" in _refused(call(n=N - 2), "a prefix of a tree")
    assert (out == 7).all()
    rc = call()()
    assert rc == (abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID)


def test_gains_refusals_come_before_the_device():
    L = device.lib()
    cs = S.cluster()
    N = len(cs.bvh)
    gl, gr = np.full(N, 7, np.uint64), np.full(N, 7, np.uint64)

    def call(scene=cs.desc, l=gl, r=gr, cap=N):
        p = lambda a: None if a is None else a.ctypes.data_as(u64p)  # noqa: E731
        return lambda: L.hj_debug_vote_gains(None, None if scene is None else C.byref(scene), 100, p(l), p(r), cap)
    for name, c in {"null scene": call(scene=None), "null gain_l": call(l=None), "null gain_r": call(r=None), "N above capacity": call(cap=N - 1)}.items():
        assert b"hj_debug_vote_gains" in _refused(c, name), name
    assert (gl == 7).all() and (gr == 7).all()
    rc = call()()
    assert rc == (abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID)


# ---- exchange_ref
def _trees():
    yield "9 shapes", E.count_scene("9"), E.balanced_topology(9)
    yield "balanced 64", E.count_scene("64"), E.balanced_topology(64)
    yield "shuffled 257", E.count_scene("257"), reinsert_scenes.shuffled_topology(257)
    yield "left spine 65", E.count_scene("65"), E.left_spine_topology(65)


@pytest.mark.parametrize("name,cs,topo", list(_trees()), ids=[t[0] for t in _trees()])
def test_exchange_ref_keeps_a_tree_a_tree(name, cs, topo):
    nodes = E.refit_reference(topo, cs)
    N = len(nodes)
    zero = [0] * N
    out, exchanged, levels = V.exchange_ref(nodes, zero, zero)
    assert (out == nodes).all() and exchanged == 0 and levels == S.inner_levels(nodes)
    rng = np.random.default_rng(5)
    gl, gr = S.random_gains(rng, nodes)
    out, exchanged, levels = V.exchange_ref(nodes, gl, gr)
    inner = nodes[:, 3] == V.INNER
    assert exchanged == sum(1 for k in np.nonzero(inner)[0] if gr[k] > gl[k]) and 0 < exchanged < N // 2
    assert levels == S.inner_levels(nodes) == S.inner_levels(out)
    E.check_built_tree(out, cs)
    assert (E.record_multiset(out) == E.record_multiset(nodes)).all()
    assert not (out == nodes).all()
    # the gains moved along with their records: nothing is left to exchange
    gl2, gr2 = V.moved_gains(nodes, gl, gr)
    again, exchanged2, _ = V.exchange_ref(out, gl2, gr2)
    assert exchanged2 == 0 and (again == out).all()
    # every node exchanged: each subtree mirrored
    ones = [1] * N
    mirrored, exchanged, _ = V.exchange_ref(nodes, zero, ones)
    assert exchanged == N // 2
    E.check_built_tree(mirrored, cs)
    back, _, _ = V.exchange_ref(mirrored, zero, ones)
    assert (back == nodes).all()


def test_exchange_ref_decides_on_all_64_bits_and_keeps_ties():
    cs = E.count_scene("4")
    nodes = E.refit_reference(E.balanced_topology(4), cs)
    N = len(nodes)
    for gl, gr, want in ((1 << 32, 1, 0), (1, 1 << 32, 3), ((1 << 63) + 1, 1 << 63, 0), (1 << 63, (1 << 63) + 1, 3), (5, 5, 0), ((1 << 32) + 1, (1 << 32) + 1, 0)):
        assert V.exchange_ref(nodes, [gl] * N, [gr] * N)[1] == want, (gl, gr)
    either = nodes.copy()
    either[[0, 4, 6], 7] = N                                             # the other root-exit convention: carried as it is
    out, _, _ = V.exchange_ref(either, [0] * N, [1] * N)
    assert out[0, 7] == N and (out[:, 7] <= N).all() and sorted(out[:, 7].tolist()).count(N) == 3


# ---- cast_ref against an independent count
def _walk_f64(nodes, ray, pos, t_hit):
    """One ray's (node, side, ci, ct) list by the walk as kernels/hj_vote.h cast states it, in float64; and the smallest relative
    margin by which any of its comparisons was decided."""
    f = nodes.view(np.float32).astype(np.float64)
    shape, exits = nodes[:, 3].tolist(), nodes[:, 7].tolist()
    o, d, tmin, tmax = ray[0:3].astype(np.float64), ray[3:6].astype(np.float64), float(ray[6]), float(ray[7])
    margin = [np.inf]

    def less(a, b):
        if np.isfinite(a) and np.isfinite(b):
            margin[0] = min(margin[0], abs(a - b) / max(1.0, abs(a), abs(b)))
        return a < b

    def entry(j):
        tn, tp = (f[j, 0:3] - o) / d, (f[j, 4:7] - o) / d
        t0, t1 = np.minimum(tn, tp).max(), np.maximum(tn, tp).min()
        ok = less(t0, t1 + 1e-4)
        ok = less(t0, tmax) and ok
        ok = less(tmin, t1) and ok
        return t0 if ok else np.inf
    votes, i, end = [], 0, len(nodes)
    while i != pos:
        l = i + 1
        r = exits[l]
        b, e_ = (r, end) if pos < r else (l, r)
        ci = ct = 0
        j = b
        while j < e_:
            e = entry(j)
            if e < np.inf:
                ci += 1
                ct += 1 if less(e, t_hit) else 0
            j = j + 1 if (e < np.inf and shape[j] == V.INNER) else exits[j]
        votes.append((i, 0 if pos < r else 1, ci, ct))
        i, end = (l, r) if pos < r else (r, end)
    return votes, margin[0]


def test_cast_ref_counts_what_a_float64_walk_counts():
    """64 rays in general position through the sphere cluster's tree - picked from a fixed candidate list as the first 64 whose
    float64 walk decides every comparison by a relative margin above 1e-5, so all 64 qualify and none is skipped - give the same
    (node, side, ci, ct) from cast_counts' float32 bottom-up statement and from the float64 walk, and the same gains."""
    cs = S.cluster()
    nodes = cs.bvh.copy()
    rays, ref = S.cluster_rays(400)
    pos = S.leaf_positions(nodes, ref["shape"])
    t32 = ref["t"].astype(np.float32)
    chosen, walks = [], {}
    for k in range(len(rays)):
        if pos[k] == V.MISS:
            continue
        votes, margin = _walk_f64(nodes, rays[k], int(pos[k]), float(t32[k]))
        if margin > 1e-5:
            chosen.append(k)
            walks[k] = votes
        if len(chosen) == 64:
            break
    assert len(chosen) == 64
    sel = np.array(chosen)
    counts = V.cast_counts(nodes, rays[sel], (pos[sel], t32[sel]))
    got = {}
    for ray, node, side, ci, ct, depth in counts:
        got.setdefault(chosen[ray], []).append((node, side, ci, ct))
    assert got == walks
    assert any(ct > 0 for v in walks.values() for _, _, _, ct in v) and {s for v in walks.values() for _, s, _, _ in v} == {0, 1}
    N = len(nodes)
    for any_hit, w in ((False, 1), (True, 0), (True, 1), (True, 16)):
        gl, gr = [0] * N, [0] * N
        for v in walks.values():
            for node, side, ci, ct in v:
                (gl if side == 0 else gr)[node] += ci * w if any_hit else (ci - ct) * 4
        assert V.cast_ref(nodes, rays[sel], (pos[sel], t32[sel]), any_hit, w) == (gl, gr)
    assert V.cast_ref(nodes, rays[sel], (np.full(64, V.MISS), t32[sel]), False, 1) == ([0] * N, [0] * N)


def test_ray_sets_hold_what_the_gpu_tests_claim():
    """The two sets of tests/test_vote_gpu.py, from the references alone: 4096 rays each, axis-parallel ones without a 0 x inf
    product, finite windows, at most 2 % ambiguous by closest_f64, votes on both sides, in front of the hit, and at depth >= 5."""
    for name in ("cluster", "cbox"):
        cs, rays, ref = S.case(name)
        assert rays.shape == (4096, 8) and rays.dtype == np.float32
        d = rays[:, 3:6]
        zeros = (d == 0).sum(axis=1)
        assert (zeros == 1).sum() >= 64 and (zeros == 2).sum() >= 64 and (zeros < 3).all()
        f = cs.bvh.view(np.float32)
        for k in range(3):                                                # 0 x inf: a zero box bound or origin on an axis the ray does not move along
            on = d[:, k] == 0
            assert (rays[on, k] != 0).all()
            assert (f[:, k] > 0).all() and (f[:, 4 + k] > 0).all() and (rays[:, k] > 0).all()    # (inf - inf on such an axis, never -inf: vote_scenes.case)
        assert np.isfinite(rays[:, 7]).sum() >= 512 and np.isinf(rays[:, 7]).sum() >= 2048
        amb = V.ambiguous(ref)
        print(f"{name}: {int(amb.sum())} of 4096 rays ambiguous, {int((ref['shape'] < 0).sum())} miss")
        assert amb.sum() <= 0.02 * 4096
        assert (ref["shape"] >= 0).sum() >= 1500                          # (the cluster is open, and a short window ends before the hit)
        pos = S.leaf_positions(cs.bvh, ref["shape"])
        counts = V.cast_counts(cs.bvh, rays[:512], (pos[:512], ref["t"][:512].astype(np.float32)))
        assert {c[2] for c in counts} == {0, 1} and any(c[4] > 0 for c in counts) and max(c[5] for c in counts) >= 5
