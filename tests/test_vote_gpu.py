"""The device ray vote (kernels/hj_vote.h, api/tree_vote.hip) against tests/vote_ref.py, half by half ("The vote's two
halves, pinned"): the exchange on given gains and the counting on given rays and hits bit for bit, the vote's own closest hit against
a float64 brute force, the sampler by the properties its seeds give it, and the two halves joined on the product's routes."""
import numpy as np
import pytest

import lbvh_edges as E
import reinsert_scenes
import vote_ref as V
import vote_scenes as S
from hijiki_amd import abi, device, host

pytestmark = pytest.mark.gpu


def _u64(g):
    return np.array([int(x) for x in g], np.uint64)


def _same_gains(got, want, what):
    for side, g, w in zip(("gain_l", "gain_r"), got, want):
        g = [int(x) for x in g]
        bad = [k for k in range(len(w)) if g[k] != w[k]]
        assert not bad, f"{what}: {side} differs in {len(bad)} of {len(w)} records, first {bad[0]}: {g[bad[0]]} against {w[bad[0]]}"


# ---------------------------------------------------------------------------------------------------------------- the exchange
def _exchange_trees():
    for n in (1, 2, 3, 4):                                                 # N = 1, 3, 5, 7 records
        yield f"{2 * n - 1} records", n, E.balanced_topology
    for n in (64, 257, 1025):
        yield f"balanced {n}", n, E.balanced_topology
    yield "shuffled 257", 257, reinsert_scenes.shuffled_topology
    for level in (14, 15, 16, 17, 31, 32, 33):                             # the level loop reads its progress every 16 levels
        yield f"right spine, deepest inner level {level}", level + 2, S.right_spine
    yield "left spine, deepest inner level 33", 35, E.left_spine_topology


_TREES = list(_exchange_trees())


@pytest.mark.parametrize("name,n,make", _TREES, ids=[t[0] for t in _TREES])
def test_exchange_equals_the_reference(gpu_renderer, name, n, make):
    """Records, exchanged nodes and levels of hj_debug_vote_exchange against exchange_ref, word for word, for every gain set and both
    root-exit conventions; every result is a valid tree of the same records."""
    cs = E.count_scene(str(n)) if n > 1 else None
    start = E.refit_reference(make(n), cs) if cs is not None else np.array([[1, 2, 3, 0, 4, 5, 6, abi.BVH_ROOT_EXIT]], np.uint32)
    if "level" in name:
        assert S.inner_levels(start) == int(name.split()[-1]) + 1
    for convention, nodes in (("constant", start), ("N", S.root_exit_n(start))):
        for k, kind in enumerate(S.GAIN_SETS):
            gl, gr = S.gains(kind, nodes, seed=k)
            want, want_exchanged, want_levels = V.exchange_ref(nodes, gl, gr)
            got, exchanged, levels = gpu_renderer.debug_vote_exchange(nodes, _u64(gl), _u64(gr))
            what = f"{name}, root exit {convention}, gains {kind}"
            assert (got == want).all(), f"{what}: {int((got != want).sum())} words differ"
            if len(nodes) >= 3:                                            # (fewer: the copy, which counts nothing)
                assert (exchanged, levels) == (want_exchanged, want_levels), what
            else:
                assert (exchanged, levels) == (0, 0) and want_exchanged == 0
            if kind == "zero" or kind == "left 2^32":
                assert (got == nodes).all() and exchanged == 0, what
            if kind in ("ones", "right 2^32"):
                assert want_exchanged == len(nodes) // 2, what
            if cs is not None:
                E.check_built_tree(got if convention == "constant" else S.root_exit_constant(got), cs)
                assert (E.record_multiset(got) == E.record_multiset(nodes)).all(), what


def test_exchange_at_its_level_limit(gpu_renderer):
    """A spine with abi.VOTE_MAX_LEVELS inner levels is accepted and, every node exchanged, equals the reference; one level more is
    HJ_ERR_UNSUPPORTED and leaves the context usable; a broken link is HJ_ERR_INVALID."""
    n = abi.VOTE_MAX_LEVELS + 1
    cs = E.count_scene(str(n))
    nodes = E.refit_reference(S.right_spine(n), cs)
    N = len(nodes)
    assert S.inner_levels(nodes) == abi.VOTE_MAX_LEVELS
    want, want_exchanged, want_levels = V.exchange_ref(nodes, [0] * N, [1] * N)
    got, exchanged, levels = gpu_renderer.debug_vote_exchange(nodes, _u64([0] * N), _u64([1] * N))
    assert (got == want).all() and (exchanged, levels) == (want_exchanged, want_levels) == (N // 2, abi.VOTE_MAX_LEVELS)
    E.check_built_tree(got, cs)
    deeper = E.refit_reference(S.right_spine(n + 1), E.count_scene(str(n + 1)))
    with pytest.raises(abi.HijikiError) as err:
        gpu_renderer.debug_vote_exchange(deeper, _u64([0] * (N + 2)), _u64([1] * (N + 2)))
    assert err.value.status == abi.HJ_ERR_UNSUPPORTED and "deeper" in str(err.value)
    again, _, _ = gpu_renderer.debug_vote_exchange(nodes, _u64([0] * N), _u64([1] * N))
    assert (again == want).all()
    broken = nodes.copy()
    broken[N - 1, 7] += 1                                                  # (the last leaf leaves through another exit than its parent)
    with pytest.raises(abi.HijikiError) as err:
        gpu_renderer.debug_vote_exchange(broken, _u64([0] * N), _u64([1] * N))
    assert err.value.status == abi.HJ_ERR_INVALID and "not a pre-order skip-link tree" in str(err.value)


# ---------------------------------------------------------------------------------------------------------------- the counting
@pytest.fixture(scope="module", params=["cluster", "cbox"])
def cast_case(request):
    """scene, rays, the reference's hits (leaf position, t as float32) and cast_counts of them - computed once"""
    cs, rays, ref = S.case(request.param)
    hits = (S.leaf_positions(cs.bvh, ref["shape"]), ref["t"].astype(np.float32))
    return request.param, cs, rays, ref, hits, V.cast_counts(cs.bvh, rays, hits)


def test_cast_equals_the_reference(gpu_renderer, cast_case):
    """gain_l and gain_r of hj_debug_vote_cast on given hits against cast_ref, integer for integer, in every record: closest-hit
    votes, shadow votes at w_shadow 0, 1, 4, 16, and prefixes of 1, 63, 64, 65 rays."""
    name, cs, rays, ref, hits, counts = cast_case
    N = len(cs.bvh)
    gl, gr = V.gains_of(counts, N, False, 1)
    assert sum(1 for g in gl if g) > 10 and sum(1 for g in gr if g) > 10                 # votes land on both sides,
    assert sum(1 for c in counts if c[4] > 0) > 100                                      # in front of the hit (ct > 0),
    assert max(c[5] for c in counts) >= 5 and sum(1 for c in counts if c[5] >= 5 and c[3] > c[4]) > 100   # and at depth 5 or deeper
    for any_hit, w in ((False, 1), (True, 0), (True, 1), (True, 4), (True, 16)):
        want = V.gains_of(counts, N, any_hit, w)
        got_l, got_r, found = gpu_renderer.debug_vote_cast(cs, rays, any_hit=any_hit, w_shadow=w, hits=hits)
        _same_gains((got_l, got_r), want, f"{name}, any_hit {any_hit}, w_shadow {w}")
        assert (found[:, 0] == hits[0].astype(np.uint32)).all() and (found[hits[0] != V.MISS, 2] == hits[1].view(np.uint32)[hits[0] != V.MISS]).all()
        if any_hit and w == 0:
            assert not got_l.any() and not got_r.any()
        if not any_hit:
            again = gpu_renderer.debug_vote_cast(cs, rays, any_hit=False, w_shadow=1, hits=hits)
            assert all((a == b).all() for a, b in zip(again, (got_l, got_r, found)))    # a second call: the same bytes
    for n in (1, 63, 64, 65):
        part = [c for c in counts if c[0] < n]
        got_l, got_r, _ = gpu_renderer.debug_vote_cast(cs, rays[:n], hits=(hits[0][:n], hits[1][:n]))
        _same_gains((got_l, got_r), V.gains_of(part, N, False, 1), f"{name}, the first {n} rays")
    away = S.missing_rays(cs)
    got_l, got_r, found = gpu_renderer.debug_vote_cast(cs, away)           # (the vote's own closest hit: none)
    assert not got_l.any() and not got_r.any() and (found[:, 0] == V.MISS).all() and (found[:, 1] == 0xFFFFFFFF).all()


def test_cast_votes_below_level_4096(gpu_renderer):
    """A ray votes at EVERY ancestor of its leaf down to the depth the exchange accepts (cast stopped after 4096 ancestors while the
    exchange took 8192 levels): on a right spine of 5001 spheres, rays given a hit in the deepest leaves."""
    n = 5001
    cs = E.count_scene(str(n))
    nodes = E.refit_reference(S.right_spine(n), cs)
    cs = E.count_scene.__wrapped__(str(n))                                 # (a scene of its own: the shared one keeps no tree)
    cs.set_bvh(nodes)
    N = len(nodes)
    rng = np.random.default_rng(4)
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = rng.uniform(0.1, 0.9, (64, 3))
    d = rng.normal(size=(64, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6], rays[:, 7] = 1e-4, np.inf
    leaves = np.nonzero(nodes[:, 3] != V.INNER)[0]
    hits = (leaves[-64:].astype(np.int64), np.full(64, 0.5, np.float32))
    counts = V.cast_counts(nodes, rays, hits)
    assert max(c[5] for c in counts) >= 4999 and sum(1 for c in counts if c[5] >= 4096 and c[3] > c[4]) > 0
    got_l, got_r, _ = gpu_renderer.debug_vote_cast(cs, rays, hits=hits)
    _same_gains((got_l, got_r), V.gains_of(counts, N, False, 1), "spine of 5001")


# the largest |t - t64| / max(1, t64) over the unambiguous hits of each set, measured on the MI355X, and the bound: 8 x that.  The
# spheres' is the larger: c = |o - centre|^2 - r^2 is formed in float32 from terms near 1 for radii of 0.05 ... 0.12.
T_ERROR_MEASURED = {"cluster": 1.581e-05, "cbox": 4.020e-07}
T_ERROR_BOUND = {name: 8.0 * err for name, err in T_ERROR_MEASURED.items()}


def test_closest_finds_the_nearest_shape(gpu_renderer, cast_case):
    """hj::vote::closest through hj_debug_vote_cast without given hits: shape = the float64 brute force's nearest, the leaf position
    the record that holds that shape; rays closest_f64 alone calls ambiguous (vote_ref.ambiguous) are left out - at most 2 % - and
    casting with the device's hits given back gives the gains of casting without.
    t: the largest |t - t64| / max(1, t64) measured on the MI355X is 1.581e-05 on the sphere cluster (2039 hits) and 4.020e-07 on the
    Cornell box (3425 hits); the bound is 8 x the set's figure, 1.265e-04 and 3.216e-06 (T_ERROR_MEASURED, T_ERROR_BOUND)."""
    name, cs, rays, ref, hits, counts = cast_case
    got_l, got_r, found = gpu_renderer.debug_vote_cast(cs, rays)
    keep = ~V.ambiguous(ref)
    assert keep.sum() >= 0.98 * len(rays)
    shape = found[:, 1].view(np.int32).astype(np.int64)
    wrong = np.nonzero(keep & (shape != ref["shape"]))[0]
    assert len(wrong) == 0, f"{name}: {len(wrong)} rays find another shape, first {wrong[0]}: {shape[wrong[0]]} against {ref['shape'][wrong[0]]}"
    hit = keep & (ref["shape"] >= 0)
    assert (found[keep, 0].astype(np.int64) == S.leaf_positions(cs.bvh, ref["shape"])[keep]).all()
    t = found[:, 2].view(np.float32).astype(np.float64)
    err = float((np.abs(t[hit] - ref["t"][hit]) / np.maximum(1.0, ref["t"][hit])).max())
    print(f"{name}: largest |t - t64| / max(1, t64) = {err:.3e} over {int(hit.sum())} hits")
    assert err <= T_ERROR_BOUND[name], (err, T_ERROR_BOUND[name])
    pos = np.where(found[:, 0] == V.MISS, V.MISS, found[:, 0]).astype(np.int64)
    back = gpu_renderer.debug_vote_cast(cs, rays, hits=(pos, found[:, 2].view(np.float32)))
    assert (back[0] == got_l).all() and (back[1] == got_r).all() and (back[2] == found).all()
    _same_gains((got_l, got_r), V.cast_ref(cs.bvh, rays, (pos, found[:, 2].view(np.float32)), False, 1), f"{name}: the device's own hits")


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _fresh_gains(monkeypatch, cs, paths, shadow=None):
    if shadow is None:
        monkeypatch.delenv("HJ_BVH_VOTE_SHADOW", raising=False)
    else:
        monkeypatch.setenv("HJ_BVH_VOTE_SHADOW", str(shadow))
    r = device.Renderer(0)
    try:
        return [g.astype(object) for g in r.debug_vote_gains(cs, paths)]
    finally:
        r.close()


def test_sampler_properties(gpu_renderer, monkeypatch, cbox_spheres):
    """The paths draw their directions with the device's fast trigonometry: pinned by what the seeds and the weights imply.  A path's
    seed is its index (2000 paths' gains <= 4000 paths'), two runs agree, the shadow rays' votes are linear in HJ_BVH_VOTE_SHADOW and
    not all zero, absent without emitters, and no paths leave no gains."""
    cs = cbox_spheres
    assert len(cs.emitters) > 0
    g2000, g4000 = gpu_renderer.debug_vote_gains(cs, 2000), gpu_renderer.debug_vote_gains(cs, 4000)
    for a, b in zip(g2000, g4000):
        assert (a <= b).all() and (a < b).any() and a.any()
    for a, b in zip(g4000, gpu_renderer.debug_vote_gains(cs, 4000)):
        assert (a == b).all()
    assert not any(g.any() for g in gpu_renderer.debug_vote_gains(cs, 0))
    g0, g4, g8 = (_fresh_gains(monkeypatch, cs, 4000, w) for w in (0, 4, 8))
    for side in range(2):
        assert ((g8[side] - g0[side]) == 2 * (g4[side] - g0[side])).all()
        assert ((g4[side] - g0[side]) >= 0).all()
    assert (g4[0] - g0[0]).any() or (g4[1] - g0[1]).any()
    dark = S.cluster(emitters=False, shift=0.0)
    assert len(dark.emitters) == 0
    d0, d4 = (_fresh_gains(monkeypatch, dark, 4000, w) for w in (0, 4))
    assert all((a == b).all() for a, b in zip(d0, d4)) and (d0[0].any() or d0[1].any())


# ---------------------------------------------------------------------------------------------------------------- the two halves joined
def _worst_order(nodes):
    """every node's children exchanged where the right one has more records (tests/test_gpu_parity.py _order_children)"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    N = len(nodes)
    gl, gr = [0] * N, [0] * N
    for i in np.nonzero(nodes[:, 3] == V.INNER)[0].tolist():
        r = int(nodes[i + 1, 7])
        gl[i], gr[i] = r - (i + 1), min(int(nodes[i, 7]), N) - r
    return V.exchange_ref(nodes, gl, gr)[0]


@pytest.mark.parametrize("kind,tris", [(host.SYNTH_CBOX_SPHERES, 0), (host.SYNTH_CBOX_MESH, 20000)])
def test_tune_is_the_exchange_of_the_sampled_gains(gpu_renderer, monkeypatch, kind, tris):
    monkeypatch.delenv("HJ_BVH_VOTE_SHADOW", raising=False)
    P = 30000
    cs = host.Scene.synthetic(kind, mesh_triangles=tris).compile()
    worst = _worst_order(cs.bvh)
    cs.set_bvh(worst)
    gl, gr = gpu_renderer.debug_vote_gains(cs, P)
    want, exchanged, _ = V.exchange_ref(worst, gl, gr)
    assert exchanged > 0
    got = gpu_renderer.tune_bvh_device(cs, vote_paths=P)
    assert (got == want).all(), f"{int((got != want).any(axis=1).sum())} records differ"


def test_build_ends_with_the_exchange_of_the_sampled_gains(monkeypatch):
    P = 20000
    cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=20000).compile(with_tree=False)
    monkeypatch.delenv("HJ_BVH_VOTE_SHADOW", raising=False)
    built = {}
    for paths in (0, P):
        monkeypatch.setenv("HJ_LBVH_VOTE_PATHS", str(paths))
        r = device.Renderer(0)
        try:
            built[paths] = r.build_bvh(cs).copy()
            if paths == 0:
                cs.set_bvh(built[0])
                gl, gr = r.debug_vote_gains(cs, P)
        finally:
            r.close()
    want, exchanged, _ = V.exchange_ref(built[0], gl, gr)
    assert exchanged > 0
    assert (built[P] == want).all(), f"{int((built[P] != want).any(axis=1).sum())} records differ"
