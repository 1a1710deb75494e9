"""The build level on the GPU: hj_build_bvh_device, hj_refit_bvh_device in both kernel forms and the exchange of
hj_tune_bvh_device against tests/lbvh_edges.py - what every correct build and refit must give, decided on raw words - on the scenes
that put the kernels of kernels/hj_lbvh.h at their size and value edges (premises: tests/test_lbvh_edges_host.py).

The switches are not crossed in full.  Every scene is built under the pairs of its own family (one test per scene, a context of
its own, the pairs one after the other); a few scenes (MATRIX_SCENES) under all of them.  The pairs, and the kernel or branch each one is for:

  wave            HJ_LBVH_CLUSTER=512                      k_emit_clusters_sah_wave + k_place_clusters; the smaller side first
  wave as split   ... HJ_BVH_CHILD_ORDER=0                 the wave kernel without the exchange of the two blocks of ids
  wave 65         HJ_LBVH_CLUSTER=65                       the wave kernel on small clusters (m == 1, m == 2, ranges of 64 and 65)
  thread          HJ_LBVH_CLUSTER=64                       k_emit_clusters_sah: one thread per cluster, its 64-entry arrays and stack
  thread as split ... HJ_BVH_CHILD_ORDER=0                 the one-thread kernel without its three reversals
  one cluster     HJ_LBVH_CLUSTER=0                        K = 1, the host's top is one item; above 512 small shapes k_refit + k_emit_clusters
  leaf clusters   HJ_LBVH_CLUSTER=1                        every leaf a cluster: the whole tree is the host's, the kernel only sees m == 1
  pairs           HJ_LBVH_CLUSTER=2                        clusters of one or two leaves
  morton          HJ_LBVH_SAH=0                            k_refit + k_emit_clusters with many clusters: the Morton splits as they are
  morton 64       HJ_LBVH_SAH=0 HJ_LBVH_CLUSTER=64         the same below a taller host top
  vote            HJ_LBVH_VOTE_PATHS=2000                  the exchange pass at the end of the build, over the wave kernel's records
  thread vote     ... HJ_LBVH_CLUSTER=64                   ... over the one-thread kernel's
  top as built    HJ_LBVH_TOP_ROTATE=0                     the host's top without its rotation passes
  top rotated     HJ_LBVH_TOP_ROTATE=64                    ... with as many as the table allows (by default 8 on tops below 4096 items)
  timing          HJ_LBVH_TIMING=1                         the stage clocks' synchronisations between the kernels; times on stderr

HJ_LBVH_VOTE_PATHS is 0 wherever it is not named (its default is 60000); HJ_LBVH_BIG_PCT is 0 on the blob scenes (nothing is "big")
and the default elsewhere, with one big-shape scene also at 0."""
import numpy as np
import pytest

import lbvh_edges as E
import refit_scenes
from hijiki_amd import device, host
from oracle import hj_oracle as O
from test_gpu_parity import assert_same
from test_ray_query_gpu import assert_hits, assert_surface

pytestmark = pytest.mark.gpu

PAIRS = {
    "wave": {"HJ_LBVH_CLUSTER": "512"},
    "wave as split": {"HJ_LBVH_CLUSTER": "512", "HJ_BVH_CHILD_ORDER": "0"},
    "wave 65": {"HJ_LBVH_CLUSTER": "65"},
    "thread": {"HJ_LBVH_CLUSTER": "64"},
    "thread as split": {"HJ_LBVH_CLUSTER": "64", "HJ_BVH_CHILD_ORDER": "0"},
    "one cluster": {"HJ_LBVH_CLUSTER": "0"},
    "leaf clusters": {"HJ_LBVH_CLUSTER": "1"},
    "pairs": {"HJ_LBVH_CLUSTER": "2"},
    "morton": {"HJ_LBVH_SAH": "0"},
    "morton 64": {"HJ_LBVH_SAH": "0", "HJ_LBVH_CLUSTER": "64"},
    "vote": {"HJ_LBVH_VOTE_PATHS": "2000"},
    "thread vote": {"HJ_LBVH_VOTE_PATHS": "2000", "HJ_LBVH_CLUSTER": "64"},
    "top as built": {"HJ_LBVH_TOP_ROTATE": "0"},
    "top rotated": {"HJ_LBVH_TOP_ROTATE": "64"},
    "timing": {"HJ_LBVH_TIMING": "1"},
}
DEFAULTS = {"HJ_LBVH_CLUSTER": "512", "HJ_LBVH_SAH": "1", "HJ_LBVH_VOTE_PATHS": "0", "HJ_BVH_CHILD_ORDER": "3", "HJ_LBVH_TOP_ROTATE": "-1",
            "HJ_LBVH_TIMING": "0"}
HOME_WAVE, HOME_THREAD = ("wave", "wave as split"), ("thread", "thread as split")
HOME_SMALL = ("wave", "thread", "one cluster", "leaf clusters", "morton")


def _blob(gen, a, b, cmax):
    return ("blob", gen, a, b, cmax)


MATRIX_SCENES = [_blob("random", 65, 520, 512), _blob("equal", 512, 520, 512), _blob("exp", 500, 520, 512), _blob("line", 64, 70, 64),
                 ("big", 1, 50), ("big", 257, 2), ("count", "3"), ("count", "1025"), ("count", "2 quads"), ("count", "sphere+quad+triangle"),
                 ("zero", "x", 64), ("zero", "xyz", 64), ("zero", "x", 600)]


def _cases():
    """(scene key, the pairs it is built under)"""
    out = []
    for g, a, b, cmax in E.BLOBS:
        key = _blob(g, a, b, cmax)
        home = HOME_WAVE + (("wave 65",) if a in (1, 2, 3, 65) else ()) if cmax == 512 else HOME_THREAD
        out.append((key, tuple(PAIRS) if key in MATRIX_SCENES else home))
    for key in [("big", p, q) for p, q in E.BIG_SCENES] + [("count", n) for n in E.COUNT_SCENES] + [("zero", k, n) for k, n in E.ZERO_SCENES]:
        out.append((key, tuple(PAIRS) if key in MATRIX_SCENES else HOME_SMALL))
    out.append((("big", 1, 50, "HJ_LBVH_BIG_PCT=0"), ("wave", "thread")))
    return out


def _scene(key):
    if key[0] == "blob":
        return E.blob_scene(key[1], key[2], key[3])
    if key[0] == "big":
        return E.big_scene(key[1], key[2])
    if key[0] == "count":
        return E.count_scene(key[1])
    return E.zero_scene(key[1], key[2])


def _setenv(monkeypatch, key, pair):
    env = dict(DEFAULTS)
    env.update(PAIRS[pair])
    env["HJ_LBVH_BIG_PCT"] = "0" if key[0] == "blob" or key[-1] == "HJ_LBVH_BIG_PCT=0" else "2"
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture
def r():
    """A context of its own: no tree and no kept links of an earlier test on it."""
    with device.Renderer(0) as ctx:
        yield ctx


def _differ(a, b):
    return f"{int((a != b).any(axis=1).sum())} of {len(a)} records differ, the first at {int(np.argmax((a != b).any(axis=1)))}"


def _build_and_refit(r, monkeypatch, cs):
    """the four assertions of a combination; returns the built tree"""
    built = r.build_bvh(cs)
    E.check_built_tree(built, cs)
    again = r.build_bvh(cs)
    assert (again == built).all(), "a second build: " + _differ(again, built)
    want = E.refit_reference(built, cs)
    assert (built == want).all(), "the build against the reference refit of its own links: " + _differ(built, want)
    for tiled in ("1", "0"):
        monkeypatch.setenv("HJ_REFIT_TILED", tiled)
        got = r.refit_bvh(cs, topology=built)
        assert (got == built).all(), f"HJ_REFIT_TILED={tiled} against the build: " + _differ(got, built)
    return built


@pytest.mark.parametrize("key,pairs", _cases(), ids=[" ".join(str(x) for x in key) for key, _ in _cases()])
def test_build_and_refit(r, monkeypatch, key, pairs):
    cs = _scene(key)
    for pair in pairs:
        with monkeypatch.context() as m:
            _setenv(m, key, pair)
            try:
                built = _build_and_refit(r, m, cs)
            except AssertionError as e:
                raise AssertionError(f"[{pair}] {e}") from None
        if key[0] == "zero":
            both = E.has_both_zeros(built)
            print(f"{key} {pair}: {both} inner nodes take -0 from one child and +0 from the other")
            assert both >= 1, pair
            side = 4 if key[1] == "upper" else 0
            assert built[0, side] == (E.POS_ZERO if key[1] == "upper" else E.NEG_ZERO), pair


def test_top_rotation_takes_effect(r, monkeypatch):
    """the premise of the two HJ_LBVH_TOP_ROTATE rows: with clusters of one or two leaves the host's top is most of the tree, and
    its rotation passes move records of 520 random shapes - both trees valid, the same leaves, other links"""
    key = _blob("random", 65, 520, 512)
    cs = _scene(key)
    built = {}
    for passes in ("0", "64"):
        with monkeypatch.context() as m:
            _setenv(m, key, "pairs")
            m.setenv("HJ_LBVH_TOP_ROTATE", passes)
            built[passes] = _build_and_refit(r, m, cs)
    assert built["0"].shape == built["64"].shape and (built["0"] != built["64"]).any(), "64 rotation passes left the top as it was built"


@pytest.mark.parametrize("kind,n", E.ZERO_SCENES)
@pytest.mark.parametrize("shape", list(E.REFIT_TOPOLOGIES))
def test_refit_orders_the_zeros_on_given_topologies(r, monkeypatch, kind, n, shape):
    """-0 beside +0 among the children: both kernel forms give the reference's words, whoever arrives first"""
    cs = E.zero_scene(kind, n)
    topo = E.REFIT_TOPOLOGIES[shape](n)
    want = E.refit_reference(topo, cs)
    for tiled in ("1", "0", "1"):
        monkeypatch.setenv("HJ_REFIT_TILED", tiled)
        got = r.refit_bvh(cs, topology=topo if tiled == "1" else None)
        assert (got == want).all(), f"HJ_REFIT_TILED={tiled}: " + _differ(got, want)


def _refit_topologies():
    return [(n, s) for n in E.REFIT_SIZES for s in list(E.REFIT_TOPOLOGIES) + ["device-built"]] + [(1025, "boundary")]


@pytest.mark.parametrize("n,shape", _refit_topologies())
def test_refit_around_one_run_of_records(r, monkeypatch, n, shape):
    """N = 1023, 1025, 2047, 2049 records around kRfTile = 1024: both kernel forms equal the reference, unmoved and after one
    deformation step, and the kept-links call afterwards gives the same (the counters were left zero)."""
    cs = E.count_scene(str(n))
    for k, v in DEFAULTS.items():
        monkeypatch.setenv(k, v)
    topo = r.build_bvh(cs) if shape == "device-built" else E.boundary_topology(n) if shape == "boundary" else E.REFIT_TOPOLOGIES[shape](n)
    d = refit_scenes.Deformation(cs, seed=12)
    try:
        for step in (0, 1):
            if step:
                d.apply(0.02, t=0.3)
            want = E.refit_reference(topo, cs)
            if step:
                assert (want != unmoved).any()
            unmoved = want
            for tiled in ("1", "0"):
                monkeypatch.setenv("HJ_REFIT_TILED", tiled)
                got = r.refit_bvh(cs, topology=topo)
                assert (got == want).all(), f"step {step}, HJ_REFIT_TILED={tiled}: " + _differ(got, want)
                kept = r.refit_bvh(cs)
                assert (kept == want).all(), f"step {step}, HJ_REFIT_TILED={tiled}, kept links: " + _differ(kept, want)
            E.check_built_tree(want, cs)
    finally:
        d.restore()


TUNED = [_blob(g, a, b, cmax) for g, a, b, cmax in E.BLOBS if a in (3, 64, 65, 512, 500, 48)] + [("big", p, q) for p, q in E.BIG_SCENES]


@pytest.mark.parametrize("key", TUNED, ids=lambda v: " ".join(str(x) for x in v))
def test_vote_keeps_the_records(r, monkeypatch, key):
    """hj_tune_bvh_device with 2000 paths on a built tree: still a tree with exact boxes, the same records as a multiset"""
    cs = _scene(key)
    _setenv(monkeypatch, key, "wave" if key[0] == "big" or key[4] == 512 else "thread")
    built = r.build_bvh(cs)
    E.check_built_tree(built, cs)                                         # (no rays through a broken tree)
    cs.set_bvh(built)
    tuned = r.tune_bvh_device(cs, vote_paths=2000)
    E.check_built_tree(tuned, cs)
    assert (E.record_multiset(tuned) == E.record_multiset(built)).all()
    print(f"{key}: {int((tuned != built).any(axis=1).sum())} of {len(built)} records moved by the vote")


@pytest.mark.parametrize("name", list(E.USABLE))
def test_every_shape_is_found_through_the_built_tree(r, monkeypatch, name):
    """One ray per shape through the uploaded device-built tree against the oracle walking the same tree: ids, the bits of t, u, v and
    the surface record, the any-hit boolean (premise: tests/test_lbvh_edges_host.py)."""
    cs = E.USABLE[name]()
    for k, v in DEFAULTS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HJ_LBVH_BIG_PCT", "0" if name.startswith("blob") else "2")
    r.build_bvh(cs, keep_on_device=True)
    nodes = r.read_device_bvh()
    E.check_built_tree(nodes, cs)
    cs.set_bvh(nodes)
    r.upload_scene(cs, device_tree=True)
    rays = E.shape_rays(cs)
    want = O.intersect(cs, rays, full=True)
    got = r.trace_rays(rays, surface=True)
    own = int((want[0] == np.arange(cs.num_shapes)).sum())
    print(f"{name}: {own} of {cs.num_shapes} shapes found by their own ray, {int((want[0] < 0).sum())} misses")
    if name in E.EVERY_SHAPE:
        assert own == cs.num_shapes
    assert_hits(got, want, name)
    assert_surface(cs, got, want, name)
    ai, *_ = r.trace_rays(rays, any_hit=True)
    assert ((ai >= 0) == (want[0] >= 0)).all(), f"{name}: any-hit booleans"


@pytest.mark.parametrize("name", E.FRAMES)
def test_frame_through_the_built_tree(r, oracle, monkeypatch, name):
    cs = E.USABLE[name]()
    for k, v in DEFAULTS.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HJ_LBVH_BIG_PCT", "0" if name.startswith("blob") else "2")
    nodes = r.build_bvh(cs)
    E.check_built_tree(nodes, cs)                                         # (no rays through a broken tree)
    cs.set_bvh(nodes)
    W, H = 64, 48
    blocks = host.make_blocks(W, H, 1, 29)
    want, ctr, _ = oracle.render_blocks(cs, blocks, W, H)
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    st = r.render_blocks(blocks)
    assert_same(r.read(), want, name)
    assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"] and st["hits"] == ctr["hits"]
