"""The premises of test_follow_edges_gpu.py on the reference alone, over the oracle's trace: a scene or a sweep that stops exercising
its edge fails here, without a GPU.  The live counts of the patch scenes, the counts that shrink to one, the cap between the facing
mirrors for motion, the sizes whose last tile is one live pixel, the launches of differing size, and the fabricated records: the k
and fr edges straddled, every class there."""
import numpy as np
import pytest

import follow_ref as R
import motion_follow_ref as MF
import motion_ref as M
import path_query_ref as P
import test_follow_edges_gpu as E
from test_follow_gpu import _facing_mirrors
from test_motion_follow_gpu import _mirror_scene
from test_walk_forms_gpu import _scene_seen_from_inside

U, F = np.uint32, np.float32


@pytest.mark.parametrize("live", sorted(E.PATCHES))
def test_a_patch_scene_has_exactly_so_many_live_chains(oracle, live):
    cs = E.patch_scene(live)
    trace = R.oracle_trace(cs)
    det = MF.render_motion_followed(cs, E.quads_moved(cs), E.PATCH_W, E.PATCH_H, 2, trace, detail=True)[1]
    assert E.motion_rounds(det, 2) == [live, 0] and int(det["went"].sum()) == live and int((det["length"] > 0).sum()) == live
    ids = MF.ids_of(MF.render_motion_followed(cs, E.quads_moved(cs), E.PATCH_W, E.PATCH_H, 2, trace))
    assert (ids[det["went"]] == 1).all() and (ids[~det["went"]] == 0).all()     # the mirror shows the quad behind the camera; beside it the wall
    _, rounds, rec = E.expected_aovs(cs, E.PATCH_W, E.PATCH_H, E.one_block(E.PATCH_W, E.PATCH_H), 2, trace)
    assert rounds == [live, 0] and (rec[:, 11] == 1).all()
    a, b = E.PATCHES[live]
    assert a * b == live and a < E.PATCH_W and b <= E.PATCH_H


def test_the_nested_scene_loses_chains_every_round_down_to_one(oracle):
    cs = E.nested_scene()
    trace = R.oracle_trace(cs)
    mf = E.NESTED_FOLLOW
    det = MF.render_motion_followed(cs, E.quads_moved(cs), E.NESTED_W, 1, mf, trace, detail=True)[1]
    rounds = E.expected_aovs(cs, E.NESTED_W, 1, E.one_block(E.NESTED_W, 1), mf, trace)[1]
    assert E.motion_rounds(det, mf) == rounds == [11, 5, 3, 1], (E.motion_rounds(det, mf), rounds)
    assert int(det["count"][E.NESTED_W // 2]) == mf                     # the one chain left is the middle pixel's


@pytest.mark.parametrize("mf", [1, 7, 8])
def test_every_chain_between_the_facing_mirrors_reaches_the_cap_for_motion(oracle, mf):
    cs = _facing_mirrors()
    prev = E.quads_moved(cs)
    want, det = MF.render_motion_followed(cs, prev, 64, 64, mf, R.oracle_trace(cs), detail=True)
    assert (det["count"] == mf).all() and (det["length"] == mf).all() and not det["left"].any()
    still = MF.render_motion_followed(cs, M.Prev(cs, prev.camera), 64, 64, mf, R.oracle_trace(cs))
    assert (want.view(U)[..., 0:3] != still.view(U)[..., 0:3]).any(-1).mean() > 0.9
    assert (want.view(U)[..., 3] == (1 if mf % 2 else 0)).all()         # the chain ends on the mirror behind the camera after an odd count


def test_the_sizes_of_the_motion_scans(oracle):
    """257 pixels of a mirror: all live, the last tile one pixel; the inside camera takes no continuation at the side limit and the
    wide mirror takes one at every pixel; "rich" at 257 x 256 and 513 x 257 has live pixels in the first and the last tile"""
    for cs, W, H in ((_mirror_scene(0), 257, 1), (E.wide_mirror_scene(), 1, 257), (E.wide_mirror_scene(), 16384, 1), (E.wide_mirror_scene(), 1, 16384),
                     (_mirror_scene(0), 257, 256)):
        det = MF.render_motion_followed(cs, E.quads_moved(cs), W, H, 2, R.oracle_trace(cs), detail=True)[1]
        assert det["went"].all() and W * H % 256 in (0, 1), (W, H)
    inside = _scene_seen_from_inside()
    for W, H in ((16384, 1), (1, 16384)):
        assert MF.render_motion_followed(inside, E._prev(inside), W, H, 2, R.oracle_trace(inside), detail=True)[1]["went"].sum() == 0
    cs = P.scene("rich")
    for W, H in ((257, 256), (513, 257)):
        det = MF.render_motion_followed(cs, E._prev(cs), W, H, 2, R.oracle_trace(cs), detail=True)[1]
        live = det["went"].ravel()
        tiles = -(-W * H // 256)
        per_tile = np.bincount(np.flatnonzero(live) // 256, minlength=tiles)
        assert tiles == (257 if H == 256 else 516) and live.sum() > 20000 and (per_tile == 0).any() and (per_tile > 0).sum() > 100 and (det["count"] == 2).sum() > 1000


def test_the_launches_differ_in_samples_and_live_chains(oracle):
    cs = P.scene("rich")
    blocks = E.launch_blocks()
    trace = R.oracle_trace(cs)
    rounds = E.expected_aovs(cs, 40, 40, blocks, 2, trace)[1]
    assert rounds[0] > rounds[1] > 0
    for per_launch, launches in ((9, 1), (5, 2), (2, 5)):
        per = E.launch_live(cs, blocks, trace, per_launch)
        assert len(per) == launches and sum(p[1] for p in per) == rounds[0] and min(p[1] for p in per) > 0, per
    assert per[4][0] == 64 and per[3][0] == 256 and per[4][1] < per[3][1], per


def test_the_fabricated_records_straddle_every_edge(oracle):
    f = E.fabricated()
    report = E.check_fabricated(f)
    print({str(k): v for k, v in report.items()})
    assert len(f["sweep"]) == 6 + 4 + 2                                 # a k edge per eta (two for eta 1), an fr edge on both sides of 1.5 and 1 / 1.5, the quad's two
    cs = E.record_scene()
    ns, nq, nt = len(cs.spheres), len(cs.quads), len(cs.triangles)
    ids = f["hits"][:, 0].copy().view(U)
    for edge in (0, ns - 1, ns, ns + nq - 1, ns + nq, ns + nq + nt - 1, ns + nq + nt, 0xFFFFFFFE, 0xFFFFFFFF):
        assert (ids == edge).sum() >= 8, edge
    out = (ids >= ns + nq + nt)
    assert (f["cls"][out] == R.END).all() and (f["want"][out, 6] == np.inf).all()
    # the populated record of surface_of is the oracle's where the oracle has one: rays that hit the scene
    rng = np.random.default_rng(3)
    rays = np.zeros((6000, 8), F)
    rays[:, 0:3] = np.stack([rng.uniform(-2.5, 22, 6000), rng.uniform(-6.5, 5.5, 6000), np.full(6000, 6.0)], 1)
    rays[:, 3:6] = np.array([0, 0, -1]) + rng.normal(size=(6000, 3)) * 0.05
    rays[:, 6], rays[:, 7] = R.KEPS, np.inf
    hit_ids, t, u, v, full = oracle.intersect(cs, rays, full=True)
    hit = hit_ids >= 0
    assert hit.sum() > 500 and set(hit_ids[hit].tolist()) == set(range(ns + nq + nt))
    hits = np.stack([hit_ids.view(F), t, u, v], 1)[hit]
    mine = E.surface_of(cs, rays[hit], hits)
    assert (mine[:, 0:6].view(U) == full[hit][:, 0:6].view(U)).all()
