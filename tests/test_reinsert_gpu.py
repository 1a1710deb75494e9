"""hj_optimize_bvh_device on the GPU ("Reinsertion on the device"): topologies are installed through the refit, so that
bad trees can be made on purpose; what comes back is decided exactly by tests/lbvh_edges.py check_built_tree."""
import numpy as np
import pytest

from hijiki_amd import abi, device, host

import lbvh_edges as E
import reinsert_scenes as R

pytestmark = pytest.mark.gpu


def _optimise(r, cs, topo, passes=R.PASSES, compiled=None):
    """install `topo` over the shapes of cs, optimise; -> (input records, result dict with the records)"""
    start = r.refit_bvh(cs, topology=topo, keep_on_device=False)
    res = r.optimize_bvh_device(compiled, passes=passes, keep_on_device=False)
    assert (res["nodes"] == r.read_device_bvh()).all()
    return start, res


def _check(cs, start, res):
    out = res["nodes"]
    E.check_built_tree(out, cs)
    leaf_in, leaf_out = start[start[:, 3] != E.INNER], out[out[:, 3] != E.INNER]
    assert (E.record_multiset(leaf_in) == E.record_multiset(leaf_out)).all()          # every leaf record, box bits included
    assert res["cost_after"] <= res["cost_before"], (res["cost_before"], res["cost_after"])
    if res["moves"] == 0:
        assert (out == start).all() and res["cost_after"] == res["cost_before"]


@pytest.mark.parametrize("topology", sorted(R.TOPOLOGIES))
@pytest.mark.parametrize("size", R.SIZES)
def test_valid_at_the_size_edges(gpu_renderer, size, topology):
    cs = E.count_scene(size)
    start, res = _optimise(gpu_renderer, cs, R.TOPOLOGIES[topology](cs.num_shapes))
    print(size, topology, {k: v for k, v in res.items() if k != "nodes"})
    _check(cs, start, res)
    if len(start) < 7:
        assert res["moves"] == 0 and (res["nodes"] == start).all()


def test_it_optimises(gpu_renderer):
    """From the shuffled balanced tree over 1025 small spheres, 8 device passes recover at least 0.7 of what the host's 8 passes
    recover from the same start: c0 - c_dev >= 0.7 * (c0 - c_host).  MEASURED on the MI355X: c0 336.7640, c_host 19.8712, c_dev
    81.9679 after 619 moves, share 0.8040 ("Reinsertion on the device"); the floor is 0.1 below that - the result is
    deterministic, the margin is for later tie-break changes on the host side - and never below 0.5."""
    cs, start, c0, c_host = R.shuffled_case()
    got, res = _optimise(gpu_renderer, cs, R.shuffled_topology(1025))
    assert (got == start).all()
    _check(cs, start, res)
    c_dev = res["cost_after"]
    share = (c0 - c_dev) / (c0 - c_host)
    print(f"c0 {c0:.4f} (device {res['cost_before']:.4f}), c_dev {c_dev:.4f}, c_host {c_host:.4f}, moves {res['moves']}, share {share:.4f}")
    assert abs(res["cost_before"] - c0) <= 1e-9 * c0
    ref = R.restatement(start, R.PASSES)                                     # the same steps on the host: the same tree, bit for bit
    assert res["moves"] == ref["moves"] and (res["nodes"] == ref["nodes"]).all()
    assert c0 - c_dev >= 0.7 * (c0 - c_host), share


def test_fixed_point_and_determinism():
    """Three fresh runs give identical bytes; the call's own output fed back reaches a call without a move within 64 passes, and
    that call returns its input bit for bit (tests/test_reinsert_host.py runs the same start through the host restatement)."""
    cs = E.count_scene("257")
    topo = R.shuffled_topology(257)                                         # (a start with a pass that the whole-path rule repeats)
    runs = []
    for _ in range(3):                                                      # fresh runs: install, then optimise
        with device.Renderer(0) as r:
            runs.append(_optimise(r, cs, topo)[1])
    assert all((x["nodes"] == runs[0]["nodes"]).all() and x["moves"] == runs[0]["moves"] and x["cost_after"] == runs[0]["cost_after"] for x in runs)
    assert runs[0]["moves"] > 0
    with device.Renderer(0) as r:                                           # 64 passes in one call: the host restatement's tree, bit for bit
        start, one = _optimise(r, cs, topo, passes=64)
        ref = R.restatement(start, 64)
        assert sum(ref["rules"]) > 0 and ref["pass_moves"][-1] == 0
        assert one["moves"] == ref["moves"] and (one["nodes"] == ref["nodes"]).all()
    with device.Renderer(0) as r:
        r.refit_bvh(cs, topology=topo, keep_on_device=True)
        done = 0
        while True:                                                         # the call's own output, again, until nothing moves
            before = r.read_device_bvh()
            res = r.optimize_bvh_device(None, passes=R.PASSES, keep_on_device=False)
            _check(cs, before, res)
            if res["moves"] == 0:
                assert (res["nodes"] == before).all()                        # a call without a move returns its input bit for bit
                break
            done += R.PASSES
            assert done < 64, "no fixed point within 64 passes"
        with pytest.raises(abi.HijikiError) as e:                            # the links the refit kept were the old tree's: dropped
            r.refit_bvh(cs, keep_on_device=True)
        assert e.value.status == abi.HJ_ERR_STATE
        r.refit_bvh(cs, topology=res["nodes"], keep_on_device=True)
        assert (r.read_device_bvh() == res["nodes"]).all()
        with_vote = r.optimize_bvh_device(cs, passes=R.PASSES, keep_on_device=False)   # ... also with a scene: no move, no vote
        assert with_vote["moves"] == 0 and (with_vote["nodes"] == res["nodes"]).all()


@pytest.mark.parametrize("kind", ("same", "line"))
def test_ties_and_degenerate_boxes(kind):
    cs = R.tie_scene(kind)
    runs = []
    for _ in range(3):
        with device.Renderer(0) as r:
            start, res = _optimise(r, cs, E.balanced_topology(cs.num_shapes))
            _check(cs, start, res)
            runs.append(res)
    assert all((x["nodes"] == runs[0]["nodes"]).all() and x["moves"] == runs[0]["moves"] for x in runs)


def test_the_rest_of_the_route_still_works(oracle):
    cs = E.blob_scene.__wrapped__("random", 512, 520)                       # (a scene of its own: it gets a tree below)
    W, H = 96, 64
    blocks = host.make_blocks(W, H, 2, 5)
    with device.Renderer(0) as r:
        r.build_bvh(cs, keep_on_device=True)
        built = r.read_device_bvh()
        res = r.optimize_bvh_device(cs, passes=R.PASSES, keep_on_device=True)           # the vote is on
        nodes = r.read_device_bvh()
        assert res["nodes"] == len(nodes) == len(built)
        E.check_built_tree(nodes, cs)
        assert res["cost_after"] < res["cost_before"] and res["moves"] > 0            # (the optimised and voted tree is what is uploaded)
        assert (nodes != built).any()
        print({k: v for k, v in res.items()})
        r.upload_scene(cs, device_tree=True)
        r.create_framebuffer(W, H)
        st = r.render_blocks(blocks)
        got = r.read().copy()
        again = r.refit_bvh(cs, topology=nodes)                             # unmoved shapes: the optimised tree bit for bit
        assert (again == nodes).all()
    cs.set_bvh(nodes)
    want, ctr, _ = oracle.render_blocks(cs, blocks, W, H)
    assert int((got.view(np.uint32) != want.view(np.uint32)).sum()) == 0
    assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"]


def test_refusals_with_a_device():
    cs, other = E.count_scene("65"), E.count_scene("64")
    with device.Renderer(0) as r:
        with pytest.raises(abi.HijikiError) as e:
            r.optimize_bvh_device(None)
        assert e.value.status == abi.HJ_ERR_STATE
        start = r.refit_bvh(cs, topology=E.balanced_topology(65))
        r.refit_bvh(cs, topology=E.balanced_topology(65), keep_on_device=True)
        with pytest.raises(abi.HijikiError) as e:
            r.optimize_bvh_device(other)
        assert e.value.status == abi.HJ_ERR_INVALID
        assert (r.read_device_bvh() == start).all()
        with pytest.raises(ValueError):
            r.optimize_bvh_device(None, passes=65)
        assert (r.read_device_bvh() == start).all()
