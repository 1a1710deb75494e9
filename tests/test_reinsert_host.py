"""hj_optimize_bvh_device, the part that needs no GPU: the symbol is declared, listed and exported, the refusals that come before the
device, the compiler's resource report of the new unit (no scratch: the search has no stack), and the GPU test's input checked on
the CPU (the host's passes gain a great deal from the shuffled start), and the pass itself restated on the host
(tests/reinsert_restatement.hip calls the steps of api/tree_reinsert.h from plain loops): what the GPU test compares the device with."""
import ctypes as C
import os
import re
import subprocess

from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions

import lbvh_edges as E
import refit_scenes
import reinsert_scenes as R


def _call(ctx, passes):
    return device.lib().hj_optimize_bvh_device(ctx, None, passes, None, 0, None, None, None, None)


def test_entry_point_is_declared_listed_and_exported():
    assert "hj_optimize_bvh_device" in declared_functions("hijiki_hip.h")
    assert "hj_optimize_bvh_device" in device.EXPORTS and hasattr(device.lib(), "hj_optimize_bvh_device")
    assert device.lib().hj_version() >= 0x000F00
    assert abi.REINSERT_MAX_PASSES == 64
    assert callable(device.Renderer.optimize_bvh_device)


def test_refusals_that_need_no_device():
    L = device.lib()
    L.hj_context_create(-1, None)                                          # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert _call(None, 65) == abi.HJ_ERR_INVALID
    text = L.hj_last_error(None)
    assert text != before and b"hj_optimize_bvh_device" in text and b"65" in text
    moves, cost = C.c_uint32(7), C.c_double(7.0)
    rc = L.hj_optimize_bvh_device(None, None, 8, None, 0, None, C.byref(cost), C.byref(cost), C.byref(moves))
    if L.hj_device_count() == 0:                                           # a valid call without a GPU: there is no context to give it
        assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
    else:
        assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert moves.value == 7 and cost.value == 7.0


def test_new_kernels_use_no_scratch(tmp_path):
    """The search walks through the parent links: no stack, so no scratch memory - the compiler's own report for
    api/tree_reinsert.hip with the Makefile's flags gives 0 bytes per lane for every kernel of the unit (DESIGN.md 4 has the table)."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "tree_reinsert.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "tree_reinsert.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in report.items() if "k_ri_" in k}
    for want in ("k_ri_init", "k_ri_search", "k_ri_lock", "k_ri_check", "k_ri_win", "k_ri_apply", "k_ri_cost", "k_ri_climb", "k_ri_flatten"):
        assert any(want in k for k in kernels), (want, sorted(report))
    assert len(kernels) == 13, sorted(kernels)                             # (lock, check, win: two conflict rules; climb: boxes and sizes)
    for k, v in kernels.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["LDS Size"] == (2048 if "k_ri_cost" in k else 0), (k, v)     # (the cost's sum tree)


def test_the_shuffled_start_has_a_great_deal_to_gain():
    """The input of tests/test_reinsert_gpu.py::test_it_optimises proves something only if the host's passes gain much from it."""
    cs, start, c0, c_host = R.shuffled_case()
    E.check_built_tree(start, cs)
    print(f"shuffled start: cost {c0:.3f}, after the host's {R.PASSES} passes {c_host:.3f}")
    assert c_host < 0.25 * c0
    for kind in ("same", "line"):
        tie = R.tie_scene(kind)
        E.check_built_tree(E.refit_reference(E.balanced_topology(tie.num_shapes), tie), tie)


def _leaves(nodes):
    return E.record_multiset(nodes[nodes[:, 3] != E.INNER])


def test_host_restatement_optimises_and_keeps_a_tree():
    """The steps of api/tree_reinsert.h on the host, from the shuffled 1025-sphere start: a valid tree with the same leaves after 8
    passes (the program checks the links after every pass as well), at least 0.7 of the host optimiser's gain, the area sum lower after
    every pass."""
    cs, start, c0, c_host = R.shuffled_case()
    res = R.restatement(start, R.PASSES)
    E.check_built_tree(res["nodes"], cs)
    assert (_leaves(res["nodes"]) == _leaves(start)).all()
    c_dev = refit_scenes.sa_cost(res["nodes"])
    assert abs(c_dev - res["cost_after"]) <= 1e-9 * c_dev and abs(res["cost_before"] - c0) <= 1e-9 * c0
    share = (c0 - c_dev) / (c0 - c_host)
    print(f"c0 {c0:.4f}, restated {c_dev:.4f}, c_host {c_host:.4f}, moves {res['moves']}, share {share:.4f}")
    assert c0 - c_dev >= 0.7 * (c0 - c_host), share
    assert all(b < a for a, b in zip(res["sums"], res["sums"][1:]))


def test_host_restatement_reaches_a_fixed_point():
    """... and from the shuffled 257-sphere start of the GPU test: a pass without a move within 64 passes, the area sum lower after
    every pass that moved something - also where a pass had to be done again by the whole-path rule; ties and zero areas move nothing."""
    cs = E.count_scene("257")
    start = E.refit_reference(R.shuffled_topology(257), cs)
    res = R.restatement(start, 64)
    assert sum(res["rules"]) > 0                                            # (this start has a pass that is done again by the whole-path rule)
    print(f"{res['passes']} passes, {res['moves']} moves, whole-path passes {sum(res['rules'])}, cost {res['cost_before']:.4f} -> {res['cost_after']:.4f}")
    assert res["passes"] < 64 and res["pass_moves"][-1] == 0 and res["moves"] > 0
    moving = res["sums"][:-1]
    assert all(b < a for a, b in zip(moving, moving[1:]))
    E.check_built_tree(res["nodes"], cs)
    again = R.restatement(res["nodes"], 8)
    assert again["moves"] == 0 and (again["nodes"] == res["nodes"]).all()
    for kind in ("same", "line"):
        tie = R.tie_scene(kind)
        t0 = E.refit_reference(E.balanced_topology(tie.num_shapes), tie)
        assert R.restatement(t0, 8)["moves"] == 0
