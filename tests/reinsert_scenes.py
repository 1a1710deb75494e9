"""Shared by tests/test_reinsert_host.py and tests/test_reinsert_gpu.py: the inputs of hj_optimize_bvh_device's tests - scenes, the
topologies installed through the refit, the shuffled tree with a great deal to gain and the host's result from the same start."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

import lbvh_edges as E
import refit_scenes

PASSES = 8
SIZES = ("2", "3", "4", "64", "65", "256", "257", "1025", "sphere+quad+triangle")
TOPOLOGIES = {"balanced": E.balanced_topology, "chain": refit_scenes.chain_topology, "left spine": E.left_spine_topology}


def shuffled_topology(n, seed=7):
    """the balanced topology with its leaves' shapes permuted: neighbours in the tree are far apart in space"""
    topo = E.balanced_topology(n)
    perm = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    leaf = topo[:, 3] != E.INNER
    topo[leaf, 3] = perm[topo[leaf, 3]]
    return topo


@functools.lru_cache(maxsize=None)
def shuffled_case():
    """(scene of 1025 random small spheres, start records, c0, c_host): c_host = the cost of the same start after the host's PASSES
    insertion passes (hjh_compiled_tune_bvh without the vote, which does not change the cost), computed once, on the CPU."""
    cs = E.count_scene("1025")
    start = E.refit_reference(shuffled_topology(1025), cs)
    tuned = E.count_scene.__wrapped__("1025")                              # (a scene of its own: the shared one keeps no tree)
    tuned.set_bvh(start)
    tuned.tune_bvh(reinsert_passes=PASSES, vote_paths=0)
    return cs, start, refit_scenes.sa_cost(start), refit_scenes.sa_cost(tuned.bvh)


@functools.lru_cache(maxsize=None)
def tie_scene(kind):
    """"same": 257 spheres with one centre and radius (every gain ties); "line": 64 zero-radius spheres on a line (every area is zero)"""
    if kind == "same":
        return E._compile(spheres=[(0.5, 0.5, 0.5, 0.125)] * 257, emitter=0)
    return E._compile(spheres=[(k / 64.0, 0.5, 0.5, 0.0) for k in range(64)], emitter=0)


@functools.lru_cache(maxsize=None)
def _restatement_program():
    """tests/reinsert_restatement.hip compiled once a session (host code only is run)"""
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tempfile.mkdtemp(prefix="reinsert_restatement_")
    exe = os.path.join(tmp, "reinsert_restatement")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
           os.path.join(here, "reinsert_restatement.hip"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=tmp))
    assert out.returncode == 0, out.stderr[-2000:]
    return tmp, exe


def restatement(start, passes):
    """hj_optimize_bvh_device restated on the host (tests/reinsert_restatement.hip: the steps of api/tree_reinsert.h in plain loops)
    -> dict: nodes, moves, passes (run), cost_before, cost_after, sums (the area sum after every pass), rules (per pass: whole path?)"""
    tmp, exe = _restatement_program()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.ascontiguousarray(start, np.uint32).tofile(fin)
    out = subprocess.run([exe, fin, fout, str(int(passes))], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-500:])
    m = re.search(r"result passes (\d+) moves (\d+) cost_before (\S+) cost_after (\S+)", out.stdout)
    per_pass = re.findall(r"pass \d+: (\d+) moves( \(whole-path rule\))?, area sum (\S+)", out.stdout)
    return {"nodes": np.fromfile(fout, np.uint32).reshape(-1, 8), "passes": int(m.group(1)), "moves": int(m.group(2)),
            "cost_before": float(m.group(3)), "cost_after": float(m.group(4)), "pass_moves": [int(p[0]) for p in per_pass],
            "rules": [bool(p[1]) for p in per_pass], "sums": [float(p[2]) for p in per_pass]}
