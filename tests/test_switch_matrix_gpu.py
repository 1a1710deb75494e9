"""Every entry point under every tuning switch: api/hj_tuning.h promises that no row of its table changes a result bit, and
test_gpu_parity.py::test_tuning_switches_never_change_a_bit holds one rendered frame to that.  Here the rest.

MATRIX: the upload and walk switches, and HJ_STREAM_MIN_NODES=0 - with one number the whole large-tree configuration: streamed
path state, 8 x 8 camera packets, no light-shaft grid -, each with a context of its own through EVERY query that walks the
uploaded tree with a kernel of its own: hj_trace_rays (closest hit with surface records, any-hit), hj_trace_paths with and without
an environment, hj_trace_irradiance in both forms, hj_bake_probes, hj_render_aovs, hj_render_motion, hj_closest_points,
hj_trace_rays_all, and the followed calls: hj_follow_specular, hj_render_aovs_followed, hj_render_aovs_frame_followed and
hj_render_motion_followed.  The expected values are the oracle's or the numpy restatements', as the query modules cache them; hj_render_aovs'
and the followed calls' are the restatements over the hit records of a renderer no switch has touched (`plain`).  Never a context
under the switch.
FRAMES: the switches of the render calls - how the work is dealt to workgroups, batches and slots - on rendered frames against the
oracle with the ray counts.
Each environment also shows that it took effect where the library lets one see it; where it does not, a comment says so.

ELSEWHERE names, for every other row of the table, the test file that pins it: tests/test_tuning_table_host.py fails for a row
that is in neither list, or whose file does not name it."""
import functools
import os
import re

import numpy as np
import pytest

import allhits_cases
import allhits_ref
import gather_ref as G
import motion_follow_ref as MF
import motion_ref as M
import path_query_ref as P
import probe_ref
import relayout_check as RC
import test_allhits_gpu as AH
import test_closest_gpu as CP
import test_follow_gpu as FG
import test_gather_gpu as GQ
import test_path_query_gpu as PQ
import test_probes_gpu as PV
import test_ray_query_gpu as RQ
from hijiki_amd import abi, device, host
from test_abi import ROOT
from test_aov_gpu import expected_aovs, ragged_blocks, same_bits
from test_gpu_parity import assert_same, render
from test_motion_gpu import _cameras, _moved, _scene, check

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
BIG = str(1 << 30)                                                      # the table's upper bound of the *_MIN_NODES / *_BLOCKS rows

MATRIX = [
    {"HJ_STREAM_MIN_NODES": "0"},                                       # every tree is "large"
    {"HJ_STREAM_MIN_NODES": "0", "HJ_INNER_BURST": "8", "HJ_REFILL_MIN": "32"},   # ... with the burst and refill of a tree of 600 k records
    {"HJ_PAIR_LEAVES": "0"},
    {"HJ_PAIR_MIN_NODES": BIG},                                         # the same tree through the automatic branch
    {"HJ_INNER_BURST": "1"},                                            # a round of the walk loop = the merged step alone
    {"HJ_INNER_BURST": "16", "HJ_REFILL_MIN": "1"},
    {"HJ_REFILL_MIN": "64"},                                            # refill only when the whole wave is idle
    {"HJ_NODE_ORDER": "0", "HJ_COLLAPSE_PCT": "0"},
    {"HJ_NODE_ORDER": "1", "HJ_COLLAPSE_PCT": "1000"},
    {"HJ_LEAF_GUARDS": "0"},
    {"HJ_UPLOAD_DEVICE": "1"},
    {"HJ_UPLOAD_DEVICE_MIN": "0"},                                      # the same route through the automatic branch
    {"HJ_UPLOAD_DEVICE": "1", "HJ_RL_DEBUG": "1"},
]

SPLIT = abi.RENDER_SPLIT_KERNELS | abi.RENDER_TIME_KERNELS              # (the per-bounce table needs the timer: render_batch_split)
SMALL, EVEN, ODD, MANY = (160, 96, 3, 31), (130, 130, 2, 5), (130, 130, 3, 5), (130, 130, 40, 5)   # (W, H, spp, seed): 6, 8, 12, 160 blocks
# (environment, scene fixtures, frames, hj_render_opts fields); hj_render_blocks reconstructs every batch it renders
FRAMES = [
    ({"HJ_STREAM_MIN_NODES": "0"}, ("cbox_small", "cbox_spheres"), (SMALL,), {}),
    ({"HJ_XCD_DEAL": "1", "HJ_WG_SMALL": "8"}, ("cbox_spheres",), ((160, 96, 1, 31), ODD, EVEN), {}),     # 2, 12, 8 blocks
    ({"HJ_BATCH_CAP": "64"}, ("cbox_spheres",), (MANY,), {}),
    ({"HJ_WG_SMALL": "1", "HJ_WG_SMALL_BLOCKS": BIG}, ("cbox_spheres",), (SMALL,), {}),                   # every call small: one workgroup per CU
    ({"HJ_WG_SMALL_BLOCKS": "0"}, ("cbox_spheres",), (SMALL,), {}),                                       # no call small
    ({"HJ_SLOTS": "2"}, ("cbox_spheres",), (SMALL,), {"batch_blocks": 1}),
    ({"HJ_SLOTS": "4"}, ("cbox_spheres",), (SMALL,), {"batch_blocks": 1}),
    ({"HJ_RECON_PRIORITY": "0"}, ("cbox_spheres",), (SMALL, EVEN), {}),
    ({"HJ_LDS_PAD_KB": "16"}, ("cbox_spheres",), (SMALL,), {}),
    ({"HJ_TRACE_BOUNCES": "1"}, ("cbox_spheres",), (SMALL,), {"flags": SPLIT}),
    ({"HJ_UPLOAD_TIMING": "1", "HJ_LIGHT_GRID_TIMING": "1"}, ("cbox_small",), (SMALL,), {}),
    ({"HJ_LDS_PAD_KB": "64"}, ("cbox_spheres",), (SMALL,), {}),                                           # the table's bound: see the test's text
]

# every other row of the table: the file whose tests run it with a value
_GPU, _LBVH, _RAYS, _PATHS = "tests/test_gpu_parity.py", "tests/test_lbvh_edges_gpu.py", "tests/test_ray_query_gpu.py", "tests/test_path_query_gpu.py"
ELSEWHERE = {
    "HJ_POOL": _GPU, "HJ_WG_PER_CU": _GPU, "HJ_STREAM_STATE": _GPU, "HJ_MEM_LIMIT_MB": _GPU, "HJ_ALLOC_LIMIT_MB": _GPU,
    "HJ_COMM_SHARED_GPU": _GPU, "HJ_COMM_FORCE_RCCL": _GPU,
    "HJ_GROUP_TILE": "tests/test_walk_forms_gpu.py",
    "HJ_LIGHT_GRID": "tests/test_shade_step_gpu.py", "HJ_LIGHT_GRID_MESH": "tests/test_light_grid.py",
    "HJ_LBVH_TIMING": _LBVH, "HJ_LBVH_BIG_PCT": _LBVH, "HJ_LBVH_CLUSTER": _LBVH, "HJ_LBVH_SAH": _LBVH, "HJ_LBVH_TOP_ROTATE": _LBVH,
    "HJ_LBVH_VOTE_PATHS": _LBVH, "HJ_REFIT_TILED": _LBVH, "HJ_BVH_CHILD_ORDER": _LBVH,
    "HJ_BVH_VOTE_SHADOW": "tests/test_vote_gpu.py",
    "HJ_TRACE_PERSISTENT": _RAYS, "HJ_TRACE_WG_RAYS": _RAYS, "HJ_TRACE_CHUNK": _RAYS,
    "HJ_CLOSEST_ORDERED": "tests/test_closest_gpu.py",
    "HJ_PATHS_POOL": _PATHS, "HJ_PATHS_WGS": _PATHS, "HJ_PATHS_CHUNK": _PATHS,
    "HJ_LIGHTMAP_LANE_TEXELS": "tests/test_lightmap_gpu.py", "HJ_LIGHTMAP_SLICES": "tests/test_lightmap_gpu.py",
    "HJ_LIGHTMAP_FILTER_LDS_STEP": "tests/test_lightmap_filter_gpu.py",
    "HJ_DENOISE_LDS_STEP": "tests/test_denoise_gpu.py",
}

N_PATHS, N_FLAT, K_ALL = 513, 1025, 3                                   # rays of a path query; points and rays of the flat queries; hits kept per ray
GATHER = ("hemisphere-1", "sphere-sh9-4")                               # gather_ref.MODES: the hemisphere and the sphere form
MOTION_SIZES = ((9, 9), (70, 41))
FOLLOW_AOVS, FOLLOW_MOTION, FOLLOW_SIZE = 2, 8, (70, 41)                # max_follow of the followed AOV calls and of the followed motion image; its size


def _id(env):
    return ",".join(f"{k.replace('HJ_', '')}={v}" for k, v in env.items()) or "default"


def table_names():
    """every "HJ_..." name api/hj_tuning.h holds: the rows and the presence flags"""
    return sorted(set(re.findall(r'"(HJ_[A-Z0-9_]+)"', open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_tuning.h")).read())))


@pytest.fixture(autouse=True)
def _no_switch_from_outside(monkeypatch):
    names = table_names()
    for env in MATRIX + [f[0] for f in FRAMES]:
        assert set(env) <= set(names), env                              # (a switch the table does not know would switch nothing)
    for name in names:
        monkeypatch.delenv(name, raising=False)


def switch_on(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def tree_counts(r, cs):
    """relayout_check's verdict on the tree the context holds for `cs`, and the walk in canonical form"""
    tree = r.scene_tree()
    counts = RC.check_tree(tree, cs.bvh, len(cs.spheres), len(cs.quads), True, cs=cs)
    return counts, RC.canonical(tree, cs.bvh)


@pytest.fixture(scope="module")
def plain():
    """What only a renderer can say, from one that no switch has touched - created, and used for the last time, before any test of
    this module puts a switch into the environment (a module fixture is set up before the function fixtures of its first test; the
    table's names are taken out here as well): hj_render_aovs' expected image, the default tree of the scene the premises look at,
    and how many next-event samples the light-shaft grid answers by default."""
    saved = {n: os.environ.pop(n) for n in table_names() if n in os.environ}
    try:
        out = {}
        with device.Renderer(0) as r:
            cs = P.scene("rich")
            r.upload_scene(cs)
            out["aovs"] = expected_aovs(r, cs, 40, 24, ragged_blocks())
            r.upload_scene(_scene())
            out["counts"], out["walk"] = tree_counts(r, _scene())
            r.upload_scene(P.scene("cbox"))
            out["free"] = r.trace_paths(P.ray_set("cbox")[:N_PATHS], opts=P.options(40), stats=True)[1]["shadow_rays_proven_free"]
            # the followed calls: the per-record query's records and restatement, the followed sums of the ragged block list and of
            # the 64 x 64 frame at max_follow 2, and the followed motion image at 8 with every kind moved - all on "rich" but the records
            out["follow"] = FG.records(r)[0:4:3] + (FG.records(r)[1],)
            out["followed"] = {key: FG.expected(r, "rich", key, FOLLOW_AOVS)[0] for key in ("ragged", "64")}
            cs = P.scene("rich")
            r.upload_scene(cs)
            out["prev"] = M.Prev(cs, _cameras(cs)["translated"], **_moved(cs, 5))
            out["motion followed"], det = MF.render_motion_followed(cs, out["prev"], *FOLLOW_SIZE, FOLLOW_MOTION, FG.gpu_trace(r), detail=True)
            assert det["went"].sum() > 50 and det["count"].max() >= 3 and det["left"].any()
    finally:
        os.environ.update(saved)
    w, c = out["aovs"], out["counts"]
    # (the scene is closed: every sample hits, so word 11 - the hits - is word 3 - the samples; the repeated block's pixels have four)
    assert (w[..., 3] == 3).sum() == 40 * 24 - 256 and (w[:16, :16, 3] == 4).all() and (w[..., 11] > 0).all() and w[..., 0:3].any()
    assert c["pairs"] > 0 and c["guards"] > 0 and c["dropped"] > 0, c                     # what the switches below take away is there by default
    assert out["free"] > 0
    w.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_paths(name):
    """path_query_ref.compose of the first N_PATHS rays (a record depends on its own ray alone), with the counts of exactly these"""
    samples, counts = P.compose(P.scene(name), P.ray_set(name)[:N_PATHS], 1, P.options(40))
    samples.setflags(write=False)
    return samples, counts


@functools.lru_cache(maxsize=None)
def expected_all_hits(nodes_key):
    """allhits_ref under the nodes the upload was fed (test_allhits_gpu.upload), the first N_FLAT rays of the mesh case"""
    _, sh, rays = allhits_cases.case("mesh")
    return allhits_ref.all_hits(sh, np.frombuffer(nodes_key, U).reshape(-1, 8), rays[:N_FLAT], 8)


def queries(r, oracle, plain, what):
    """every entry point that walks the uploaded tree, on the context `r`; each against its own reference, on bits"""
    # hj_trace_rays: ids, t, u, v and the surface records; any-hit
    cs, rays, want, _ = RQ.case("cluster")
    r.upload_scene(cs)
    got = r.trace_rays(rays, surface=True)
    RQ.assert_hits(got, want, f"trace_rays, {what}")
    RQ.assert_surface(cs, got, want, f"trace_rays, {what}")
    ai, at, au, av = r.trace_rays(rays, any_hit=True)
    assert ((ai >= 0) == (want[0] >= 0)).all(), f"any-hit booleans, {what}"
    miss = ai < 0
    assert (ai[miss] == -1).all() and not (RQ.bits(at)[miss] | RQ.bits(au)[miss] | RQ.bits(av)[miss]).any(), f"any-hit misses, {what}"
    # hj_trace_paths: triangle leaves through the kernels without and with an environment
    for name in ("rich", "env"):
        samples, counts = expected_paths(name)
        r.upload_scene(P.scene(name))
        got, stats = r.trace_paths(P.ray_set(name)[:N_PATHS], opts=P.options(40), stats=True)
        PQ.assert_samples(got, samples, f"trace_paths {name}, {what}")
        PQ.assert_counts(stats, counts, f"trace_paths {name}, {what}")
    # hj_trace_irradiance in both forms, hj_bake_probes, hj_render_aovs: the scene with triangles
    cs = P.scene("rich")
    r.upload_scene(cs)
    for mode in GATHER:
        records, counts = G.expected("rich", mode)
        got, stats = GQ.run(r, "rich", mode)
        GQ.assert_records(got, records, f"trace_irradiance {mode}, {what}")
        GQ.assert_counts(stats, counts, f"trace_irradiance {mode}, {what}")
    d, volume, _, counts = probe_ref.expected_bake("rich")
    got, stats = r.bake_probes(**PV.grid_kw(d, seed=PV.SEED, seed_stride=PV.STRIDE), spp=probe_ref.BAKE_SPP, opts=P.options(40), stats=True)
    PV.assert_bits(got.reshape(-1, 28), volume, f"bake_probes, {what}")
    assert {k: stats[k] for k in G.COUNTS} == {k: counts[k] for k in G.COUNTS}, f"bake_probes, {what}"
    same_bits(r.render_aovs(40, 24, blocks=ragged_blocks()), plain["aovs"], f"render_aovs, {what}")
    # hj_render_motion: one pixel into the next tile both ways, and a launch of several workgroups
    cs = _scene()
    prev = M.Prev(cs, _cameras(cs)["translated"], **_moved(cs, 5))
    r.upload_scene(cs)
    for W, H in MOTION_SIZES:
        check(r, oracle, cs, prev, W, H, "rest", f"render_motion {W} x {H}, {what}")
    # hj_follow_specular on the box's records; the followed AOVs in block and in frame form and the followed motion image on "rich"
    rays, want, hits = plain["follow"]
    r.upload_scene(P.scene("cbox"))
    same_bits(r.follow_specular(rays, hits), want, f"follow_specular, {what}")
    r.upload_scene(P.scene("rich"))
    same_bits(r.render_aovs(40, 24, blocks=FG.ragged_blocks(), follow=FOLLOW_AOVS), plain["followed"]["ragged"], f"render_aovs followed, blocks, {what}")
    same_bits(r.render_aovs(64, 64, spp=2, master_seed=31, follow=FOLLOW_AOVS), plain["followed"]["64"], f"render_aovs followed, frame, {what}")
    same_bits(r.render_motion(plain["prev"], *FOLLOW_SIZE, follow=FOLLOW_MOTION), plain["motion followed"], f"render_motion followed, {what}")
    # hj_closest_points and hj_trace_rays_all read the verbatim copy at root2: no re-layout switch may move them
    cs, _, pts, want = CP.case("mesh")
    fed = AH.upload(r, cs, "host_tree")                                 # (asserts that the second copy is the uploaded array)
    CP.assert_records(r.closest_points(pts[:N_FLAT]), want[:N_FLAT], f"closest_points, {what}")
    cs2, _, rays = allhits_cases.case("mesh")
    assert (np.array(cs2.bvh, U) == fed).all()                          # (both cases are scenes.smooth_mesh_scene(11))
    AH.assert_same(r.trace_rays_all(np.array(rays[:N_FLAT]), K_ALL), AH.head(expected_all_hits(fed.tobytes()), K_ALL), f"trace_rays_all, {what}")


def premise(r, plain, env, err):
    """the environment took effect, shown on the tree of hj_render_motion's scene above (the box with a 1280-triangle mesh, two
    spheres and two quads: pair nodes, leaf guards and collapsed nodes by default) - and through whatever else the library lets one see"""
    cs = _scene()
    r.upload_scene(cs)
    tree = r.scene_tree()
    no_pairs = env.get("HJ_PAIR_LEAVES") == "0" or "HJ_PAIR_MIN_NODES" in env
    counts = RC.check_tree(tree, cs.bvh, len(cs.spheres), len(cs.quads), not no_pairs, cs=cs)
    walk = RC.canonical(tree, cs.bvh)
    default, what = plain["counts"], _id(env)
    if no_pairs:
        assert counts["pairs"] == 0, (what, counts)
    if env.get("HJ_LEAF_GUARDS") == "0":
        assert counts["guards"] == 0, (what, counts)
    if "HJ_COLLAPSE_PCT" in env:
        # 0: every inner node whose children lie inside it goes (its area exceeds 0 x its ancestor's); 1000: none can be ten times its ancestor
        # (the default's 50 per cent lies between the two)
        assert counts["dropped"] == 0 if env["HJ_COLLAPSE_PCT"] == "1000" else counts["dropped"] > default["dropped"], (what, counts, default)
        assert walk.shape != plain["walk"].shape or (walk != plain["walk"]).any(), f"{what}: the walk is the default one"
        # (HJ_NODE_ORDER places records and changes no link: nothing of it shows in the canonical form, and which order the
        # default takes for a tree is not exposed - test_relayout_gpu.py checks each order's tree by itself)
    if not (no_pairs or "HJ_COLLAPSE_PCT" in env or "HJ_LEAF_GUARDS" in env):
        assert walk.shape == plain["walk"].shape and (walk == plain["walk"]).all(), f"{what}: another walk than the default one"
    if "HJ_STREAM_MIN_NODES" in env:
        # no light-shaft grid: the default context's grid answers next-event samples of these rays, this one's none.  (Streamed path
        # state and the 8 x 8 packets show in no statistic; HJ_STREAM_STATE / HJ_GROUP_TILE alone are ELSEWHERE's.)
        r.upload_scene(P.scene("cbox"))
        stats = r.trace_paths(P.ray_set("cbox")[:N_PATHS], opts=P.options(40), stats=True)[1]
        assert plain["free"] > 0 and stats["shadow_rays_proven_free"] == 0, (what, plain["free"], stats["shadow_rays_proven_free"])
    if "HJ_RL_DEBUG" in env:
        assert "rl debug:" in err, f"{what}: the device re-layout did not report its stages"      # (only scene_relayout.hip prints it: the route is the device's)
    # HJ_UPLOAD_DEVICE / HJ_UPLOAD_DEVICE_MIN without HJ_RL_DEBUG: both routes derive the same walk (asserted above) and the library
    # exposes nothing else of the route.  HJ_INNER_BURST / HJ_REFILL_MIN: DeviceScene::inner_burst and refill_min are read by the
    # kernels alone; no statistic counts rounds or refills.
    return counts


@pytest.mark.parametrize("env", MATRIX, ids=_id)
def test_every_query_under_the_switch(oracle, plain, monkeypatch, capfd, env):
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:                                       # a context of its own: some rows are read when it is created
        queries(r, oracle, plain, _id(env))
        err = capfd.readouterr().err
        counts = premise(r, plain, env, err)
    print(f"{_id(env)}: {counts}")


# --------------------------------------------------------------------------------------------------------------------- frames

_ORACLE = {}


def oracle_frame(oracle, name, cs, frame):
    """the oracle's frame and counters, once per (scene, frame)"""
    if (name, frame) not in _ORACLE:
        W, H, spp, seed = frame
        _ORACLE[name, frame] = oracle.render_blocks(cs, host.make_blocks(W, H, spp, seed), W, H)[0:2]
    return _ORACLE[name, frame]


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("env,names,frames,fields", FRAMES, ids=[_id(f[0]) for f in FRAMES])
def test_frames_under_the_switch(request, oracle, monkeypatch, capfd, env, names, frames, fields):
    """The frame is the oracle's bit for bit, with its ray counts.

    HJ_XCD_DEAL: wg_group() (kernels/hj_stages.h) gives workgroup g group g >> 3 of every block b = 8 k + (g & 7) - a bijection
    between (g, k) and the batch's 256 groups per block exactly when there are 8 x 256 = 2048 workgroups, which is what
    stage_blocks() demands before it switches the deal on: fewer blocks than 8 (some XCDs' workgroups get nothing), a count that is
    no multiple of 8 and one that is.  HJ_WG_SMALL=8 makes these small calls' workgroup count 8 per CU.  The library exposes
    nothing that shows which deal a batch took.
    HJ_LDS_PAD_KB: the path kernel's static LDS is WgSharedEnv - 2 x 512 hot-node float4s and under 200 bytes of counters: 16 560
    bytes in the compiler's resource report -, a gfx950 workgroup may be given 160 KiB, so the largest pad that still launches is
    floor((163 840 - 16 560) / 1024) = 143 KiB and the table's bound of 64 fits: it runs here (tests/test_tuning_table_host.py pins
    the sum).  A pad shows in no statistic."""
    if "HJ_XCD_DEAL" in env and cus() * 8 != 2048:
        pytest.skip(f"the XCD deal needs 2048 workgroups: {cus()} CUs x 8 = {cus() * 8}")
    opts = device.default_opts()
    for k, v in fields.items():
        setattr(opts, k, getattr(opts, k) | v if k == "flags" else v)
    switch_on(monkeypatch, env)
    what = _id(env)
    for name in names:
        cs = request.getfixturevalue(name)
        with device.Renderer(0) as r:
            for frame in frames:
                W, H, spp, seed = frame
                want, ctr = oracle_frame(oracle, name, cs, frame)
                got, st = render(r, cs, W, H, host.make_blocks(W, H, spp, seed), opts)
                assert_same(got, want, f"{what}, {name} {W} x {H} x {spp}")
                assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"], (what, name, frame)
                n = len(host.make_blocks(W, H, spp, seed))
                if "HJ_BATCH_CAP" in env:
                    assert n == 160 and st["batches"] >= 3, (n, st["batches"])         # batches of the cap's 64 blocks
                if "HJ_SLOTS" in env:
                    assert st["batches"] == n > int(env["HJ_SLOTS"]), (n, st["batches"])   # more one-block batches than slots: they rotate
                if "HJ_STREAM_MIN_NODES" in env:
                    assert st["shadow_rays_proven_free"] == 0, st["shadow_rays_proven_free"]   # no light-shaft grid
                # HJ_RECON_PRIORITY, HJ_WG_SMALL / HJ_WG_SMALL_BLOCKS, HJ_LDS_PAD_KB: which stream reconstructs, how many workgroups a
                # call gets and how much LDS each holds show in no statistic and in nothing else the library exposes
        err = capfd.readouterr().err
        if "HJ_TRACE_BOUNCES" in env:
            assert "[bounce   0]" in err, err[-300:]
        if "HJ_UPLOAD_TIMING" in env:
            assert "hj_scene_upload:" in err and "light grid:" in err, err[-300:]
