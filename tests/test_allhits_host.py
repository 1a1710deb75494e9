"""hj_trace_rays_all and hj_points_inside, the part that needs no GPU: the symbols are declared, listed and exported, the version, the
header's defines and the sentences of the contract; every argument refusal in the header's order without a device, with its message
and with nothing written; the compiler's resource report of the unit; the reference of the GPU tests (allhits_ref) against itself -
hand-built scenes with counts written out by hand, the walk against brute force, the box test's special values, the vote."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import allhits_cases as cases
import allhits_ref as A
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
INF, NAN = float("inf"), float("nan")
NAMES = ("hj_trace_rays_all", "hj_points_inside")


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001900
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_ALLHITS_DEVICE_ARRAYS 1u", "#define HJ_ALLHITS_MAX_HITS 8u", "#define HJ_INSIDE_DEVICE_ARRAYS 1u", "#define HJ_INSIDE_PARITY 2u",
                 "All-hit queries (ABI 0.25)", "never shrunk", "leaf boxes are not tested", "!(T0 > T1) && !(T0 > tMax) && !(T1 < tMin)",
                 "A NaN T0, T1, tMin or tMax never culls", "(t as a float, shape index, root)", "equal t goes to the lower shape index", "a sphere's t0 enters, its t1 leaves",
                 "not on the lane, the workgroup, the launch or the chunk", "A refused call writes nothing", "the rest are (-1, 0, 0, 0)"):
        assert text in header, text
    kernel = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_multihit.h")).read()
    for text in ("NEVER shrunk", "a leaf's box is not tested", "!(T0 > T1) && !(T0 > tMax) && !(T1 < tMin)", "(t as a float, shape index, root)",
                 "no global atomics", "no inline assembly", "Gribble"):
        assert text in kernel, text
    # the directions: one set of literals in the header, the kernels (through the header) and abi.py; the properties the header claims
    lit = [[float(re.search(rf"#define HJ_INSIDE_DIR{k}_{c} (-?[0-9.]+)f", header).group(1)) for c in "XYZ"] for k in range(3)]
    d = np.array(lit, F)
    assert (d == np.array(abi.INSIDE_DIRECTIONS, F)).all() and (d == A.DIRECTIONS).all()
    assert (d != 0).all() and all(len(set(np.abs(row).tolist())) == 3 for row in d)
    assert all(np.linalg.norm(np.cross(d[i], d[j])) > 0.5 for i in range(3) for j in range(i))
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 2.0 ** -23
    assert "HJ_INSIDE_DIR0_X" in kernel
    assert (abi.ALLHITS_DEVICE_ARRAYS, abi.ALLHITS_MAX_HITS, abi.INSIDE_DEVICE_ARRAYS, abi.INSIDE_PARITY) == (1, 8, 1, 2)
    for fn in ("trace_rays_all", "points_inside"):
        assert callable(getattr(device.Renderer, fn)) and getattr(device.Renderer, fn).__doc__


# -------------------------------------------------------------------------------------------------------------------- refusals

def _refused(call, name, word, status=abi.HJ_ERR_INVALID):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call() == status, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and (name.encode() + b":") in text and word in text, (name, word, text)


def test_argument_refusals_come_before_the_device_in_order():
    L = device.lib()
    rays, counts, hits = np.full((3, 8), 7.0, F), np.full((3, 2), 7, U), np.full((3, 8, 4), 7.0, F)
    R, Cn, H = rays.ctypes.data, counts.ctypes.data, hits.ctypes.data
    assert R % 16 == 0 and Cn % 16 == 0 and H % 16 == 0
    ta = lambda r=R, n=3, k=8, f=0, c=Cn, h=H: (lambda: L.hj_trace_rays_all(None, r, n, k, f, c, h))      # noqa: E731
    name = NAMES[0]
    # each refusal alone, then each in front of every later one: the header's order
    order = [(b"null rays", dict(r=None)), (b"null hits", dict(h=None)), (b"max_hits 9", dict(k=9)), (b"unknown flag bits", dict(f=2)),
             (b"at most 2^31 - 1", dict(n=1 << 31)), (b"16-byte aligned", dict(f=1, r=R + 4))]
    for i, (word, kw) in enumerate(order):
        _refused(ta(**kw), name, word)
        for _, later in order[i + 1:]:
            if set(later) & set(kw):
                continue
            _refused(ta(**dict(later, **kw)), name, word)
    _refused(ta(c=None), name, b"null counts")
    _refused(ta(r=None, c=None), name, b"null rays")
    _refused(ta(f=0x80000000), name, b"unknown flag bits")
    _refused(ta(f=1, c=Cn + 8), name, b"16-byte aligned")
    _refused(ta(f=1, h=H + 4), name, b"16-byte aligned")
    _refused(ta(k=0xFFFFFFFF), name, b"max_hits")
    # past the argument checks: no context (and here no device); K = 0 takes null hits, aligned or not
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
    _refused(ta(), name, gate, status)
    _refused(ta(k=0, h=None), name, gate, status)
    _refused(ta(k=0, h=H + 4, f=1), name, gate, status)
    _refused(ta(n=0, r=None, c=None, h=None), name, gate, status)
    _refused(ta(f=1), name, gate, status)

    pts, out = np.full((3, 4), 7.0, F), np.full((3, 2), 7, U)
    P, O = pts.ctypes.data, out.ctypes.data
    pi = lambda p=P, n=3, f=0, o=O: (lambda: L.hj_points_inside(None, p, n, f, o))                          # noqa: E731
    name = NAMES[1]
    order = [(b"null points", dict(p=None)), (b"unknown flag bits", dict(f=4)), (b"at most 2^31 - 1", dict(n=1 << 31)), (b"16-byte aligned", dict(f=1, p=P + 4))]
    for i, (word, kw) in enumerate(order):
        _refused(pi(**kw), name, word)
        for _, later in order[i + 1:]:
            if set(later) & set(kw):
                continue
            _refused(pi(**dict(later, **kw)), name, word)
    _refused(pi(o=None), name, b"null out")
    _refused(pi(f=3, o=O + 8), name, b"16-byte aligned")
    for f in (0, 1, 2, 3):
        _refused(pi(f=f), name, gate, status)
    _refused(pi(n=0, p=None, o=None), name, gate, status)
    assert (rays == 7.0).all() and (counts == 7).all() and (hits == 7.0).all() and (pts == 7.0).all() and (out == 7).all()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_all_hit_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/multi_hit.hip (the Makefile's flags): exactly the kernels of hj_multihit.h - the walk
    with and without the list, the containment kernel in both votes -, none has scratch, and LDS only for the list: 8 x 256 x 16 B =
    32 KB a workgroup.  Occupancy is printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert "-fPIC" in flags and "-fvisibility=hidden" in flags and "-ffp-contract=off" in flags and "-O3" in flags
    assert " multi_hit " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "multi_hit.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "multi_hit.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_mh_[a-z]+<\w+>", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_mh_inside<false>", "k_mh_inside<true>", "k_mh_walk<false>", "k_mh_walk<true>"] and len(report) == 4, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] == (abi.ALLHITS_MAX_HITS * 256 * 16 if k == "k_mh_walk<true>" else 0), (k, v)
        assert v["LDS Size"] <= 32 * 1024
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_multihit.h")).read()
    assert "atomic" not in src.replace("no global atomics", "") and "asm" not in src.replace("no inline assembly", "")
    assert "fmaf" not in src and "#pragma clang fp contract(off)" in src
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "multi_hit.hip")).read()
    assert '"hj_multihit.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()


# ------------------------------------------------------------------------------------------------- the reference against itself

def test_hand_built_scenes_give_the_counts_written_out_by_hand():
    """cases.HAND: per ray the number of candidates, the crossing sum and the shapes in key order, derived in its comment; the walk
    under the hand-written tree and the brute force both give them, at K = 8 and - the head of the same list - at K = 3 and 1."""
    for name, ray, n, cross, ids in cases.HAND:
        cs, sh = cases.scene(name)
        r = np.array([ray], F)
        for brute in (False, True):
            counts, crossings, hits = A.all_hits(sh, cs.bvh, r, 8, brute=brute)
            assert (int(counts[0]), int(crossings[0])) == (n, cross), (name, ray, brute, counts, crossings)
            got = hits[0, :, 0].view(np.int32).tolist()
            assert got == list(ids[:8]) + [-1] * (8 - min(n, 8)), (name, ray, got)
            t = hits[0, :min(n, 8), 1]
            assert (np.diff(t) >= 0).all() and (t >= ray[6]).all() and (t <= ray[7]).all()
            for K in (0, 1, 3):
                c2, x2, h2 = A.all_hits(sh, cs.bvh, r, K, brute=brute)
                assert (c2 == counts).all() and (x2 == crossings).all() and h2.shape == (1, K, 4) and (h2.view(U) == hits[:, :K].view(U)).all()
    # through all nine: the sphere's roots carry u = 0 (near) and 1 (far), and the tenth candidate would not fit
    cs, sh = cases.scene("stack")
    hits = A.all_hits(sh, cs.bvh, np.array([cases.HAND[0][1]], F), 8)[2][0]
    assert hits[:4, 2].tolist() == [0.0, 0.0, 1.0, 1.0] and hits[4:, 1].tolist() == [8.0, 9.0, 10.0, 11.0]
    assert np.allclose(hits[:4, 1], [5 - 14.75 ** 0.5 / 2, 5 - 2.75 ** 0.5 / 2, 5 + 2.75 ** 0.5 / 2, 5 + 14.75 ** 0.5 / 2], rtol=1e-6)
    # the coincident quads tie on t exactly
    cs, sh = cases.scene("coincident")
    hits = A.all_hits(sh, cs.bvh, np.array([cases.HAND[4][1]], F), 8)[2][0]
    assert hits[0, 1] == hits[1, 1] == 1.0 and hits[:3, 0].view(np.int32).tolist() == [0, 1, 2]


def test_box_test_special_values_and_nans():
    lo, hi = np.array([[-1, -1, -1]], F), np.array([[1, 1, 1]], F)

    def enter(o, d, tmin=0.0, tmax=INF):
        return bool(A.box_enter(np.array([o], F), A.inverse(np.array([d], F)), F(tmin), F(tmax), lo, hi)[0])

    assert enter((0, 0, -5), (0, 0, 1)) and not enter((0, 0, -5), (0, 0, -1)) and not enter((2, 0, -5), (0, 0, 1))
    assert enter((0, 0, -5), (0, 0, 1), 4, 6) and not enter((0, 0, -5), (0, 0, 1), 0, 3.9) and not enter((0, 0, -5), (0, 0, 1), 6.1, INF)
    assert enter((0, 0, -5), (0, 0, 1), 0, 4) and enter((0, 0, -5), (0, 0, 1), 6, INF)              # (the range's ends count)
    assert enter((0, 0, -5), (-0.0, 0, 1)) and enter((0, 0, -5), (0, -0.0, 1))                       # (negative zeros: the slab's order flips, the test not)
    # in a face's plane with a zero component: 0 * inf = NaN takes one end of that axis' slab and the other end, -inf as the far
    # one or +inf as the near one, culls - the header says so ("can miss a box that a ray ... touches on its face")
    assert not enter((1, 0, -5), (0, 0, 1)) and not enter((-1, 0, -5), (0, 0, 1))
    assert enter((0, 0, 0), (0, 0, 0)) and not enter((2, 0, 0), (0, 0, 0))                           # a zero direction: the point's own boxes
    for bad in ((NAN, 0, 1), (NAN, NAN, NAN)):
        assert enter((0, 0, -5), bad)
    assert enter((NAN, 0, -5), (0, 0, 1)) and enter((0, 0, -5), (0, 0, 1), NAN, INF) and enter((0, 0, -5), (0, 0, 1), 0, NAN)


def test_walk_candidates_are_brute_force_candidates_on_every_scene():
    """On every scene and ray set the GPU tests use: the walk's candidates are a subset of the brute force's - per ray the counts are
    no larger and every listed record is one of brute force's records for that ray.  The share of rays where the two differ is printed
    (DESIGN.md quotes it): a statement about the box test, not a pass criterion.  On the hand-built scenes they are equal."""
    for name in cases.SCENES:
        cs, sh, rays = cases.case(name)
        counts, cross, hits = cases.want(name)
        bc, bx, bh = A.all_hits(sh, cs.bvh, rays, 8, brute=True)
        assert (counts <= bc).all(), name
        # every walk record with rank < 8 appears among brute force's first 8 unless brute force has more than 8
        small = bc <= 8
        for i in np.nonzero(small & (counts > 0))[0][:400].tolist():
            mine = {tuple(r) for r in hits[i, :counts[i]].view(U).tolist()}
            assert mine <= {tuple(r) for r in bh[i, :bc[i]].view(U).tolist()}, (name, i)
        differ = (counts != bc) | (cross != bx) | (hits.view(U) != bh.view(U)).any((1, 2))
        print(f"{name}: {len(rays)} rays, {int(counts.sum())} candidates by the walk, {int(bc.sum())} by brute force; "
              f"{int(differ.sum())} rays differ ({differ.mean():.4f}); rays with more than 8 candidates: {int((counts > 8).sum())}")
        if name in ("stack", "coincident"):
            k = sum(1 for h in cases.HAND if h[0] == name)
            assert not differ[:k].any()
        # what the GPU tests lean on: every kind of ray is there, and lists longer than K for every K
        assert (name == "coincident" or (counts > 8).any()) and (counts == 3).any() and (counts == 0).any() and ((counts > 1) & (counts <= 8)).any(), name


def test_vote_and_point_rays():
    pts = np.array([[0, 0, 0, 9], [1, 2, 3, 0]], F)
    rays = A.point_rays(pts)
    assert rays.shape == (6, 8) and (rays[:3, 0:3] == 0).all() and (rays[3:, 0:3] == F([1, 2, 3])).all()
    assert (rays[0:3, 3:6] == A.DIRECTIONS).all() and (rays[:, 6] == 0).all() and np.isinf(rays[:, 7]).all()
    counts, cross = np.array([1, 1, 0, 2, 3, 4], U), np.array([1, 1, 0, 2, -1, 0], np.int32)
    assert [x.tolist() for x in A.vote(counts, cross)] == [[1, 0], [2, 1]]
    assert [x.tolist() for x in A.vote(counts, cross, parity=True)] == [[1, 0], [2, 1]]
    # the cube: interior points by the oriented vote, the flipped cube by parity alone
    pts, inside, outside = cases.cube_points()
    for flipped in (False, True):
        cs = cases.cube_scene(flipped)
        sh = A.shapes_of(cs)
        got, votes = A.points_inside(sh, cs.bvh, pts)
        par, pvotes = A.points_inside(sh, cs.bvh, pts, parity=True)
        in_cube = inside & (np.abs(pts[:, 0:3]).max(1) <= 0.95)
        assert (par[inside] == 1).all() and (par[outside] == 0).all(), flipped
        assert (got[outside] == 0).all()
        if flipped:
            assert (got[in_cube] == 0).all() and (got[inside & ~in_cube] == 1).all()
        else:
            assert (got[inside] == 1).all() and (votes[inside] == 3).sum() > 0.9 * inside.sum()
