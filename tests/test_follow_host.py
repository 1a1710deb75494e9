"""hj_follow_specular, hj_render_aovs_followed and hj_render_aovs_frame_followed, the part that needs no GPU: the symbols, the
version, the defines and the contract's key sentences in the header and in DESIGN.md; every argument refusal of the three calls in
the header's order without a device, with its message and with nothing written; the compiler's resource report of the unit; the
reference of the GPU tests (follow_ref) against itself on fabricated records, each input chosen by computing k and fr; and the
premise of the GPU tests - every branch class occurs among the query rays - from the oracle's hits."""
import os
import re
import subprocess

import numpy as np
import pytest

import follow_ref as R
import path_query_ref as P
from hijiki_amd import abi, device, host
from test_abi import ROOT, declared_functions
from test_aov_host import _block, _in_order, _refused
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_follow_specular", "hj_render_aovs_followed", "hj_render_aovs_frame_followed")


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001E00
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in ("#define HJ_AOV_MAX_FOLLOW 8", "#define HJ_FOLLOW_DEVICE_ARRAYS 1u", "Followed AOVs (ABI 0.30)", "reflect when k <= 0 or fr >= 0.5f, else refract",
                 "not normalised, as the reference leaves it", "tMin = +inf, tMax = -inf", "(t0 + t1) + t2", "planar mirror's virtual image",
                 "max_follow == 0 is hj_render_aovs bit for bit", "word 11, is exactly hj_render_aovs'", "then max_follow above HJ_AOV_MAX_FOLLOW",
                 "glass extinction does not tint the followed albedo", "hj_render_motion still stops at the first hit",
                 "hj_render_aovs_followed below"):
        assert text in header, text
    for text in ("Followed AOVs", "hj_follow_specular", "k_aov_follow", "fr >= 0.5f", "kernels/hj_follow.h", "api/follow.hip"):
        assert text in design, text
    assert (abi.AOV_MAX_FOLLOW, abi.FOLLOW_DEVICE_ARRAYS) == (8, 1)
    assert '"hj_follow.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "api/follow.hip" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_internal.h")).read()
    assert callable(device.Renderer.follow_specular) and device.Renderer.follow_specular.__doc__
    assert "follow" in device.Renderer.render_aovs.__code__.co_varnames
    with pytest.raises(ValueError):
        device.Renderer.render_aovs(None, 4, 4, spp=1, follow=9)


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    """every test of this file is about the three calls, the reference's self-checks included: none passes without the symbols"""
    assert all(hasattr(device.lib(), n) and n in device.EXPORTS for n in NAMES)


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_argument_refusals_come_before_the_device_in_order():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"

    rays, hits, out = np.full((3, 8), 7.0, F), np.full((3, 4), 7.0, F), np.full((3, 8), 7.0, F)
    Rp, Hp, Op = rays.ctypes.data, hits.ctypes.data, out.ctypes.data
    assert Rp % 16 == 0 and Hp % 16 == 0 and Op % 16 == 0
    fs = lambda r=Rp, h=Hp, n=3, f=0, o=Op: (lambda: L.hj_follow_specular(None, r, h, n, f, o))                 # noqa: E731
    name = NAMES[0]
    _in_order(fs, name, [(b"null rays", dict(r=None)), (b"unknown flag bits", dict(f=2)), (b"at most 2^31 - 1", dict(n=1 << 31)),
                         (b"16-byte aligned", dict(f=1, h=Hp + 4))])
    _refused(fs(h=None), name, b"null hits")
    _refused(fs(o=None), name, b"null out_rays")
    _refused(fs(f=0x80000000), name, b"unknown flag bits")
    _refused(fs(f=1, r=Rp + 8), name, b"16-byte aligned")
    _refused(fs(f=1, o=Op + 4), name, b"16-byte aligned")
    for f in (0, 1):
        _refused(fs(f=f), name, gate, status)
    _refused(fs(r=Rp + 4), name, gate, status)                          # (host arrays need no alignment)
    _refused(fs(n=0, r=None, h=None, o=None), name, gate, status)

    W, Hh = 40, 24
    blocks = (abi.ImageBlock * 2)(_block(W, Hh), _block(W, Hh, origin=(16, 0)))
    bad_orig = (abi.ImageBlock * 2)(_block(W, Hh), _block(W, Hh + 1))
    bad_dim = (abi.ImageBlock * 2)(_block(W, Hh), _block(W, Hh, dim=(129, 1)))
    aov = np.full((Hh, W, 12), 7.0, F)
    Ap = aov.ctypes.data
    assert Ap % 16 == 0
    ra = lambda b=blocks, n=2, w=W, h=Hh, m=2, f=0, a=Ap: (lambda: L.hj_render_aovs_followed(None, b, n, w, h, m, f, a))   # noqa: E731
    name = NAMES[1]
    _in_order(ra, name, [(b"null blocks", dict(b=None)), (b"unknown flag bits", dict(f=2)), (b"image 0 x", dict(w=0)),
                         (b"original_dimension", dict(b=bad_orig)), (b"16-byte aligned", dict(f=1, a=Ap + 4)), (b"max_follow 9 above 8", dict(m=9))])
    _refused(ra(a=None), name, b"null aov")
    _refused(ra(h=16385), name, b"x 16385")
    _refused(ra(w=16385), name, b"image 16385 x")
    _refused(ra(b=bad_dim), name, b"dimension 129 x 1 above 128")
    _refused(ra(m=0xFFFFFFFF), name, b"max_follow 4294967295 above 8")
    for m in (0, 1, 8):
        for f in (0, 1):
            _refused(ra(m=m, f=f), name, gate, status)
    _refused(ra(b=None, n=0), name, gate, status)

    rf = lambda w=W, h=Hh, spp=4, p0=0, p1=4, m=2, f=0, a=Ap: (lambda: L.hj_render_aovs_frame_followed(None, w, h, spp, 99, p0, p1, m, f, a))   # noqa: E731
    name = NAMES[2]
    _in_order(rf, name, [(b"null aov", dict(a=None)), (b"unknown flag bits", dict(f=4)), (b"image 0 x", dict(w=0)), (b"max_follow 9 above 8", dict(m=9)),
                         (b"bad pass range [3,2)", dict(p0=3, p1=2))])
    _refused(rf(h=16385), name, b"x 16385")
    _refused(rf(f=1, a=Ap + 4), name, b"16-byte aligned")
    _refused(rf(f=1, a=Ap + 4, m=9), name, b"16-byte aligned")
    _refused(rf(p1=5), name, b"bad pass range [0,5) of 4")
    for m in (0, 8):
        _refused(rf(m=m), name, gate, status)
    _refused(rf(p0=2, p1=2), name, gate, status)
    assert all((a == 7.0).all() for a in (rays, hits, out, aov))


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_follow_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/follow.hip (the Makefile's flags): exactly the kernels of hj_follow.h and the one copy
    of hj_chain.h's count and scan - none of hj_aov.h's, which api/aov.hip holds -; no kernel has scratch and none spills a register: a reload inside the walk's loops would be
    a dependent memory trip per node.  LDS: the path kernels' WgShared in the walk, the scan's partial sums, a word per wave in the
    count and the scatter.  Registers and occupancy are printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert " follow " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "fl.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "follow.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_(follow|chain_scan|aov_resolve_followed|chain_count<\w+>|af_scatter<\w+>|aov_follow<\w+>)", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_af_scatter<false>", "k_af_scatter<true>", "k_aov_follow<false>", "k_aov_follow<true>", "k_aov_resolve_followed",
                             "k_chain_count<false>", "k_chain_count<true>", "k_chain_scan", "k_follow"] and len(report) == 9, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert (v["LDS Size"] > 16 * 1024) == k.startswith("k_aov_follow<") and v["LDS Size"] <= 20 * 1024, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    kernels = os.path.join(ROOT, "hijiki_amd", "csrc", "kernels")
    src, chain, segment = (open(os.path.join(kernels, f)).read() for f in ("hj_follow.h", "hj_chain.h", "hj_walk_segment.h"))
    for text in (src, chain, segment):
        assert "atomic" not in text.replace("No global atomics", "") and "asm" not in text.replace("no inline assembly", "") and "getenv" not in text
        assert "#pragma clang fp contract(off)" in text
    assert "aov_record(" in src and "HJ_DEV bool aov_record" not in src                                                       # (included, not restated)
    # the rounds' text is hj_chain.h's, once: the compaction, the continuation's call and the walk's shell are nowhere else
    assert '#include "hj_stages.h"' not in src and '#include "hj_stages.h"' not in chain and '#include "hj_chain.h"' in src
    assert "compact_scan_tiles<" in chain and "HJ_COMPACT_RANK(" in chain and "compact_scan_tiles<" not in src and "HJ_COMPACT_RANK(" not in src
    assert "chain_scatter<FIRST>(" in src and "chain_round<PAIRS>(" in src and "walk_segment<0, PAIRS>(" in chain
    assert "trace_persistent<" not in src and "trace_persistent<" not in chain and "load_hot_nodes(" not in src + chain
    assert "trace_persistent<MODE, PAIRS>(" in segment and "load_hot_nodes(sc, sh);" in segment
    assert '#include "hj_follow.h"' in chain and '#include "hj_compact.h"' in chain and "HJ_FOLLOW_NO_KERNELS" in chain and "HJ_CHAIN_NO_KERNELS" in chain
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "follow.hip")).read()


# ------------------------------------------------------------------------------------------------- the reference against itself

def _flat(material):
    """shape 0: the quad (-1, -1, 0) + s (2, 0, 0) + t (0, 2, 0) of a specular material: its stored normal is (0, 0, 1) exactly"""
    s = host.Scene()
    s.set_camera((0, 0, 5), (0, 0, 0, 1), 40.0)
    m = s.add_mirror() if material == "mirror" else s.add_dielectric(material)
    s.add_quad((-1, -1, 0), (2, 0, 0), (0, 2, 0), m)
    s.add_quad((-1, -1, -9), (2, 0, 0), (0, 2, 0), s.add_diffuse((0.5, 0.5, 0.5)))
    return s.compile()


def _at_origin(cs, d, ids=0):
    """the records of rays with directions d (n, 3) that hit shape `ids` at the origin, t = 1, normal (0, 0, 1)"""
    d = np.asarray(d, F).reshape(-1, 3)
    n = len(d)
    rays, hits, surf = np.zeros((n, 8), F), np.zeros((n, 4), F), np.zeros((n, 16), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = -d, d, R.KEPS, np.inf
    hits.view(np.int32)[:, 0] = ids
    hits[:, 1] = 1
    surf[:, 5] = 1
    return rays, hits, surf


def _unit(sin):
    """(sin, 0, -cos) towards -z, float32 (not renormalised: the continuation never normalises either)"""
    sin = np.asarray(sin, np.float64)
    return np.stack([sin, np.zeros_like(sin), -np.sqrt(1 - sin * sin)], -1).astype(F)


def test_a_mirror_reflects_about_the_stored_normal_from_both_sides():
    cs = _flat("mirror")
    front, back = _unit(0.6)[None], _unit(0.6)[None] * F(-1)
    for d in (front, back):
        out, cls = R.continue_rays(cs, *_at_origin(cs, d))
        assert cls.tolist() == [R.MIRROR]
        assert out[0, 3:6].tolist() == [d[0, 0], 0, -d[0, 2]] and out[0, 0:3].tolist() == [0, 0, 0]   # z flips, whichever side
        assert out[0, 6] == R.KEPS and out[0, 7] == np.inf
    # another material, a miss, an id outside the scene: the empty ray
    out, cls = R.continue_rays(cs, *_at_origin(cs, np.repeat(front, 4, 0), ids=[1, -1, 2, 1 << 20]))
    assert (cls == R.END).all() and not out[:, 0:6].any() and (out[:, 6] == np.inf).all() and (out[:, 7] == -np.inf).all()


def test_a_dielectric_at_normal_incidence_refracts_straight_through():
    cs = _flat(1.5)
    for d, want in ((np.array([[0, 0, -1]], F), R.REFRACT_IN), (np.array([[0, 0, 1]], F), R.REFRACT_OUT)):
        out, cls, det = R.continue_rays(cs, *_at_origin(cs, d), detail=True)
        assert cls.tolist() == [want] and det["k"][0] > 0 and det["fr"][0] < 0.05
        wo = out[0, 3:6]
        assert wo[0] == 0 and wo[1] == 0 and wo[2] * d[0, 2] > 0          # straight on, on the same side
        assert abs(abs(wo[2]) - 1) < 1e-6                                  # |par * etaInv - normal * cosO| = cosO = 1 at k = 1


def test_the_critical_angle_splits_k_and_fr_splits_the_rest():
    """From inside glass of eta 1.5 (the ray travels along +z, against the flipped normal): sin(theta_c) = 1 / 1.5.  The inputs are
    chosen by computing k and fr in the restatement, not by guessing angles: the two float32 sines nearest the critical one on
    whose sides k changes sign, and from outside the two on whose sides fr crosses 0.5f."""
    cs = _flat(1.5)
    eta = np.array([1.5], F)
    nz = np.array([[0, 0, 1]], F)

    def scan(lo, hi, inside, key):
        s = np.linspace(lo, hi, 20001)
        d = _unit(s) * F(-1 if inside else 1)
        r = R.dielectric(np.repeat(eta, len(d)), d, np.repeat(nz, len(d), 0))
        return d, r

    d, r = scan(0.60, 0.72, True, "k")
    assert r["flipped"].all()
    tir = r["k"] <= 0
    i = int(np.argmax(tir))
    assert 0 < i and not tir[:i].any() and tir[i:].all()                   # one crossing, monotone
    assert abs(float(d[i, 0]) + 1 / 1.5) < 1e-4                            # (x = -sin: the direction was mirrored through the origin)
    out, cls, det = R.continue_rays(cs, *_at_origin(cs, d[i - 1:i + 1]), detail=True)
    # just inside the critical angle k > 0 and fr, close to 1 there, already reflects; just outside k <= 0 does: two classes, one direction
    assert cls.tolist() == [R.REFLECT_FR, R.REFLECT_TIR] and det["k"][0] > 0 >= det["k"][1] and det["fr"][0] > F(0.9) and np.isnan(det["fr"][1])
    for j in (0, 1):
        assert out[j, 3:6].tolist() == [d[i - 1 + j, 0], 0, -d[i - 1 + j, 2]]   # internal reflection: z flips

    d, r = scan(0.95, 0.99999, False, "fr")
    assert not r["flipped"].any() and (r["k"] > 0).all()
    big = r["fr"] >= F(0.5)
    i = int(np.argmax(big))
    assert 0 < i and not big[:i].any() and big[i:].all()
    out, cls, det = R.continue_rays(cs, *_at_origin(cs, d[i - 1:i + 1]), detail=True)
    assert cls.tolist() == [R.REFRACT_IN, R.REFLECT_FR] and det["fr"][0] < F(0.5) <= det["fr"][1]
    assert out[1, 3:6].tolist() == [d[i, 0], 0, -d[i, 2]] and out[0, 5] < 0
    # the same from inside, below the critical angle: fr crosses 0.5 before k crosses 0
    d, r = scan(0.60, 0.6666, True, "fr")
    with np.errstate(invalid="ignore"):
        big = r["fr"] >= F(0.5)
    assert (r["k"] > 0).all() and big.any() and not big.all()
    i = int(np.argmax(big))
    out, cls = R.continue_rays(cs, *_at_origin(cs, d[i - 1:i + 1]))
    assert cls.tolist() == [R.REFRACT_OUT, R.REFLECT_FR]
    assert out[0, 5] > 0 and abs(out[0, 3]) > abs(d[i - 1, 0])             # it leaves, bent away from the normal


def test_the_refracted_direction_obeys_snell_in_float64():
    """the restatement's refract candidate against sin(theta_o) = sin(theta_i) / eta computed apart from it"""
    cs = _flat(1.5)
    s = np.linspace(0.05, 0.9, 50)
    out, cls = R.continue_rays(cs, *_at_origin(cs, _unit(s)))
    assert (cls == R.REFRACT_IN).all()
    wo = out[:, 3:6].astype(np.float64)
    assert np.abs(wo[:, 0] / np.linalg.norm(wo, axis=1) - s / 1.5).max() < 1e-6 and (wo[:, 2] < 0).all()


# ----------------------------------------------------------------------------------------------- the premise of the GPU tests

def test_every_class_occurs_among_the_query_rays_and_chains_reach_length_two(oracle):
    """From the oracle's hits: each of the five continuing classes and the end class occurs at least 16 times among the cbox query
    rays (the ray set plus the aimed ones), and the 64 x 64 two-pass frames of the GPU tests have at least 64 chains of length 1 and
    64 of length 2 at max_follow = 2.  The box's glass sphere holds a diffuse mesh (every ray refracted into it ends on one of its
    triangles), so no chain of the box's frame reaches length 2: that half of the condition is held on the "rich" scene, whose
    glass is clear - the box's frame keeps every case and the length-1 half."""
    cs = P.scene("cbox")
    rays = R.query_rays("cbox")
    hits, surf = R.oracle_trace(cs)(rays)
    _, cls = R.continue_rays(cs, rays, hits, surf)
    counts = np.bincount(cls, minlength=6)
    print({R.CLASS_NAMES[k]: int(c) for k, c in enumerate(counts)})
    assert (counts >= 16).all(), counts
    blocks = host.make_blocks(64, 64, 2, 31)
    cam = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    cam[:, 6], cam[:, 7] = R.KEPS, np.inf
    rec, length, classes = R.followed_records(cs, cam, 2, R.oracle_trace(cs))
    assert (length == 1).sum() >= 64 and (length == 2).sum() == 0, np.bincount(length)
    assert (rec[:, 3] == 1).all() and len(classes) == 2
    cs = P.scene("rich")
    cam = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    cam[:, 6], cam[:, 7] = R.KEPS, np.inf
    rec, length, classes = R.followed_records(cs, cam, 2, R.oracle_trace(cs))
    assert (length == 1).sum() >= 64 and (length == 2).sum() >= 64, np.bincount(length)
