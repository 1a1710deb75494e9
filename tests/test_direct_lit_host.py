"""hj_render_direct_lit / hj_render_direct_lit_frame, HJ_GATHER_INDIRECT and HJ_PROBES_INDIRECT_ONLY, the part that needs no GPU: the
symbols, the version and the contract's key sentences, the two reserved bits among them; every argument refusal of the two frame calls
in hj_render_probe_lit's order, a null lighting accepted; the new flag bits accepted by every call that reads them and the reserved ones
still refused; the compiled unit's resource report; and the reference of the GPU tests (direct_lit_ref) on the oracle alone - against
path_query_ref.compose sample for sample, and the indirect gather against the full one per point."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import direct_lit_ref as DL
import follow_ref as R
import gather_ref as G
import path_query_ref as P
import probe_place_ref as PP
import probe_ref as PR
import probe_update_ref as PU
import probe_vis_ref as PV
from hijiki_amd import abi, device, host
from test_abi import ROOT, declared_functions
from test_aov_host import _block, _in_order, _refused
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_render_direct_lit", "hj_render_direct_lit_frame")


def _gate():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    return status, (b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context")


def test_entry_points_flags_and_version_agree():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    v = device.lib().hj_version()
    assert v >= 0x002100 and abi.VERSION >= (0, 33, 0) and (v >> 16, (v >> 8) & 0xFF, v & 0xFF) == abi.VERSION
    assert (abi.GATHER_INDIRECT, abi.PROBES_INDIRECT_ONLY) == (16, 4)
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_GATHER_INDIRECT 16u", "#define HJ_PROBES_INDIRECT_ONLY 4u", "Direct-lit frames (ABI 0.33)",
                 "Bit 8u is reserved and stays\n *     refused as an unknown flag bit", "Bit 2u is reserved and stays refused as an unknown flag bit",
                 "A path starts with wasDiscrete clear", "a first segment that ends on an emitter adds nothing and ends", "a first segment that leaves\n *     into an uploaded environment adds nothing",
                 "D = ((albedo * dot(n, sdir)) * 0.318309886f) * imp", "tMin = 2 eps and tMax = stmax", "L = Lp + D, one rounding a channel",
                 "bit for bit the radiance hj_trace_paths", "max_bounces = 1", "with a plain volume it has it twice", "does not and cannot check this",
                 "a null lighting is accepted", "the light-shaft grid's proven-free shortcut", "(For those: hj_render_direct_lit, below",
                 # hj_render_probe_lit's block keeps its sentences
                 "so DIRECT light is in E", "separately traced direct shadows - direct light is as soft as the volume has it"):
        assert text in header, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in ("### Direct-lit frames", "k_dl_sample", "k_dl_shadow", "k_dl_resolve", "kernels/hj_direct_lit.h", "api/direct_lit.hip"):
        assert text in design, text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "**Direct-lit frames**" in readme and "render_direct_lit" in readme
    assert '"hj_direct_lit.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "api/direct_lit.hip" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_internal.h")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "direct_lit_cost.py"))
    sig = inspect.signature(device.Renderer.render_direct_lit).parameters
    assert list(sig)[1:6] == ["width", "height", "volume", "origin", "spacing"] and sig["volume"].default is None and sig["blocks"].default is None
    for fn, kw in (("bake_probes", "indirect_only"), ("update_probes", "indirect_only"), ("place_probes", "indirect_only"), ("trace_irradiance", "indirect"),
                   ("trace_irradiance_adaptive", "indirect")):
        assert inspect.signature(getattr(device.Renderer, fn)).parameters[kw].default is False
    with pytest.raises(ValueError):
        device.Renderer.render_direct_lit(None, 4, 4, spp=1, follow=9)
    with pytest.raises(ValueError):
        device.Renderer.render_direct_lit(None, 4, 4)
    d = device.Renderer._probe_desc("x", (0, 0, 0), (1, 1, 1), (2, 2, 2), device=True, indirect_only=True)
    assert d.flags == abi.PROBES_DEVICE_ARRAYS | abi.PROBES_INDIRECT_ONLY


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_come_before_the_device_in_order():
    """test_probe_lit_host's table under the new names; the one change: a null lighting reaches the gate"""
    L = device.lib()
    status, gate = _gate()
    W, H = 6, 5
    image = np.full((H, W, 4), 7.0, F)
    probes, atlas, place = np.full((8, 28), 1.0, F), np.full((8, 6, 6, 2), 1.0, F), PP.zeros(8)
    bad_place = place.copy()
    bad_place[5, 1] = np.inf
    Ip, Pp, Ap, Lp, Bp = (a.ctypes.data for a in (image, probes, atlas, place, bad_place))
    assert all(p % 16 == 0 for p in (Ip, Pp, Ap, Lp))
    keep = []

    def make(frame=False, blk=True, img=Ip, f=0, w=W, h=H, bdim=None, mf=2, passes=(0, 1), light=True, desc=True, count=(2, 2, 2), dflags=0, vis=False,
             vflags=0, res=4, bias=0.0, p=Pp, a=Ap, pl=None):
        d = PR.abi_desc(count=count, flags=dflags)
        v = PV.abi_vis(res=res, normal_bias=bias, flags=vflags)
        lighting = abi.ProbeLighting(C.pointer(d) if desc else None, C.pointer(v) if vis else None, p, a, pl)
        blocks = (abi.ImageBlock * 1)(_block(*(bdim or (W, H))))
        keep.append((d, v, lighting, blocks))
        lp = C.byref(lighting) if light else None
        if frame:
            return lambda: L.hj_render_direct_lit_frame(None, w, h, 1, 5, passes[0], passes[1], mf, f, lp, img)
        return lambda: L.hj_render_direct_lit(None, blocks if blk else None, 1, w, h, mf, f, lp, img)

    head = [(b"null blocks", dict(blk=False)), (b"null aov", dict(img=None)), (b"unknown flag bits", dict(f=2)), (b"image 0 x", dict(w=0)),
            (b"original_dimension", dict(bdim=(W + 1, H))), (b"max_follow 9 above 8", dict(mf=9)), (b"a placement needs vis", dict(pl=Lp))]
    plain = [(b"null desc", dict(desc=False)), (b"null probes", dict(p=None)), (b"count 0 x", dict(count=(0, 2, 2))),
             (b"16-byte aligned", dict(dflags=abi.PROBES_DEVICE_ARRAYS, p=Pp + 4))]
    _in_order(make, NAMES[0], head[:-1] + plain)
    _in_order(make, NAMES[0], head)
    on = abi.PROBE_VIS_DEVICE_ARRAYS
    visible = [(b"null desc", dict(desc=False)), (b"null probes", dict(p=None)), (b"null atlas", dict(a=None)), (b"count 0 x", dict(count=(0, 2, 2))),
               (b"unknown visibility flag bits", dict(vflags=0x100)), (b"must agree", dict(dflags=abi.PROBES_DEVICE_ARRAYS)), (b"res 5", dict(res=5)),
               (b"normal_bias", dict(bias=-1.0))]
    _in_order(lambda **kw: make(vis=True, **kw), NAMES[0], head[:-1] + visible)
    _in_order(lambda **kw: make(vis=True, pl=Lp, **kw), NAMES[0], head[:-1] + visible)
    _refused(make(vis=True, dflags=abi.PROBES_DEVICE_ARRAYS, vflags=on, a=Ap + 8), NAMES[0], b"16-byte aligned")
    _refused(make(vis=True, dflags=abi.PROBES_DEVICE_ARRAYS, vflags=on, pl=Lp + 4), NAMES[0], b"16-byte aligned")
    _refused(make(vis=True, pl=Bp), NAMES[0], b"probe 5 has a non-finite offset")
    _refused(make(f=1, img=Ip + 4), NAMES[0], b"16-byte aligned")
    _refused(make(dflags=2), NAMES[0], b"unknown flag bits 0x2")                                   # (the reserved desc bit)
    # a null lighting: the refusals in front of it stand, nothing of a volume is checked behind it
    _in_order(lambda **kw: make(light=False, **kw), NAMES[0], head[:-1])
    frame = [(b"null aov", dict(img=None)), (b"unknown flag bits", dict(f=2)), (b"image 0 x", dict(w=0)), (b"max_follow 9 above 8", dict(mf=9)),
             (b"bad pass range", dict(passes=(1, 0))), (b"null desc", dict(desc=False)), (b"null probes", dict(p=None))]
    _in_order(lambda **kw: make(frame=True, **kw), NAMES[1], frame)
    _in_order(lambda **kw: make(frame=True, light=False, **kw), NAMES[1], frame[:-2])
    _refused(make(frame=True, passes=(0, 2)), NAMES[1], b"bad pass range [0,2) of 1")
    both_off = abi.PROBE_VIS_NO_BACKFACE | abi.PROBE_VIS_NO_CHEBYSHEV
    for name, kws in ((NAMES[0], (dict(), dict(mf=0), dict(mf=8), dict(p=Pp + 4), dict(vis=True), dict(vis=True, pl=Lp), dict(vis=True, a=None, vflags=both_off),
                                  dict(f=1), dict(vis=True, dflags=abi.PROBES_DEVICE_ARRAYS, vflags=on, pl=Lp), dict(light=False), dict(light=False, mf=0),
                                  dict(light=False, f=1), dict(light=False, desc=False, p=None, a=None), dict(dflags=abi.PROBES_INDIRECT_ONLY))),
                      (NAMES[1], (dict(frame=True), dict(frame=True, passes=(1, 1), p=None), dict(frame=True, vis=True, pl=Lp), dict(frame=True, light=False),
                                  dict(frame=True, light=False, passes=(1, 1))))):
        for kw in kws:
            _refused(make(**kw), name, gate, status)
    assert (image == 7.0).all()


def test_the_gathers_accept_16_and_still_refuse_8():
    L = device.lib()
    status, gate = _gate()
    pts, out = np.zeros((4, 8), F), np.full((4, 36), 7.0, F)
    pts[:, 4] = 1.0
    a = abi.AdaptiveOpts(4, 4, 16, 0.05, 0.01)
    fixed = lambda f: (lambda: L.hj_trace_irradiance(None, pts.ctypes.data, 4, 1, None, f, out.ctypes.data, None))                    # noqa: E731
    for f in (16, 16 | 2, 16 | 2 | 4, 16 | 1):
        _refused(fixed(f), "hj_trace_irradiance", gate, status)
    for f in (8, 16 | 8, 0x80000007, 32):
        _refused(fixed(f), "hj_trace_irradiance", b"unknown flag bits")
    _refused(fixed(16 | 4), "hj_trace_irradiance", b"HJ_GATHER_SH9 only together with HJ_GATHER_SPHERE")
    adaptive = lambda f: (lambda: L.hj_trace_irradiance_adaptive(None, pts.ctypes.data, 4, C.byref(a), None, f, out.ctypes.data, None, None))   # noqa: E731
    for f in (16, 16 | 2, 16 | 1):
        _refused(adaptive(f), "hj_trace_irradiance_adaptive", gate, status)
    for f in (8, 16 | 8, 0x80000007):
        _refused(adaptive(f), "hj_trace_irradiance_adaptive", b"unknown flag")
    _refused(adaptive(16 | 2 | 4), "hj_trace_irradiance_adaptive", b"HJ_GATHER_SH9 is not available")
    assert (out == 7.0).all()


def test_every_desc_reader_accepts_4_and_still_refuses_2():
    L = device.lib()
    status, gate = _gate()
    vol, atlas, place = np.full((8, 28), 1.0, F), np.full((8, 6, 6, 2), 1.0, F), PP.zeros(8)
    pts, out4, rays, field, image = np.ones((3, 8), F), np.zeros((3, 4), F), np.zeros((8 * 16 * 4, 8), F), np.zeros(8, F), np.zeros((5, 6, 4), F)
    p = lambda x: x.ctypes.data                                                                # noqa: E731
    v, u, pl = PV.abi_vis(res=4), PU.abi_update(), PP.abi_place()
    blocks = (abi.ImageBlock * 1)(_block(6, 5))
    ref = C.byref

    def calls(d):
        lighting = abi.ProbeLighting(C.pointer(d), None, p(vol), None, None)
        return {
            "hj_probe_points": lambda: L.hj_probe_points(None, ref(d), p(pts)),
            "hj_bake_probes": lambda: L.hj_bake_probes(None, ref(d), 1, None, p(vol), None),
            "hj_sample_probes": lambda: L.hj_sample_probes(None, ref(d), p(vol), p(pts), 3, p(out4)),
            "hj_probe_visibility_rays": lambda: L.hj_probe_visibility_rays(None, ref(d), ref(v), 0, 8, p(rays)),
            "hj_bake_probe_visibility": lambda: L.hj_bake_probe_visibility(None, ref(d), ref(v), p(atlas)),
            "hj_sample_probes_visible": lambda: L.hj_sample_probes_visible(None, ref(d), ref(v), p(vol), p(atlas), p(pts), 3, p(out4)),
            "hj_update_probes": lambda: L.hj_update_probes(None, ref(d), ref(u), 1, None, p(vol), None),
            "hj_update_probe_visibility": lambda: L.hj_update_probe_visibility(None, ref(d), ref(v), ref(u), p(atlas)),
            "hj_place_probes": lambda: L.hj_place_probes(None, ref(d), ref(v), ref(pl), p(place)),
            "hj_update_probes_placed": lambda: L.hj_update_probes_placed(None, ref(d), ref(u), 1, None, p(place), p(vol), None),
            "hj_update_probe_visibility_placed": lambda: L.hj_update_probe_visibility_placed(None, ref(d), ref(v), ref(u), p(place), p(atlas)),
            "hj_sample_probes_visible_placed": lambda: L.hj_sample_probes_visible_placed(None, ref(d), ref(v), p(vol), p(atlas), p(pts), 3, p(place), p(out4)),
            "hj_distance_field": lambda: L.hj_distance_field(None, ref(d), 1.0, 0, p(field)),
            "hj_render_probe_lit": lambda: L.hj_render_probe_lit(None, blocks, 1, 6, 5, 0, 0, ref(lighting), p(image)),
            "hj_render_direct_lit": lambda: L.hj_render_direct_lit(None, blocks, 1, 6, 5, 0, 0, ref(lighting), p(image)),
        }
    for name, call in calls(PR.abi_desc(flags=abi.PROBES_INDIRECT_ONLY)).items():
        _refused(call, name, gate, status)
    for flags in (2, 4 | 2, 8):
        for name, call in calls(PR.abi_desc(flags=flags)).items():
            _refused(call, name, b"unknown flag bits")
    assert not image.any() and not field.any() and (vol == 1.0).all()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_direct_lit_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/direct_lit.hip (the Makefile's flags): exactly the new kernels - k_dl_sample in its two
    instantiations, the three compaction kernels, k_dl_shadow in its two, k_dl_resolve - and no kernel of hj_probe_lit.h, hj_follow.h or
    hj_aov.h.  The three flat kernels (sample, resolve; count, scan, scatter with them) have no scratch and no spilled register; the
    walk's figures are printed, as every figure is."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert " direct_lit " in var("HIP_UNITS") + " " and "probe_lit_volume.h" in var("HIP_HDR")
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "dl.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "direct_lit.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    kinds = sorted(re.search(r"k_dl_[a-z]+", k).group(0) for k in report)
    assert kinds == ["k_dl_count", "k_dl_resolve", "k_dl_sample", "k_dl_sample", "k_dl_scan", "k_dl_scatter", "k_dl_shadow", "k_dl_shadow"], sorted(report)
    for k, v in report.items():
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, scratch {v['ScratchSize']}, LDS {v['LDS Size']}, occupancy {v['Occupancy']} waves per SIMD")
        if "k_dl_shadow" not in k:
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        if "k_dl_sample" in k or "k_dl_resolve" in k:
            assert v["LDS Size"] == 0, (k, v)
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_direct_lit.h")).read()
    assert "atomic" not in src.replace("No global atomics", "") and "asm" not in src.replace("no inline assembly", "") and "getenv" not in src
    assert "#pragma clang fp contract(off)" in src and "sample_emitter<ENV>(" in src and "pl_compose(" in src and "pl_segment(" in src
    assert "HJ_DEV v3 sample_emitter" not in src and "shadow_ray_proven_free" not in src
    unit = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "direct_lit.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "hj::k_pl_points" not in unit and "hj::k_pl_resolve" not in unit


# ------------------------------------------------------------------------------------------- the reference, on the oracle alone

@pytest.mark.parametrize("name", ["cbox", "rich", "env"])
def test_without_a_volume_a_sample_is_the_path_query_at_one_bounce(oracle, name):
    """max_follow = 0, no volume: sample for sample and bit for bit path_query_ref.compose(spp = 1, max_bounces = 1) of the camera rays
    under the samples' seeds - the shade stage takes the first hit's next-event sample before its bounce limit ends the path.  Ties the
    new contract to the oracle-pinned integrator."""
    cs = P.scene(name)
    W = H = 24
    blocks = []
    for k, (ox, oy) in enumerate([(0, 0), (12, 0), (0, 12), (12, 12)]):
        b = abi.ImageBlock()
        b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:], b.sample_offset[:] = k, 4242 + 977 * k, (ox, oy), (12, 12), (W, H), (0.25, 0.75)
        blocks.append(b)
    from oracle import hj_oracle as oracle_mod
    env = (lambda d: oracle_mod.env_lookup(cs, d)) if name == "env" else None
    rays = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    want, counts, detail = P.compose(cs, rays, 1, P.options(1, grid=False), detail=True)
    img, det = DL.render(cs, blocks, W, H, 0, R.oracle_trace(cs), DL.oracle_occluded(cs), None, env, detail=True)
    assert (det["L"].view(U) == want[:, 0:3].view(U)).all(), int((det["L"].view(U) != want[:, 0:3].view(U)).sum())
    assert det["wants"].sum() == counts["shadow_rays"] and det["counts"].sum() == counts["unoccluded_shadow_rays"]
    print(f"{name}: {int(det['wants'].sum())} of {len(rays)} samples want a shadow ray, {int(det['counts'].sum())} count")
    assert det["counts"].sum() > 20 and (det["wants"] & ~det["counts"]).sum() > 0 and (img[..., 3] == 1).all()
    # at max_bounces = 2 the integrator has gone on: the check can fail
    assert (P.compose(cs, rays, 1, P.options(2, grid=False))[0][:, 0:3].view(U) != want[:, 0:3].view(U)).any()


@pytest.mark.parametrize("name", ["cbox", "rich", "env"])
def test_the_indirect_gather_against_the_full_one(oracle, name):
    """per point at spp = 1: the records are equal unless the first segment ended on an emitter or left into the environment; there the
    indirect radiance is exactly 0 and the full one that emission or environment radiance; hit count and nearest t never differ"""
    cs = P.scene(name)
    pts = G.point_set(name)[::3]
    o = P.options(6)
    full, _, Lf, idf = DL.gather(cs, pts, 1, False, False, o, discrete=1, detail=True)
    ind, _, Li, idi = DL.gather_indirect(cs, pts, 1, False, False, o, detail=True)
    ref, _ = G.gather(cs, pts, 1, False, False, o)
    assert (full.view(U) == ref.view(U)).all()                           # discrete = 1 IS gather_ref.gather
    assert (idf == idi).all() and (full[:, 3:8].view(U) == ind[:, 3:8].view(U)).all()
    first = idf[:, 0]
    tags = np.where(first >= 0, cs.materials[np.maximum(first, 0)] >> abi.MATERIAL_TAG_SHIFT, 0xFF)
    direct = (tags == abi.MAT_EMISSIVE) | ((first < 0) & (name == "env"))
    same = (full[:, 0:3].view(U) == ind[:, 0:3].view(U)).all(1)
    assert same[~direct].all()
    assert not ind[direct, 0:3].any() and (ind[direct, 0:3].view(U) == 0).all()
    lit = direct & full[:, 0:3].any(1)
    print(f"{name}: {int(direct.sum())} of {len(pts)} first segments end on an emitter or in the environment, {int(lit.sum())} of them carry light")
    assert lit.sum() >= 3 and (~direct).sum() > 50
