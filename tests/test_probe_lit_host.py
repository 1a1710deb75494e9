"""hj_render_probe_lit / hj_render_probe_lit_frame, the part that needs no GPU: the symbols, the version, the struct and the contract's
key sentences; every argument refusal in the header's order without a device, with nothing written; the compiled unit's resource
report; and the reference of the GPU tests (probe_lit_ref) against float64 on a closed diffuse box under a volume whose probes carry
the constant band alone, so that E is a known constant."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import follow_ref as R
import probe_lit_ref as PL
import probe_place_ref as PP
import probe_ref as PR
import probe_vis_ref as PV
from hijiki_amd import abi, device, host
from test_abi import ROOT, declared_functions
from test_aov_host import _block, _in_order, _refused
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_render_probe_lit", "hj_render_probe_lit_frame")


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    """every test of this file is about the calls, the reference's self-check included: none passes without the symbols"""
    assert all(hasattr(device.lib(), n) and n in device.EXPORTS for n in NAMES)


def test_entry_points_struct_and_version_agree():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    v = device.lib().hj_version()
    assert v >= 0x002000 and abi.VERSION >= (0, 32, 0) and (v >> 16, (v >> 8) & 0xFF, v & 0xFF) == abi.VERSION
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    body = re.search(r"typedef struct hj_probe_lighting \{(.*?)\} hj_probe_lighting;", header, re.S).group(1)
    fields = re.findall(r"^\s*const\s+(\w+)\s*\*\s*(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in abi.ProbeLighting._fields_] == ["desc", "vis", "probes", "atlas", "placement"]
    assert [f[0] for f in fields] == ["hj_probe_desc", "hj_probe_vis_desc", "float", "float", "float"]
    assert C.sizeof(abi.ProbeLighting) == 5 * C.sizeof(C.c_void_p)
    assert "#define HJ_PROBE_LIT_WORDS 4" in header and abi.PROBE_LIT_WORDS == 4
    for text in ("Probe-lit frames (ABI 0.32)", "L[c] = Le[c] + (albedo[c] * E[c]) * 0.318309886f", "the shade stage's own 1 / pi", "so DIRECT light is in E",
                 "word 3 is the count of its samples, every one of them", "a null lighting; a placement without vis", "separately traced direct shadows",
                 "a glossy lobe", "glass extinction along the chain", "a baked light map", "multi-GPU split", "a flag of the command-line tool"):
        assert text in header, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in ("### Probe-lit frames", "k_pl_points", "k_pl_resolve", "kernels/hj_probe_lit.h", "api/probe_lit.hip", "AovStage"):
        assert text in design, text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "**Probe-lit frames**" in readme and "render_probe_lit" in readme
    assert '"hj_probe_lit.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "api/probe_lit.hip" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_internal.h")).read()
    with pytest.raises(ValueError):
        device.Renderer.render_probe_lit(None, np.zeros((2, 2, 2, 28), F), (0, 0, 0), (1, 1, 1), 4, 4, spp=1, follow=9)
    assert (device.resolve_probe_lit(np.array([[[2, 4, 6, 2], [0, 0, 0, 0]]], F)) == np.array([[[1, 2, 3], [0, 0, 0]]], F)).all()


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_come_before_the_device_in_order():
    """aov_check's refusals in its order behind the new names, max_follow (the frame form: then the pass range), a null lighting, a
    placement without vis, then the selected look-up's in that call's order, then the gate"""
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
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
            return lambda: L.hj_render_probe_lit_frame(None, w, h, 1, 5, passes[0], passes[1], mf, f, lp, img)
        return lambda: L.hj_render_probe_lit(None, blocks if blk else None, 1, w, h, mf, f, lp, img)

    head = [(b"null blocks", dict(blk=False)), (b"null aov", dict(img=None)), (b"unknown flag bits", dict(f=2)), (b"image 0 x", dict(w=0)),
            (b"original_dimension", dict(bdim=(W + 1, H))), (b"max_follow 9 above 8", dict(mf=9)), (b"null lighting", dict(light=False)),
            (b"a placement needs vis", dict(pl=Lp))]
    plain = [(b"null desc", dict(desc=False)), (b"null probes", dict(p=None)), (b"count 0 x", dict(count=(0, 2, 2))),
             (b"16-byte aligned", dict(dflags=abi.PROBES_DEVICE_ARRAYS, p=Pp + 4))]
    _in_order(make, NAMES[0], head[:-1] + plain)
    _in_order(make, NAMES[0], head)
    on = abi.PROBE_VIS_DEVICE_ARRAYS
    visible = [(b"null desc", dict(desc=False)), (b"null probes", dict(p=None)), (b"null atlas", dict(a=None)), (b"count 0 x", dict(count=(0, 2, 2))),
               (b"unknown visibility flag bits", dict(vflags=0x100)), (b"must agree", dict(dflags=abi.PROBES_DEVICE_ARRAYS)), (b"res 5", dict(res=5)),
               (b"normal_bias", dict(bias=-1.0))]
    _in_order(lambda **kw: make(vis=True, **kw), NAMES[0], head[:-1] + visible)
    _in_order(lambda **kw: make(vis=True, pl=Lp, **kw), NAMES[0], head[:-2] + visible)
    _refused(make(vis=True, dflags=abi.PROBES_DEVICE_ARRAYS, vflags=on, a=Ap + 8), NAMES[0], b"16-byte aligned")
    _refused(make(vis=True, dflags=abi.PROBES_DEVICE_ARRAYS, vflags=on, pl=Lp + 4), NAMES[0], b"16-byte aligned")
    _refused(make(vis=True, pl=Bp), NAMES[0], b"probe 5 has a non-finite offset")
    _refused(make(f=1, img=Ip + 4), NAMES[0], b"16-byte aligned")
    # the frame form: no block list; the pass range stands between max_follow and the lighting
    frame = [(b"null aov", dict(img=None)), (b"unknown flag bits", dict(f=2)), (b"image 0 x", dict(w=0)), (b"max_follow 9 above 8", dict(mf=9)),
             (b"bad pass range", dict(passes=(1, 0))), (b"null lighting", dict(light=False)), (b"null desc", dict(desc=False)), (b"null probes", dict(p=None))]
    _in_order(lambda **kw: make(frame=True, **kw), NAMES[1], frame)
    _refused(make(frame=True, passes=(0, 2)), NAMES[1], b"bad pass range [0,2) of 1")
    # what is accepted reaches the gate: host arrays of any alignment, the atlas unread with both factors off, no blocks or passes
    both_off = abi.PROBE_VIS_NO_BACKFACE | abi.PROBE_VIS_NO_CHEBYSHEV
    for name, kws in ((NAMES[0], (dict(), dict(mf=0), dict(mf=8), dict(p=Pp + 4), dict(vis=True), dict(vis=True, pl=Lp), dict(vis=True, a=None, vflags=both_off),
                                  dict(f=1), dict(vis=True, dflags=abi.PROBES_DEVICE_ARRAYS, vflags=on, pl=Lp))),
                      (NAMES[1], (dict(frame=True), dict(frame=True, passes=(1, 1), p=None), dict(frame=True, vis=True, pl=Lp)))):
        for kw in kws:
            _refused(make(**kw), name, gate, status)
    assert (image == 7.0).all()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_probe_lit_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/probe_lit.hip (the Makefile's flags): exactly k_pl_points and k_pl_resolve - no look-up
    kernel, which the probe units hold, nor a kernel of hj_aov.h or hj_follow.h -; neither has scratch, LDS or a spilled register.
    Registers and occupancy are printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert " probe_lit " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "pl.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "probe_lit.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_pl_(points|resolve)", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_pl_points", "k_pl_resolve"] and len(report) == 2, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["LDS Size"] == 0, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_probe_lit.h")).read()
    assert "atomic" not in src.replace("No global atomics", "") and "asm" not in src.replace("no inline assembly", "") and "getenv" not in src
    assert "#pragma clang fp contract(off)" in src and "aov_record(" in src and "HJ_DEV bool aov_record" not in src                # (included, not restated)
    assert "env_radiance(" in src and "k_pvv_sample(" not in src and "k_pp_sample(" not in src and "k_pv_sample(" not in src
    unit = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "probe_lit.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "hipLaunchKernelGGL(hj::k_pl_points" in unit
    assert not any(f"hj::{k}," in unit for k in ("k_pv_sample", "k_pvv_sample", "k_pp_sample"))   # (the units that hold them launch them)


# ------------------------------------------------------------------------------------------------------------ the float64 judge

def _box():
    """a closed box of six diffuse quads, each its own colour, the back wall a checkerboard, a small light in front of it; the
    camera inside"""
    s = host.Scene()
    s.set_camera((0.1, 0.2, 1.6), (0, 0, 0, 1), 110.0)
    cols = [(0.7, 0.6, 0.5), (0.6, 0.1, 0.15), (0.1, 0.55, 0.2), (0.75, 0.75, 0.7), (0.3, 0.3, 0.6)]
    m = [s.add_diffuse(c) for c in cols]
    s.add_quad((-2, -2, 2), (4, 0, 0), (0, 0, -4), m[0])                 # floor
    s.add_quad((-2, 2, 2), (0, 0, -4), (4, 0, 0), m[3])                  # ceiling
    s.add_quad((-2, -2, 2), (0, 0, -4), (0, 4, 0), m[1])                 # left
    s.add_quad((2, -2, 2), (0, 4, 0), (0, 0, -4), m[2])                  # right
    s.add_quad((-2, -2, -2), (4, 0, 0), (0, 4, 0), s.add_diffuse_cboard((0.9, 0.8, 0.2), 0.13, (0.1, 0.2, 0.8), 0.21))   # back
    s.add_quad((-2, -2, 2), (0, 4, 0), (4, 0, 0), m[4])                  # front, behind the camera
    s.add_quad((-0.4, 0.2, -1.95), (0.8, 0, 0), (0, 0.6, 0), s.add_emissive((9.0, 8.0, 6.0)))
    return s.compile()


def test_the_compose_against_float64_on_a_closed_diffuse_box(oracle):
    """Every probe carries the constant band alone, so E = c * Y_0 on every point whatever the weights are.  The coefficients are
    powers of two: coefficient * weight is then exact, the weighted sum is the coefficient times the weight sum bit for bit and the
    look-up's division returns the coefficient - what is left are the roundings of E = c * Y_0, albedo * E, * (1 / pi) with the
    constant's own rounding, + Le, and at 2 spp the sum of two samples: under eight roundings of 2^-24, so the mean is
    albedo * e / pi + Le to a relative 1e-6 on EVERY pixel.  Measured: 1.4e-07."""
    cs = _box()
    W, H, spp = 48, 40, 2
    d = PR.desc((-1.5, -1.5, -1.5), (1.0, 1.5, 0.75), (4, 3, 5))
    coef = np.array([2.0, 0.5, 1.0], F)
    vol = np.zeros((60, 28), F)
    vol[:, 0:3], vol[:, 27] = coef, 1.0
    vol[7, 27] = vol[31, 27] = 0.0                                       # (two invalid probes: the weights change, E does not)
    blocks = list(host.make_blocks(W, H, spp, 3))
    img, ch, L = PL.render(cs, blocks, W, H, 8, R.oracle_trace(cs), PL.lookup(d, vol), detail=True)
    assert (ch["kind"] == PL.DIFFUSE).all() and (ch["length"] == 0).all()                         # closed, nothing specular
    assert (img[..., 3] == spp).all()
    e = coef.astype(np.float64) * np.float64(F(0.28209479))
    want = (ch["albedo"].astype(np.float64) * e / np.pi + ch["emission"].astype(np.float64)).reshape(spp, H, W, 3).mean(0)
    assert (want > 0).all() and (ch["emission"] > 0).any() and len(np.unique(ch["albedo"], axis=0)) >= 6
    got = device.resolve_probe_lit(img).astype(np.float64)
    err = np.abs(got - want) / want
    print(f"compose against float64: max relative error {err.max():.3g} over {W * H} pixels")
    assert err.max() <= 1e-6
    # the check can fail: the compose without its 1 / pi misses on every lit pixel
    assert (np.abs(got * np.pi - want) / want).max() > 1e-2
