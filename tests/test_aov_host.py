"""hj_eval_materials, hj_render_aovs and hj_render_aovs_frame, the part that needs no GPU: the symbols, the version and the defines;
every argument refusal in the header's order without a device, with its message and with nothing written; the compiler's resource
report of the unit; the reference of the GPU tests (aov_ref) on hand-derived values; device.resolve_aovs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import aov_ref as A
from hijiki_amd import abi, device, host
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_eval_materials", "hj_render_aovs", "hj_render_aovs_frame")


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001A00
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_MATERIALS_DEVICE_ARRAYS 1u", "#define HJ_AOV_DEVICE_ARRAY 1u", "#define HJ_AOV_WORDS 12", "Frame AOVs and material queries (ABI 0.26)",
                 "starting from +0", "refused call writes nothing", "0xFFFFFFFF", "a pixel no sample covers is twelve zeros"):
        assert text in header, text
    assert (abi.MATERIALS_DEVICE_ARRAYS, abi.MATERIALS_WORDS, abi.AOV_DEVICE_ARRAY, abi.AOV_WORDS, abi.MATERIAL_MISS) == (1, 8, 1, 12, 0xFFFFFFFF)
    assert '"hj_aov.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    for fn in ("eval_materials", "render_aovs"):
        assert callable(getattr(device.Renderer, fn)) and getattr(device.Renderer, fn).__doc__
    assert callable(device.resolve_aovs)


# -------------------------------------------------------------------------------------------------------------------- refusals

def _refused(call, name, word, status=abi.HJ_ERR_INVALID):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call() == status, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and (name.encode() + b":") in text and word in text, (name, word, text)


def _in_order(make, name, order):
    """each refusal alone, then each in front of every later one: the header's order"""
    for i, (word, kw) in enumerate(order):
        _refused(make(**kw), name, word)
        for _, later in order[i + 1:]:
            if set(later) & set(kw):
                continue
            _refused(make(**dict(later, **kw)), name, word)


def _block(w, h, dim=(16, 16), origin=(0, 0)):
    b = abi.ImageBlock()
    b.dimension[:], b.original_dimension[:], b.origin[:] = dim, (w, h), origin
    return b


def test_argument_refusals_come_before_the_device_in_order():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"

    hits, surf, out = np.full((3, 4), 7.0, F), np.full((3, 16), 7.0, F), np.full((3, 8), 7.0, F)
    Hp, Sp, Op = hits.ctypes.data, surf.ctypes.data, out.ctypes.data
    assert Hp % 16 == 0 and Sp % 16 == 0 and Op % 16 == 0
    em = lambda h=Hp, s=Sp, n=3, f=0, o=Op: (lambda: L.hj_eval_materials(None, h, s, n, f, o))              # noqa: E731
    name = NAMES[0]
    _in_order(em, name, [(b"null hits", dict(h=None)), (b"unknown flag bits", dict(f=2)), (b"at most 2^31 - 1", dict(n=1 << 31)),
                         (b"16-byte aligned", dict(f=1, h=Hp + 4))])
    _refused(em(s=None), name, b"null surface")
    _refused(em(o=None), name, b"null out")
    _refused(em(f=0x80000000), name, b"unknown flag bits")
    _refused(em(f=1, s=Sp + 8), name, b"16-byte aligned")
    _refused(em(f=1, o=Op + 4), name, b"16-byte aligned")
    for f in (0, 1):
        _refused(em(f=f), name, gate, status)
    _refused(em(n=0, h=None, s=None, o=None), name, gate, status)

    W, Hh = 40, 24
    blocks = (abi.ImageBlock * 2)(_block(W, Hh), _block(W, Hh, origin=(16, 0)))
    bad_orig = (abi.ImageBlock * 2)(_block(W, Hh), _block(W, Hh + 1))
    bad_dim = (abi.ImageBlock * 2)(_block(W, Hh), _block(W, Hh, dim=(129, 1)))
    aov = np.full((Hh, W, 12), 7.0, F)
    Ap = aov.ctypes.data
    assert Ap % 16 == 0
    ra = lambda b=blocks, n=2, w=W, h=Hh, f=0, a=Ap: (lambda: L.hj_render_aovs(None, b, n, w, h, f, a))      # noqa: E731
    name = NAMES[1]
    _in_order(ra, name, [(b"null blocks", dict(b=None)), (b"unknown flag bits", dict(f=2)), (b"image 0 x", dict(w=0)),
                         (b"original_dimension", dict(b=bad_orig)), (b"16-byte aligned", dict(f=1, a=Ap + 4))])
    _refused(ra(a=None), name, b"null aov")
    _refused(ra(b=None, a=None), name, b"null blocks")
    _refused(ra(h=0), name, b"x 0")
    _refused(ra(w=16385), name, b"image 16385 x")
    _refused(ra(h=16385), name, b"x 16385")
    _refused(ra(b=bad_dim), name, b"dimension 129 x 1 above 128")
    _refused(ra(b=bad_dim, f=1, a=Ap + 8), name, b"dimension 129 x 1 above 128")
    for f in (0, 1):
        _refused(ra(f=f), name, gate, status)
    _refused(ra(b=None, n=0), name, gate, status)

    rf = lambda w=W, h=Hh, spp=4, p0=0, p1=4, f=0, a=Ap: (lambda: L.hj_render_aovs_frame(None, w, h, spp, 99, p0, p1, f, a))   # noqa: E731
    name = NAMES[2]
    _in_order(rf, name, [(b"null aov", dict(a=None)), (b"unknown flag bits", dict(f=4)), (b"image 0 x", dict(w=0)),
                         (b"bad pass range [3,2)", dict(p0=3, p1=2))])
    _refused(rf(h=16385), name, b"x 16385")
    _refused(rf(f=1, a=Ap + 4), name, b"16-byte aligned")
    _refused(rf(f=1, a=Ap + 4, p1=5), name, b"16-byte aligned")
    _refused(rf(p1=5), name, b"bad pass range [0,5) of 4")
    _refused(rf(), name, gate, status)
    _refused(rf(p0=2, p1=2), name, gate, status)
    _refused(rf(spp=0, p1=0), name, gate, status)
    assert (hits == 7.0).all() and (surf == 7.0).all() and (out == 7.0).all() and (aov == 7.0).all()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_aov_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/aov.hip (the Makefile's flags): exactly the kernels of hj_aov.h; none has scratch - the
    walk instantiation above all, a reload inside its loops would be a dependent memory trip per node -; LDS only in the walk: the
    path kernels' WgShared with the hot nodes' copy.  Registers and occupancy are printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert "-fPIC" in flags and "-ffp-contract=off" in flags and "-O3" in flags
    assert " aov " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "aov.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "aov.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_(mat_eval|aov_resolve|aov_walk<\w+>)", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_aov_resolve", "k_aov_walk<false>", "k_aov_walk<true>", "k_mat_eval"] and len(report) == 4, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert (v["LDS Size"] > 16 * 1024) == k.startswith("k_aov_walk") and v["LDS Size"] <= 20 * 1024, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_aov.h")).read()
    assert "atomic" not in src.replace("No global atomics", "") and "asm" not in src.replace("no inline assembly", "")
    assert "#pragma clang fp contract(off)" in src
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "aov.hip")).read()
    # the walk's shell is hj_walk_segment.h's; k_aov_walk does not restate it
    segment = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_walk_segment.h")).read()
    assert "__shared__ WgShared sh;" in segment and "load_hot_nodes(sc, sh);" in segment and "trace_persistent<MODE, PAIRS>(" in segment
    assert "walk_segment<0, PAIRS>(" in src and "walk_hit_record(h)" in src and "walk_empty_range(" in src
    assert "__shared__ WgShared" not in src and "load_hot_nodes(" not in src and "trace_persistent<" not in src and "hit ? h.t" not in src


# ------------------------------------------------------------------------------------------------- the reference against itself

def _material_scene():
    s = host.Scene()
    s.set_camera((0, 0, 5), (0, 0, 0, 1), 40.0)
    d = s.add_diffuse((0.25, 0.5, 0.75))
    cb = s.add_diffuse_cboard((1, 0, 0), 0.5, (0, 0, 1), 0.25)
    mi = s.add_mirror()
    gl = s.add_dielectric(1.5, (0.1, 0.2, 0.3))
    em = s.add_emissive((3, 5, 7))
    tex = np.zeros((2, 2, 3), F)
    tex[0, 0], tex[0, 1], tex[1, 0], tex[1, 1] = (1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)
    tx = s.add_diffuse_textured(s.add_texture(tex, abi.TEX_NEAREST))
    for i, m in enumerate((d, cb, mi, gl, em, tx)):
        s.add_sphere((3 * i, 0, 0), 1.0, m)
    return s.compile()


def test_materials_gives_hand_derived_values():
    cs = _material_scene()
    tags = (cs.materials >> abi.MATERIAL_TAG_SHIFT).tolist()
    assert tags == [abi.MAT_DIFFUSE, abi.MAT_DIFFUSECBOARD, abi.MAT_MIRROR, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE, abi.MAT_DIFFUSE_TEXTURED]
    # the checkerboard: fu = frac(0.5 u / 0.5) = frac(u), fv = frac(0.5 v / 0.25) = frac(2 v); colour b (0, 0, 1) when (fu < .5) != (fv < .5)
    #   (0.25, 0.1):  fu .25 <, fv .2 <   -> a      (0.5, 0.1):   fu .5 not <, fv <  -> b   (the boundary at 0.5 belongs to the upper cell)
    #   (0.49999997, 0.1): fu < .5        -> a      (0.25, 0.25): fv .5 not <        -> b
    #   (-0.25, 0.1): fu = -0.25 - floor(-0.25) = 0.75 not <, fv <  -> b             (-0.75, 0.1): fu 0.25 < -> a
    cases = [(0.25, 0.1, "a"), (0.5, 0.1, "b"), (np.nextafter(F(0.5), F(0)), 0.1, "a"), (0.25, 0.25, "b"), (0.25, np.nextafter(F(0.25), F(0)), "a"),
             (-0.25, 0.1, "b"), (-0.75, 0.1, "a"), (0.75, 0.3, "a")]
    u, v = np.array([c[0] for c in cases], F), np.array([c[1] for c in cases], F)
    got = A.materials(cs, cs.textures, np.full(len(cases), 1), u, v)
    colour = {"a": [1.0, 0.0, 0.0], "b": [0.0, 0.0, 1.0]}
    for row, c in zip(got, cases):
        assert row[0:3].tolist() == colour[c[2]] and row[4:8].tolist() == [0, 0, 0, 0], (c, row)
    assert (got.view(U)[:, 3] == (abi.MAT_DIFFUSECBOARD << 24) | 0).all()
    # one row per other tag, and the misses
    ids = np.array([0, 2, 3, 4, 5, 5, -1, 6, 1 << 20], np.int32)
    u, v = np.array([0.3, 0.3, 0.3, 0.3, 0.25, 0.75, 0.3, 0.3, 0.3], F), np.array([0.6, 0.6, 0.6, 0.6, 0.75, 0.25, 0.6, 0.6, 0.6], F)
    got = A.materials(cs, cs.textures, ids, u, v)
    assert got[0].tolist() == [0.25, 0.5, 0.75, got[0, 3], 0, 0, 0, 0] and got.view(U)[0, 3] == cs.materials[0]
    assert got[1].tolist()[:3] == [1, 1, 1] and got[1].tolist()[4:] == [0, 0, 0, 0] and got.view(U)[1, 3] >> 24 == abi.MAT_MIRROR
    assert got[2].tolist()[:3] == [1, 1, 1] and got[2].tolist()[4:] == [0, 0, 0, 0] and got.view(U)[2, 3] >> 24 == abi.MAT_DIELECTRIC
    assert got[3].tolist()[:3] == [0, 0, 0] and got[3].tolist()[4:] == [3, 5, 7, 0] and got.view(U)[3, 3] >> 24 == abi.MAT_EMISSIVE
    # the 2 x 2 texture, nearest: (u .25, v .75) is the left column of the TOP row, (u .75, v .25) the right column of the bottom row
    assert got[4].tolist()[:3] == [1, 2, 3] and got[5].tolist()[:3] == [10, 11, 12] and got.view(U)[4, 3] == (abi.MAT_DIFFUSE_TEXTURED << 24)
    for row in got[6:]:
        assert row.view(U).tolist() == [0, 0, 0, 0xFFFFFFFF, 0, 0, 0, 0]


def test_accumulate_sums_in_block_order_where_float32_addition_does_not_commute():
    W, H = 6, 4
    b1, b2, b3 = _block(W, H, (2, 2), (1, 1)), _block(W, H, (3, 2), (3, 0)), _block(W, H, (2, 2), (1, 1))
    # block 3 repeats block 1's rectangle: pixel (1, 1) gets record 0, then record 10.  Word 1: 2^24 + 1 = 2^24 in float32 (a tie,
    # to even); word 2: -2^24 + 1 = -(2^24 - 1), exact
    rec = np.zeros((4 + 6 + 4, 12), F)
    rec[:, 3] = 1
    rec[0, 1], rec[10, 1] = 2.0 ** 24, 1.0
    rec[0, 2], rec[10, 2] = -(2.0 ** 24), 1.0
    rec[4:10, 4] = np.arange(6)
    out = A.accumulate(W, H, [b1, b2, b3], rec)
    assert out.dtype == F and out.shape == (H, W, 12)
    assert out[1, 1, 3] == 2 and out[2, 2, 3] == 2 and out[0, 3, 3] == 1 and out[0, 0].tolist() == [0] * 12 and out[3, 5].tolist() == [0] * 12
    assert out[0, 3:6, 4].tolist() == [0, 1, 2] and out[1, 3:6, 4].tolist() == [3, 4, 5]
    assert out[1, 1, 1] == F(2.0 ** 24) and out[1, 1, 2] == F(-(2.0 ** 24) + 1)
    # three samples on one pixel, in an order where float32 addition does not commute: (2^24 + 1) + -2^24 = 0, (2^24 + -2^24) + 1 = 1
    one = _block(W, H, (1, 1), (0, 0))
    r3 = np.zeros((3, 12), F)
    r3[:, 0] = [2.0 ** 24, 1.0, -(2.0 ** 24)]
    assert A.accumulate(W, H, [one, one, one], r3)[0, 0, 0] == 0.0
    assert A.accumulate(W, H, [one, one, one], r3[[0, 2, 1]])[0, 0, 0] == 1.0
    # a block that reaches over the image's edge loses the samples outside
    edge = _block(W, H, (2, 2), (5, 3))
    r4 = np.ones((4, 12), F)
    out = A.accumulate(W, H, [edge], r4)
    assert out[3, 5, 3] == 1 and out[..., 3].sum() == 1


def test_sample_records_from_hit_and_surface_records():
    cs = _material_scene()
    b = _block(8, 8, (2, 1))
    hits = np.zeros((2, 4), F)
    hits.view(np.int32)[:, 0] = [4, -1]
    hits[0, 1:4] = [2.5, 0.1, 0.2]
    surf = np.zeros((2, 16), F)
    surf[0, 3:6], surf[0, 6:8] = [0, 0.6, 0.8], [0.3, 0.4]
    surf[1, 3:6] = [9, 9, 9]                                           # (a miss takes nothing from its records)
    rec = A.sample_records(cs, [b], hits, surf)
    assert rec[0].tolist() == [0, 0, 0, 1, 0, F(0.6), F(0.8), 2.5, 3, 5, 7, 1]
    assert rec[1].tolist() == [0, 0, 0, 1] + [0] * 8


def test_resolve_aovs_divides_by_the_right_counts():
    a = np.zeros((2, 2, 12), F)
    a[0, 0] = [2, 4, 6, 4, 0, 0, 3, 9, 1, 2, 3, 3]                      # 4 samples, 3 hits
    a[0, 1, 3] = 2                                                      # 2 samples, no hit
    r = device.resolve_aovs(a)
    assert set(r) == {"albedo", "normal", "depth", "emission", "coverage"}
    assert r["albedo"].shape == (2, 2, 3) and r["depth"].shape == (2, 2) and all(x.dtype == F for x in r.values())
    assert r["albedo"][0, 0].tolist() == [0.5, 1.0, 1.5] and r["emission"][0, 0].tolist() == [0.25, 0.5, 0.75]
    assert r["normal"][0, 0].tolist() == [0, 0, 1] and r["depth"][0, 0] == 3 and r["coverage"][0, 0] == 0.75
    assert r["depth"][0, 1] == 0 and r["coverage"][0, 1] == 0 and r["normal"][0, 1].tolist() == [0, 0, 0]
    for k, x in r.items():
        assert np.isfinite(x).all() and not x[1].any(), k               # count 0 -> 0, never NaN
