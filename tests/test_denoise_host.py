"""hj_denoise_frame, the part that needs no GPU: the symbol, the version, the defines and the contract's key sentences; every argument
refusal in the header's order without a device, with its message and with nothing written; the compiler's resource report of the
unit; the reference of the GPU tests (denoise_ref) on hand-derived values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as D
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_aov_host import _in_order, _refused
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAME = "hj_denoise_frame"


def test_entry_point_is_declared_listed_and_exported():
    assert NAME in declared_functions("hijiki_hip.h") and NAME in device.EXPORTS and hasattr(device.lib(), NAME)
    assert device.lib().hj_version() >= 0x001B00
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_DENOISE_DEVICE_ARRAYS 1u", "#define HJ_DENOISE_MAX_ITERATIONS 8u", "hj_denoise_frame (ABI 0.27)",
                 "A_ch = fmaxf(aov[ch] / S, 0.015625f)", "a pixel is LIT when aov[8], aov[9] or aov[10] is above 0",
                 "no in-image pixel of the 5 x 5", "a tie takes the forward one", "V = fmaxf(m2 / cnt - mu * mu, 0.0f)",
                 "at step 1 WHATEVER s is", "w = h * hj_exp(-(((en + ez) + el) + ea))", "V' = vs / (ws * ws)", "no scene is needed: this call traces nothing",
                 "The framebuffer is read, never written", "A refused call writes nothing", "they are not tuned", "HJ_DENOISE_LDS_STEP"):
        assert text in header, text
    assert "a denoiser. */" not in header                                # (the AOV section's "Not here" list no longer names it)
    assert (abi.DENOISE_DEVICE_ARRAYS, abi.DENOISE_MAX_ITERATIONS) == (1, 8)
    assert C.sizeof(abi.DenoiseOpts) == 24 and [f[0] for f in abi.DenoiseOpts._fields_] == ["iterations", "sigma_normal", "sigma_depth", "sigma_luminance",
                                                                                          "sigma_albedo", "flags"]
    assert '"hj_denoise.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert '"HJ_DENOISE_LDS_STEP"' in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_tuning.h")).read()
    assert callable(device.Renderer.denoise_frame) and device.Renderer.denoise_frame.__doc__


@pytest.fixture(autouse=True)
def _the_library_has_the_call():
    """every test of this file is about hj_denoise_frame, the reference's self-checks included: none passes without the symbol"""
    assert hasattr(device.lib(), NAME) and NAME in device.EXPORTS


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_argument_refusals_come_before_the_device_in_order():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
    W, H = 6, 5
    beauty, aov, out = np.full((H, W, 4), 7.0, F), np.full((H, W, 12), 7.0, F), np.full((H, W, 4), 7.0, F)
    Bp, Ap, Op = beauty.ctypes.data, aov.ctypes.data, out.ctypes.data
    assert Bp % 16 == 0 and Ap % 16 == 0 and Op % 16 == 0

    def make(o=True, it=5, sn=0.5, sz=1.0, sl=4.0, sa=0.1, f=0, w=W, h=H, b=Bp, a=Ap, out=Op):
        opts = abi.DenoiseOpts(it, sn, sz, sl, sa, f)
        return lambda: L.hj_denoise_frame(None, w, h, b, a, C.byref(opts) if o else None, out)

    _in_order(make, NAME, [(b"null opts", dict(o=False)), (b"unknown flag bits", dict(f=2)), (b"9 iterations, at most 8", dict(it=9)),
                           (b"sigma_depth -1", dict(sz=-1.0)), (b"image 0 x", dict(w=0)), (b"16-byte aligned", dict(f=1, a=Ap + 4))])
    _refused(make(a=None), NAME, b"null aov")
    _refused(make(out=None), NAME, b"null out")
    _refused(make(o=False, a=None, out=None), NAME, b"null opts")
    _refused(make(a=None, out=None), NAME, b"null aov")
    _refused(make(f=0x80000000), NAME, b"unknown flag bits")
    for kw, word in ((dict(sn=float("nan")), b"sigma_normal"), (dict(sz=float("inf")), b"sigma_depth"), (dict(sl=-0.5), b"sigma_luminance"),
                     (dict(sa=float("-inf")), b"sigma_albedo"), (dict(sn=-1.0, sa=-1.0), b"sigma_normal")):
        _refused(make(**kw), NAME, word)
    _refused(make(h=0), NAME, b"x 0")
    _refused(make(w=16385), NAME, b"image 16385 x")
    _refused(make(h=16385), NAME, b"x 16385")
    _refused(make(f=1, b=Bp + 8), NAME, b"16-byte aligned")
    _refused(make(f=1, out=Op + 4), NAME, b"16-byte aligned")
    _refused(make(b=Bp + 4), NAME, gate, status)                        # (host arrays need no alignment)
    for kw in (dict(), dict(f=1), dict(b=None), dict(f=1, b=None), dict(it=0), dict(it=8, sn=0.0, sz=0.0, sl=0.0, sa=0.0)):
        _refused(make(**kw), NAME, gate, status)
    assert (beauty == 7.0).all() and (aov == 7.0).all() and (out == 7.0).all()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_denoise_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/denoise.hip (the Makefile's flags): exactly the kernels of hj_denoise.h; none has scratch;
    LDS in the lattice form - 36 x 12 cells of 48 bytes - and, a word a cell for the lit flags, in the prepare kernel.  Registers and occupancy are printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert "-fPIC" in flags and "-ffp-contract=off" in flags and "-O3" in flags and "-fhip-fp32-correctly-rounded-divide-sqrt" in flags
    assert " denoise " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "denoise.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "denoise.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_dn_\w+", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_dn_filter_direct", "k_dn_filter_lds", "k_dn_finish", "k_dn_prepare", "k_dn_variance"] and len(report) == 5, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] == {"k_dn_filter_lds": 36 * 12 * 48, "k_dn_prepare": 36 * 12 * 4}.get(k, 0), (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_denoise.h")).read()
    assert "atomic" not in src.replace("no global atomic", "") and "asm" not in src.replace("inline assembly", "")
    assert "#pragma clang fp contract(off)" in src and "getenv" not in src
    host = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "denoise.hip")).read()
    assert "#pragma clang fp contract(off)" in host and "getenv" not in host


# ------------------------------------------------------------------------------------------------- the reference against itself

def _pixel(c, albedo, n=(0, 0, 1), z=2.0, samples=4, hits=4, bw=2.0):
    """one pixel's (beauty, aov) with the mean colour c, mean albedo `albedo`, mean normal n and mean depth z"""
    b = np.array([c[0] * bw, c[1] * bw, c[2] * bw, bw], F)
    a = np.zeros(12, F)
    a[0:3], a[3] = np.array(albedo, F) * F(samples), samples
    a[4:7], a[7], a[11] = np.array(n, F) * F(hits), F(z) * F(hits), hits
    return b, a


def _image(rows):
    """rows of _pixel results -> beauty (H, W, 4), aov (H, W, 12)"""
    return (np.array([[p[0] for p in row] for row in rows], F), np.array([[p[1] for p in row] for row in rows], F))


def test_a_single_guided_pixel_is_the_round_trip_with_variance_zero():
    beauty, aov = _image([[_pixel((1, 2, 3), (0.5, 0.25, 0.75))]])
    G, c, A, I, n, z = D.prepare(beauty, aov)
    assert G.all() and c[0, 0].tolist() == [1, 2, 3] and A[0, 0].tolist() == [0.5, 0.25, 0.75] and I[0, 0].tolist() == [2, 8, 4]
    assert n[0, 0].tolist() == [0, 0, 1] and z[0, 0] == 2
    for it in (0, 1, 5, 8):
        out = D.run(beauty, aov, it)
        assert out.dtype == F and out.shape == (1, 1, 4) and out[0, 0].tolist() == [1, 2, 3, 0], (it, out)
    # an albedo below the floor (and one of exactly 0) is floored at 1 / 64: I = c * 64, and the round trip still gives c
    beauty, aov = _image([[_pixel((1, 2, 3), (0.0, 0.001, 1.0))]])
    G, c, A, I, n, z = D.prepare(beauty, aov)
    assert A[0, 0].tolist() == [0.015625, 0.015625, 1.0] and I[0, 0].tolist() == [64, 128, 3]
    assert D.run(beauty, aov, 3)[0, 0].tolist() == [1, 2, 3, 0]


def test_an_image_without_guides_passes_its_colour_through():
    rows = [[_pixel((1, 2, 3), (0.5, 0.5, 0.5), hits=0), _pixel((4, 5, 6), (0.5, 0.5, 0.5), hits=0, bw=0.0)],
            [_pixel((0.25, 0, 9), (0, 0, 0), hits=0, samples=0), _pixel((7, 7, 7), (1, 1, 1), hits=0)]]
    beauty, aov = _image(rows)
    beauty[0, 1, 0:3] = (4, 5, 6)                                       # (bw == 0 with colour in the sums: c is +0, not a NaN)
    want = np.array([[[1, 2, 3, 0], [0, 0, 0, 0]], [[0.25, 0, 9, 0], [7, 7, 7, 0]]], F)
    for it in (0, 1, 4):
        out = D.run(beauty, aov, it)
        assert (out.view(U) == want.view(U)).all(), (it, out)
    # a guided pixel among them has no tap but itself
    rows[1][1] = _pixel((7, 7, 7), (1, 1, 1), hits=2)
    beauty, aov = _image(rows)
    beauty[0, 1, 0:3] = (4, 5, 6)
    out = D.run(beauty, aov, 4)
    assert (out.view(U) == want.view(U)).all()


def test_a_lit_pixel_takes_its_5_x_5_window_out_of_the_guides():
    """a directly seen emitter and the reach of the reconstruction filter around it are passed through"""
    rows = [[_pixel((1 + x + y, 1, 1), (0.5, 0.5, 0.5)) for x in range(9)] for y in range(7)]
    beauty, aov = _image(rows)
    aov[3, 5, 9] = 2.0                                                  # one channel of one pixel's emission sum
    G = D.prepare(beauty, aov)[0]
    want = np.ones((7, 9), bool)
    want[1:6, 3:8] = False
    assert (G == want).all(), G
    aov[0, 0, 8:11] = (0, 0, 0.5)                                       # ... in a corner: the window is clipped by the image
    want[0:3, 0:3] = False
    assert (D.prepare(beauty, aov)[0] == want).all()
    out = D.run(beauty, aov, 3)
    c = beauty[..., 0:3] / beauty[..., 3:4]
    assert (out[~want][:, 0:3] == c[~want]).all() and (out[~want][:, 3] == 0).all() and (out[want][:, 0:3] != c[want]).any()
    aov[..., 8:11] = -1.0                                               # (not above 0: nobody is lit)
    assert D.prepare(beauty, aov)[0].all()


def test_two_pixels_with_the_normal_stop_on():
    """1 x 2, albedo 1, grey colours 1 and 3, normals (0, 0, 1) and (0, 0, 0.5): with sigma_normal 0.5 en = 0.25 * 4 = 1 across the
    pair; the other stops off.  One iteration at step 1, spelled out in scalars."""
    beauty, aov = _image([[_pixel((1, 1, 1), (1, 1, 1)), _pixel((3, 3, 3), (1, 1, 1), n=(0, 0, 0.5))]])
    e1 = D.hj_exp(np.array([-1.0], F))[0]
    assert abs(float(e1) - np.exp(-1.0)) < 1e-7
    wc, ws = F(0.375) * F(0.375) * F(1), (F(0.25) * F(0.375)) * e1      # (exp(-0) is exactly 1)
    assert wc == F(0.140625)
    y0 = (F(0.2126) * F(1) + F(0.7152) * F(1)) + F(0.0722) * F(1)
    y1 = (F(0.2126) * F(3) + F(0.7152) * F(3)) + F(0.0722) * F(3)
    m1, m2 = y0 + y1, y0 * y0 + y1 * y1                                 # (the 5 x 5 window holds the same two pixels for both)
    mu = m1 / F(2)
    v0 = max(m2 / F(2) - mu * mu, F(0))
    assert abs(float(v0) - 1.0) < 1e-5                                  # (the variance of {1, 3} about their mean)
    start = D.run(beauty, aov, 0, 0.5, 0, 0, 0)
    assert start[0, 0].tolist() == [1, 1, 1, v0] and start[0, 1].tolist() == [3, 3, 3, v0]
    out = D.run(beauty, aov, 1, 0.5, 0, 0, 0)
    # pixel 0: the centre tap (dx = 0), then dx = +1; pixel 1: dx = -1, then the centre
    i0 = (F(1) * wc + F(3) * ws) / (wc + ws)
    i1 = (F(1) * ws + F(3) * wc) / (ws + wc)
    p0 = (v0 * (wc * wc) + v0 * (ws * ws)) / ((wc + ws) * (wc + ws))
    p1 = (v0 * (ws * ws) + v0 * (wc * wc)) / ((ws + wc) * (ws + wc))
    assert out[0, 0].tolist() == [i0, i0, i0, p0] and out[0, 1].tolist() == [i1, i1, i1, p1], out
    assert 1 < i0 < 1.5 and 2.5 < i1 < 3 and p0 < v0
    # without the stop the pair mixes more; with a tight one it does not mix at all
    loose, tight = D.run(beauty, aov, 1, 0, 0, 0, 0), D.run(beauty, aov, 1, 0.01, 0, 0, 0)
    assert loose[0, 0, 0] > i0 and tight[0, 0].tolist() == [1, 1, 1, v0] and tight[0, 1].tolist() == [3, 3, 3, v0]


def test_the_slope_is_the_smaller_difference_at_a_depth_step():
    z = np.array([[1, 2, 3, 10, 12, 11.5]], F)
    G = np.ones((1, 6), bool)
    # x:        0 forward only   1 tie -> forward   2 backward 1 < 7   3 forward 2 < 7   4 forward -0.5   5 backward only
    assert D.slope(z, G, 1)[0].tolist() == [1, 1, 1, 2, -0.5, -0.5]
    assert D.slope(z, G, 0)[0].tolist() == [0] * 6                      # (one row: no neighbour along y)
    assert D.slope(np.array([[0, 1, 0]], F), np.ones((1, 3), bool), 1)[0].tolist() == [1, -1, -1]   # a tie of opposite signs: forward
    G[0, 1] = False                                                     # differences whose neighbour is not guided do not count
    assert D.slope(z, G, 1)[0, [0, 2]].tolist() == [0, 7]
    col = D.slope(z.T.copy(), np.ones((6, 1), bool), 0)
    assert col[:, 0].tolist() == [1, 1, 1, 2, -0.5, -0.5]
    # a depth step in an image: the depth stop, in units of that slope, keeps the two sides apart and the ramp together
    rows = [[_pixel((1, 1, 1) if x < 3 else (5, 5, 5), (1, 1, 1), z=(1 + x) if x < 3 else (10 + x)) for x in range(6)]]
    beauty, aov = _image(rows)
    out = D.run(beauty, aov, 2, 0, 1.0, 0, 0)
    # (across the step at distance 2 the tap is 11 / 2 slopes away: exp(-5.5) of a weight, a few per cent of the difference of 4)
    assert np.allclose(out[0, :3, 0], 1, atol=0.05) and np.allclose(out[0, 3:, 0], 5, atol=0.05)
    assert not np.allclose(D.run(beauty, aov, 2, 0, 0, 0, 0)[0, :, 0], [1, 1, 1, 5, 5, 5], atol=0.5)
