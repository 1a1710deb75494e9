"""hj_denoise_frame_temporal, the part that needs no GPU: the symbol, the version, the defines, the struct and the contract's key
sentences; every argument refusal in the header's order without a device, with its message and with nothing written; the compiler's
resource report of the unit; the reference of the GPU tests (temporal_ref) on hand-derived values; and the half-pixel test, the one
geometric check that does not trust the contract's own arithmetic."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import temporal_ref as T
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_aov_host import _in_order, _refused
from test_denoise_host import _image, _pixel
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAME = "hj_denoise_frame_temporal"


def test_entry_point_is_declared_listed_and_exported():
    assert NAME in declared_functions("hijiki_hip.h") and NAME in device.EXPORTS and hasattr(device.lib(), NAME)
    assert device.lib().hj_version() >= 0x001C00
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_TEMPORAL_WORDS 12", "#define HJ_TEMPORAL_FEEDBACK 1u", "#define HJ_TEMPORAL_VARIANCE_FRAMES 4u", "hj_denoise_frame_temporal (ABI 0.28)",
                 "px = (float)x + 0.5f, py = (float)y + 0.5f", "P = position + z * d, one multiply and one add per channel", "c = rotate(v, conj(prev.rotation))",
                 "There is no history unless c.z < 0", "sx = (c.x / -c.z) * k + 0.5f * W", "sy = (-c.y / -c.z) * k + 0.5f * H", "fx = sx - 0.5f, ix = floorf(fx), tx = fx - ix",
                 "zp = sqrtf(sq(v))", "b outer, a inner", "fabsf(z_h - zp) <= depth_tolerance * zp", "ws is not above 0",
                 "N = fminf(N_prev + 1.0f, (float)max_history)", "a = fmaxf(alpha, 1.0f / N)", "I = I_prev * (1.0f - a) + I_cur * a", "V = fmaxf(m2 - m1 * m1, 0.0f)",
                 "N < HJ_TEMPORAL_VARIANCE_FRAMES", "the I' of the first iteration", "history_in == NULL gives an out that is hj_denoise_frame's bit for bit",
                 "A pixel\n *     that is not guided writes twelve zeros", "A refused call\n *   writes nothing", "they are not tuned", "motion vectors for moved shapes",
                 "3 x 3 fallback search"):
        assert text in header, text
    assert "Not here: temporal accumulation" not in header              # (the denoiser's "Not here" list no longer names it)
    assert (abi.TEMPORAL_WORDS, abi.TEMPORAL_FEEDBACK, abi.TEMPORAL_VARIANCE_FRAMES) == (12, 1, 4)
    assert C.sizeof(abi.TemporalOpts) == 120 and [f[0] for f in abi.TemporalOpts._fields_] == ["camera", "prev_camera", "alpha", "alpha_moments", "depth_tolerance",
                                                                                             "normal_cos", "max_history", "flags"]
    assert abi.TemporalOpts.alpha.offset == 96 and abi.TemporalOpts.flags.offset == 116
    assert '"hj_denoise_temporal.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert callable(device.Renderer.denoise_frame_temporal) and "not tuned" in device.Renderer.denoise_frame_temporal.__doc__


@pytest.fixture(autouse=True)
def _the_library_has_the_call():
    """every test of this file is about hj_denoise_frame_temporal, the reference's self-checks included: none passes without the symbol"""
    assert hasattr(device.lib(), NAME) and NAME in device.EXPORTS


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_argument_refusals_come_before_the_device_in_order():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
    W, H = 6, 5
    arrays = [np.full((H, W, k), 7.0, F) for k in (4, 12, 12, 12, 4)]
    Bp, Ap, Ip, Hp, Op = (a.ctypes.data for a in arrays)
    assert all(p % 16 == 0 for p in (Bp, Ap, Ip, Hp, Op))

    def make(o=True, to=True, it=5, sn=0.5, sz=1.0, sl=4.0, sa=0.1, f=0, w=W, h=H, b=Bp, a=Ap, hi=Ip, ho=Hp, out=Op, tf=1, al=0.2, am=0.2, dt=0.1, nc=0.9, mh=64,
             fov=60.0, pfov=60.0, pos=0.0, prot=0.0):
        opts = abi.DenoiseOpts(it, sn, sz, sl, sa, f)
        topts = abi.TemporalOpts(T.camera((pos, 0, 0), fov=fov), T.camera(rotation=(prot, 0, 0, 1), fov=pfov), al, am, dt, nc, mh, tf)
        return lambda: L.hj_denoise_frame_temporal(None, w, h, b, a, C.byref(opts) if o else None, C.byref(topts) if to else None, hi, ho, out)

    nan, inf = float("nan"), float("inf")
    _in_order(make, NAME, [(b"null opts", dict(o=False)), (b"unknown flag bits", dict(f=2)), (b"9 iterations, at most 8", dict(it=9)),
                           (b"sigma_depth -1", dict(sz=-1.0)), (b"image 0 x", dict(w=0)), (b"unknown temporal flag bits", dict(tf=2)), (b"alpha 2", dict(al=2.0)),
                           (b"alpha_moments -0.5", dict(am=-0.5)), (b"depth_tolerance -1", dict(dt=-1.0)), (b"normal_cos 1.5", dict(nc=1.5)),
                           (b"max_history 0", dict(mh=0)), (b" camera:", dict(fov=0.0)), (b"history_out aliases", dict(ho=Ap)),
                           (b"16-byte aligned", dict(f=1, hi=Ip + 4))])
    for kw, word in ((dict(to=False), b"null topts"), (dict(a=None), b"null aov"), (dict(ho=None), b"null history_out"), (dict(out=None), b"null out"),
                     (dict(to=False, a=None, ho=None, out=None), b"null topts"), (dict(a=None, ho=None, out=None), b"null aov"), (dict(ho=None, out=None), b"null history_out"),
                     (dict(tf=0x80000000), b"unknown temporal flag bits"), (dict(al=nan), b"alpha nan"), (dict(al=-0.25), b"alpha -0.25"), (dict(am=nan), b"alpha_moments"),
                     (dict(am=1.5), b"alpha_moments 1.5"), (dict(dt=inf), b"depth_tolerance inf"), (dict(dt=nan), b"depth_tolerance"), (dict(nc=nan), b"normal_cos"),
                     (dict(nc=-1.5), b"normal_cos -1.5"), (dict(mh=65536), b"max_history 65536"), (dict(fov=180.0), b" camera:"), (dict(fov=nan), b" camera:"),
                     (dict(pos=inf), b" camera:"), (dict(pfov=0.0), b"prev_camera:"), (dict(pfov=200.0), b"prev_camera:"), (dict(prot=nan), b"prev_camera:"),
                     (dict(fov=0.0, pfov=0.0), b" camera:"), (dict(ho=Bp), b"history_out aliases"), (dict(ho=Ip), b"history_out aliases"),
                     (dict(ho=Op), b"history_out aliases"), (dict(ho=Ap + 48), b"history_out aliases"), (dict(ho=Op - 48), b"history_out aliases"),
                     (dict(f=1, b=Bp + 8), b"16-byte aligned"), (dict(f=1, a=Ap + 4), b"16-byte aligned"), (dict(f=1, ho=Hp + 4), b"16-byte aligned"),
                     (dict(f=1, out=Op + 4), b"16-byte aligned"), (dict(w=16385), b"image 16385 x"), (dict(h=0), b"x 0")):
        _refused(make(**kw), NAME, word)
    _refused(make(b=Bp + 4), NAME, gate, status)                        # (host arrays need no alignment)
    for kw in (dict(), dict(f=1), dict(b=None), dict(hi=None), dict(f=1, b=None, hi=None), dict(it=0, tf=0), dict(al=0.0, am=1.0, dt=0.0, nc=-1.0, mh=65535),
               dict(al=1.0, nc=1.0, mh=1, fov=179.0, pfov=1.0)):
        _refused(make(**kw), NAME, gate, status)
    assert all((a == 7.0).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_temporal_kernels_use_no_scratch_and_no_lds(tmp_path):
    """The compiler's resource report for api/denoise_temporal.hip (the Makefile's flags): exactly the three kernels of
    hj_denoise_temporal.h - none of hj_denoise.h's, which stay api/denoise.hip's -, no scratch, no LDS.  Registers and occupancy are
    printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert " denoise_temporal " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "dt.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "denoise_temporal.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_d[nt]_\w+", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_dt_accumulate", "k_dt_feedback", "k_dt_variance"] and len(report) == 3, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_denoise_temporal.h")).read()
    assert "atomic" not in src.replace("no global atomic", "") and "asm" not in src.replace("inline assembly", "")
    assert "#pragma clang fp contract(off)" in src and "getenv" not in src and '#include "hj_denoise.h"' in src and '#include "hj_num.h"' in src
    host = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "denoise_temporal.hip")).read()
    assert "#pragma clang fp contract(off)" in host and "getenv" not in host


# ------------------------------------------------------------------------------------------------- the reference against itself

def _lum(c):
    return (F(0.2126) * F(c[0]) + F(0.7152) * F(c[1])) + F(0.0722) * F(c[2])


def _record(I, N, m1, m2, z, n=(0, 0, 1), valid=1):
    r = np.zeros(12, F)
    r[0:3], r[3], r[4], r[5], r[6], r[8:11] = I, N, m1, m2, z, n
    r.view(U)[7] = valid
    return r


def test_the_rotation_is_the_cameras_own():
    """rotate() over (u, -v, -1), normalised by the numeric contract's normalize3, is the oracle's camera ray, bit for bit; and the
    conjugate undoes it"""
    from probe_vis_ref import normalize3
    W, H = 9, 5
    for q in (T.axis_angle((0, 1, 0), 25), T.axis_angle((1, 2, -0.5), 140), [0, 0, 0, 1]):
        cam = T.camera((1, 2, 3), q, 70.0)
        y, x = np.mgrid[0:H, 0:W]
        u, v = (x.astype(F) + F(0.5)) - F(0.5) * F(W), (y.astype(F) + F(0.5)) - F(0.5) * F(H)
        u, v = (u * T.tan_half(cam)) / (F(0.5) * F(W)), (v * T.tan_half(cam)) / (F(0.5) * F(W))
        vv = np.stack([u, -v, np.full_like(u, -1)], -1).astype(F)
        d = normalize3(T.rotate(vv, q)).reshape(H, W, 3)
        assert (d.view(U) == T.directions(cam, W, H).view(U)).all()
        back = T.rotate(T.rotate(vv, q), [-q[0], -q[1], -q[2], q[3]])
        assert np.allclose(back, vv, atol=1e-5)


def test_one_pixel_with_a_history_blends_by_hand():
    """1 x 1, identical cameras without rotation: d = (0, 0, -1), the point reprojects to fx = fy = 0, the one tap in the image has
    the weight 1.  N_prev = 3 -> N = 4, a = max(0.2, 1 / 4) = 0.25: I = I_prev * 0.75 + I_cur * 0.25, and the variance is the
    temporal one."""
    beauty, aov = _image([[_pixel((1, 2, 3), (0.5, 0.25, 0.75), z=2.0)]])
    cam = T.camera((0.5, -1, 2), fov=60.0)
    hist = _record((4, 4, 8), 3, 5.0, 30.0, 2.0)[None, None]
    out, h, s = T.run(beauty, aov, cam, cam, hist, iterations=0, keep=True)
    assert s["has"].all() and s["I_cur"][0, 0].tolist() == [2, 8, 4]
    want_I = [F(4) * F(0.75) + F(2) * F(0.25), F(4) * F(0.75) + F(8) * F(0.25), F(8) * F(0.75) + F(4) * F(0.25)]
    assert want_I == [3.5, 5.0, 7.0] and h[0, 0, 0:3].tolist() == want_I and h[0, 0, 3] == 4
    y = _lum((2, 8, 4))
    m1, m2 = F(5) * F(0.75) + y * F(0.25), F(30) * F(0.75) + (y * y) * F(0.25)
    assert h[0, 0, 4:7].tolist() == [m1, m2, 2.0] and h.view(U)[0, 0, 7] == 1 and h[0, 0, 8:12].tolist() == [0, 0, 1, 0]
    V = max(m2 - m1 * m1, F(0))
    assert V > 0 and out[0, 0].tolist() == [F(3.5) * F(0.5), F(5) * F(0.25), F(7) * F(0.75), V]
    # a history of 2 frames: N = 3 < 4, a = 1 / 3, and the variance is the spatial one - of a single pixel: 0
    hist[0, 0, 3] = 2
    out, h = T.run(beauty, aov, cam, cam, hist, iterations=0)
    a = F(1) / F(3)
    assert h[0, 0, 3] == 3 and h[0, 0, 0] == F(4) * (F(1) - a) + F(2) * a and out[0, 0, 3] == 0
    # the cap: N_prev = 64 stays 64, a = alpha; max_history 1: N = 1, a = 1 -> the new frame alone
    hist[0, 0, 3] = 64
    assert T.run(beauty, aov, cam, cam, hist, iterations=0)[1][0, 0, 3] == 64
    h = T.run(beauty, aov, cam, cam, hist, iterations=0, max_history=1)[1]
    assert h[0, 0, 0:4].tolist() == [2, 8, 4, 1]
    # alpha 1: the new frame alone whatever N; alpha 0 with N_prev = 64: a = 1 / 64
    assert T.run(beauty, aov, cam, cam, hist, iterations=0, alpha=1.0)[1][0, 0, 0:3].tolist() == [2, 8, 4]
    assert T.run(beauty, aov, cam, cam, hist, iterations=0, alpha=0.0)[1][0, 0, 0] == F(4) * (F(1) - F(1) / F(64)) + F(2) * (F(1) / F(64))


def test_each_way_to_lose_the_history_gives_the_spatial_denoiser():
    rows = [[_pixel((1 + 0.25 * x + y, 1, 2), (0.5, 0.5, 0.5), z=2.0 + 0.125 * x) for x in range(6)] for y in range(4)]
    beauty, aov = _image(rows)
    cam = T.camera(fov=60.0)
    G, c, A, I, n, z = D.prepare(beauty, aov)
    hist = np.zeros((4, 6, 12), F)
    hist[..., 0:3], hist[..., 3], hist[..., 4], hist[..., 5], hist[..., 6], hist[..., 8:11] = 9.0, 5, 9, 90, z, n
    hist.view(U)[..., 7] = 1
    spatial = D.run(beauty, aov, 2)
    first = T.run(beauty, aov, cam, cam, None, 2)
    assert (first[0].view(U) == spatial.view(U)).all() and (first[1][..., 3] == 1).all() and (first[1].view(U)[..., 7] == 1).all()
    assert not (T.run(beauty, aov, cam, cam, hist, 2)[0] == spatial).all()                            # (the history does something)
    holes = hist.copy()
    holes.view(U)[..., 7] = 0
    far, turned = hist.copy(), hist.copy()
    far[..., 6] = z * F(1.25)
    turned[..., 8:11] = (0.0, 0.8, 0.6)
    back = T.camera(rotation=T.axis_angle((0, 1, 0), 180), fov=60.0)
    for what, got in (("valid words 0", T.run(beauty, aov, cam, cam, holes, 2)), ("depths off", T.run(beauty, aov, cam, cam, far, 2)),
                      ("normals off", T.run(beauty, aov, cam, cam, turned, 2)), ("looking the other way", T.run(beauty, aov, cam, back, hist, 2))):
        assert (got[0].view(U) == spatial.view(U)).all() and (got[1].view(U) == first[1].view(U)).all(), what
    # feedback: the history's light is the first iteration's, not the accumulated one; without an iteration there is nothing to feed
    fed, plain = T.run(beauty, aov, cam, cam, hist, 2)[1], T.run(beauty, aov, cam, cam, hist, 2, feedback=False)[1]
    assert (fed[..., 3:] == plain[..., 3:]).all() and not (fed[..., 0:3] == plain[..., 0:3]).all()
    zero = [T.run(beauty, aov, cam, cam, hist, 0, feedback=fb)[1] for fb in (True, False)]
    assert (zero[0].view(U) == zero[1].view(U)).all() and (zero[0].view(U) == plain.view(U)).all()
    # a pixel that is not guided writes twelve zeros and is no tap
    aov[1, 2, 11] = 0
    got = T.run(beauty, aov, cam, cam, hist, 1)[1]
    assert (got[1, 2].view(U) == 0).all() and (got.view(U)[..., 7].sum() == 23)


# ------------------------------------------------------------------------------------------------------------ the half-pixel test

def test_a_shifted_camera_reads_an_affine_history_exactly():
    """A plane, fronto-parallel to two cameras of one (non-trivial) orientation that differ by a translation parallel to it of
    (3.37, -2.6) pixels.  History light and current light are one affine function f of the WORLD point, evaluated in float64 from
    the geometry alone - rays through pixel centres (x + 1/2, y + 1/2), image y downwards, the camera looking down its -z - and not
    from the contract's projection.  Bilinear interpolation reproduces an affine function of the pixel position exactly, so the
    reprojected I_prev, and the accumulated I, must be f at the pixel's own point, to |grad f| per pixel x 1 / 64 pixel: the
    float32 projection chain (some twenty operations at magnitudes below 100 pixels) stays under 1e-3 pixel, while a wrong half-pixel
    convention, axis sign or conjugate is off by half a pixel or more - 32 tolerances."""
    W, H, fov, dist = 64, 48, 60.0, 4.0
    q = [np.float64(v) for v in T.axis_angle((0.3, 1.0, -0.2), 35)]
    qv, qw = np.array(q[0:3]), q[3]

    def rot(v, inverse=False):                                          # v + 2 qw (qv x v) + 2 qv x (qv x v), the textbook form, float64
        s = -1.0 if inverse else 1.0
        t = 2.0 * np.cross(s * qv, v)
        return v + qw * t + np.cross(s * qv, t)

    tan = np.tan(np.radians(fov / 2))
    pixel = dist * tan / (W / 2)                                        # the side of a pixel on the plane
    shift = np.array([3.37, -2.6])
    p_prev = np.array([0.4, -0.2, 1.0])
    p_cur = p_prev + rot(np.array([shift[0] * pixel, shift[1] * pixel, 0.0]))
    grad, f0 = np.array([0.7, -0.4, 0.5]), 6.0
    f = lambda P: f0 + P @ grad                                         # noqa: E731

    def frame_of(pos):
        """the world point and the distance along the ray of every pixel centre, float64"""
        y, x = np.mgrid[0:H, 0:W]
        u, v = (x + 0.5 - W / 2) * tan / (W / 2), (y + 0.5 - H / 2) * tan / (W / 2)
        local = np.stack([u, -v, -np.ones_like(u)], -1) * dist           # on the plane z = -dist of the camera's frame
        return pos + rot(local), np.linalg.norm(local, axis=-1)

    P_cur, t_cur = frame_of(p_cur)
    P_prev, t_prev = frame_of(p_prev)
    normal = rot(np.array([0.0, 0.0, 1.0]))
    hist = np.zeros((H, W, 12), F)
    hist[..., 0:3], hist[..., 3], hist[..., 4], hist[..., 5], hist[..., 6], hist[..., 8:11] = f(P_prev)[..., None], 7, 1, 2, t_prev, normal
    hist.view(U)[..., 7] = 1
    rows = [[_pixel((f(P_cur[y, x]),) * 3, (1, 1, 1), n=normal, z=t_cur[y, x]) for x in range(W)] for y in range(H)]
    beauty, aov = _image(rows)
    cam, prev = T.camera(p_cur, [float(F(v)) for v in q], fov), T.camera(p_prev, [float(F(v)) for v in q], fov)
    # which pixels keep all four taps: the point seen from the previous camera, by the pinhole's own inverse, float64
    local = rot(P_cur - p_prev, inverse=True)
    fx = (local[..., 0] / -local[..., 2]) * (W / 2) / tan + W / 2 - 0.5
    fy = (-local[..., 1] / -local[..., 2]) * (W / 2) / tan + H / 2 - 0.5
    keep = (fx > 0.02) & (fx < W - 1.02) & (fy > 0.02) & (fy < H - 1.02)
    assert keep.sum() * 2 >= W * H, keep.sum()
    y, x = np.mgrid[0:H, 0:W]
    assert np.allclose(fx, x + shift[0], atol=1e-9) and np.allclose(fy, y - shift[1], atol=1e-9)   # (the camera's +y is the image's -y)
    in_plane = rot(grad, inverse=True)[0:2]                             # f's gradient along the plane, per world unit
    tol = np.linalg.norm(in_plane) * pixel / 64
    G, c, A, I, n, z = D.prepare(beauty, aov)
    assert G.all()
    has, I_prev, m1, m2, N = T.reproject(G, n, z, cam, prev, hist, 0.1, 0.9)
    assert has[keep].all()
    err = np.abs(I_prev[..., 0].astype(np.float64) - f(P_cur))[keep].max()
    print(f"reprojected history against the geometry: max error {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol and np.allclose(N[keep], 7, rtol=1e-6, atol=0)
    out, h = T.run(beauty, aov, cam, prev, hist, iterations=0, alpha=0.0)
    err = np.abs(h[..., 0:3].astype(np.float64) - f(P_cur)[..., None])[keep].max()
    assert err <= tol and np.allclose(h[keep][:, 3], 8, rtol=1e-6, atol=0)
    # the check can fail: a history half a pixel off along f's gradient (a wrong convention) is off by 32 tolerances
    wrong = hist.copy()
    wrong[..., 0:3] = f(P_prev + rot(np.array([*(0.5 * pixel * in_plane / np.linalg.norm(in_plane)), 0.0])))[..., None]
    I_wrong = T.reproject(G, n, z, cam, prev, wrong, 0.1, 0.9)[1]
    assert np.abs(I_wrong[..., 0].astype(np.float64) - f(P_cur))[keep].min() > 31 * tol
