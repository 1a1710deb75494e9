"""hj_render_motion_followed, the part that needs no GPU: the symbol, the version, the defines and the contract's key sentences; every
argument refusal in the header's order without a device, with its message and with nothing written; the compiler's resource report
of the unit; and the reference of the GPU tests (motion_follow_ref) against a float64 geometry that does not trust the contract's
own arithmetic - one planar mirror, two mirrors in a corner whose reflections do not commute - and on the static anchor."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import follow_ref as R
import motion_follow_ref as MF
import motion_ref as M
import path_query_ref as P
import temporal_ref as T
from hijiki_amd import abi, device, host
from test_abi import ROOT, declared_functions
from test_aov_host import _in_order, _refused
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAME = "hj_render_motion_followed"


def test_entry_point_is_declared_listed_and_exported():
    assert NAME in declared_functions("hijiki_hip.h") and NAME in device.EXPORTS and hasattr(device.lib(), NAME)
    assert device.lib().hj_version() >= 0x001F00 and abi.VERSION >= (0, 31, 0)
    v = device.lib().hj_version()
    assert (v >> 16, (v >> 8) & 0xFF, v & 0xFF) == abi.VERSION
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_MOTION_LEFT 0xFFFFFFFEu", "hj_render_motion_followed (ABI 0.31)", "M_k = M_(k-1) H_k", "w_i = (M_i0 * n.x + M_i1 * n.y) + M_i2 * n.z",
                 "M_ij = M_ij - w2_i * n_j", "Pv = camera.position + D * d0", "delta = X_prev - X_now", "Pv_prev_i = Pv_i + ((M_i0 * delta.x + M_i1 * delta.y) + M_i2 * delta.z)",
                 "max_follow == 0 is hj_render_motion through the same two launches", "word 3 = HJ_MOTION_LEFT", "then max_follow above HJ_AOV_MAX_FOLLOW",
                 "a curved mirror\n *   is treated by its tangent plane", "a refraction carries the displacement through unchanged",
                 "a specular surface that\n *   itself moved is not accounted for", "an environment seen after a mirror is treated as static"):
        assert text in header, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in ("Followed motion", "k_mf_follow", "k_mf_resolve", "kernels/hj_motion_follow.h", "api/motion_follow.hip"):
        assert text in design, text
    assert abi.MOTION_LEFT == 0xFFFFFFFE != abi.MOTION_NONE
    assert '"hj_motion_follow.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "api/motion_follow.hip" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_internal.h")).read()
    assert "follow" in device.Renderer.render_motion.__code__.co_varnames
    with pytest.raises(ValueError):
        device.Renderer.render_motion(None, None, 4, 4, follow=9)


@pytest.fixture(autouse=True)
def _the_library_has_the_call():
    """every test of this file is about the call, the reference's self-checks included: none passes without the symbol"""
    assert hasattr(device.lib(), NAME) and NAME in device.EXPORTS


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_come_before_the_device_in_order():
    """hj_render_motion's refusals in its order (test_motion_host.py) behind the new name, then max_follow, then the gate"""
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
    W, H = 6, 5
    motion = np.full((H, W, 4), 7.0, F)
    spheres, quads, vertices = np.full((2, 4), 1.0, F), np.full((3, 12), 1.0, F), np.full((4, 8), 1.0, F)
    Mp, Sp, Qp, Vp = (a.ctypes.data for a in (motion, spheres, quads, vertices))
    assert all(p % 16 == 0 for p in (Mp, Sp, Qp, Vp))

    def make(p=True, m=Mp, f=0, w=W, h=H, fov=60.0, pos=0.0, rot=0.0, s=Sp, q=Qp, v=Vp, mf=2):
        d = abi.SceneDesc()
        d.camera = T.camera((pos, 0, 0), (rot, 0, 0, 1), fov)
        d.num_spheres, d.num_quads, d.num_vertices = 2, 3, 4
        d.spheres, d.quads, d.vertices = C.cast(C.c_void_p(s), C.POINTER(abi.Sphere)), C.cast(C.c_void_p(q), C.POINTER(abi.Quad)), C.cast(C.c_void_p(v), C.POINTER(abi.Vertex))
        return lambda: L.hj_render_motion_followed(None, C.byref(d) if p else None, w, h, mf, f, m)

    nan, inf = float("nan"), float("inf")
    _in_order(make, NAME, [(b"null prev", dict(p=False)), (b"unknown flag bits", dict(f=4)), (b"image 0 x", dict(w=0)), (b"prev->camera", dict(fov=0.0)),
                           (b"16-byte aligned", dict(f=2, m=Mp + 4)), (b"max_follow 9 above 8", dict(mf=9))])
    for kw, word in ((dict(m=None), b"null motion"), (dict(p=False, m=None), b"null prev"), (dict(f=0x80000000), b"unknown flag bits"), (dict(h=0), b"x 0"),
                     (dict(w=16385), b"image 16385 x"), (dict(h=16385), b"x 16385"), (dict(fov=180.0), b"prev->camera"), (dict(fov=nan), b"prev->camera"),
                     (dict(pos=inf), b"prev->camera"), (dict(rot=nan), b"prev->camera"), (dict(f=1, s=Sp + 4), b"16-byte aligned"),
                     (dict(f=1, q=Qp + 8), b"16-byte aligned"), (dict(f=1, v=Vp + 4), b"16-byte aligned"), (dict(f=3, m=Mp + 8), b"16-byte aligned"),
                     (dict(f=3, fov=0.0, m=Mp + 8), b"prev->camera"), (dict(mf=0xFFFFFFFF), b"max_follow 4294967295 above 8")):
        _refused(make(**kw), NAME, word)
    for kw in (dict(), dict(mf=0), dict(mf=1), dict(mf=8), dict(f=1), dict(f=2), dict(f=3), dict(m=Mp + 4), dict(s=Sp + 4, q=Qp + 4, v=Vp + 4), dict(f=2, s=Sp + 4),
               dict(f=1, m=Mp + 4), dict(s=None, q=None, v=None), dict(fov=179.0, w=16384, h=1)):
        _refused(make(**kw), NAME, gate, status)                        # (host arrays need no alignment; a NULL kind did not move)
    assert (motion == 7.0).all()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_motion_follow_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/motion_follow.hip (the Makefile's flags): exactly the kernels of hj_motion_follow.h -
    not k_mv_walk or k_mv_resolve, which api/motion.hip holds, nor a kernel of hj_follow.h or the count and scan of hj_chain.h, which
    api/follow.hip holds -; no kernel
    has scratch and none spills a register.  LDS: the path kernels' WgShared in the walk, the scan's partial sums, a word per wave
    in the count and the scatter.  Registers and occupancy are printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert " motion_follow " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "mf.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "motion_follow.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_mf_(resolve|scatter<\w+>|follow<\w+>)", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_mf_follow<false>", "k_mf_follow<true>", "k_mf_resolve", "k_mf_scatter<false>", "k_mf_scatter<true>"] and len(report) == 5, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert (v["LDS Size"] > 16 * 1024) == k.startswith("k_mf_follow<") and v["LDS Size"] <= 20 * 1024, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_motion_follow.h")).read()
    assert "atomic" not in src.replace("No global atomics", "") and "asm" not in src.replace("no inline assembly", "") and "getenv" not in src
    assert "#pragma clang fp contract(off)" in src and "mv_record(" in src and "HJ_DEV float4 mv_record" not in src               # (included, not restated)
    chain = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_chain.h")).read()
    assert "follow_continue_branch(" in chain and "compact_scan_tiles<" in chain and "HJ_COMPACT_RANK(" in chain                 # (the rounds' text, once)
    assert "follow_continue_branch(" not in src and "compact_scan_tiles<" not in src and "HJ_COMPACT_RANK(" not in src and "trace_persistent<" not in src
    assert '#include "hj_chain.h"' in src and "HJ_CHAIN_NO_KERNELS" in src and "chain_scatter<FIRST>(" in src and "chain_round<PAIRS>(" in src
    assert "mf_householder(m0, m1, m2, nrm)" in src
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "motion_follow.hip")).read()


# ------------------------------------------------------------------------------------------------------------ the float64 judges

def _rot64(q, v, inverse=False):
    """v + 2 qw (qv x v) + 2 qv x (qv x v), the textbook form, float64"""
    qv, qw = np.array(q[0:3], np.float64) * (-1.0 if inverse else 1.0), np.float64(q[3])
    t = 2.0 * np.cross(qv, v)
    return v + qw * t + np.cross(qv, t)


def _pinhole64(cam, X, W, H):
    """float64: world points X (..., 3) through the camera's pinhole - image y downwards, looking down its -z, pixel centres at
    (x + 1/2, y + 1/2) -> sx, sy, distance"""
    pos = np.array(list(cam.position)[0:3], np.float64)
    loc = _rot64(list(cam.rotation), X - pos, inverse=True)
    tan = np.tan(np.radians(float(cam.fov) / 2))
    assert (loc[..., 2] < 0).all()
    return (loc[..., 0] / -loc[..., 2]) * (W / 2) / tan + W / 2, (-loc[..., 1] / -loc[..., 2]) * (W / 2) / tan + H / 2, np.linalg.norm(X - pos, axis=-1)


def _centre_dirs64(cam, W, H):
    tan = np.tan(np.radians(float(cam.fov) / 2))
    y, x = np.mgrid[0:H, 0:W]
    local = np.stack([(x + 0.5 - W / 2) * tan / (W / 2), -(y + 0.5 - H / 2) * tan / (W / 2), -np.ones((H, W))], -1)
    d = _rot64(list(cam.rotation), local)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)


def _judge(oracle, s, mirrors, target, moved, prev_cam, W, H, min_pixels):
    """s: a host.Scene whose quads `mirrors` (ids, in chain order) are planar mirrors and whose quad `target` is diffuse; moved: the
    target's previous 12 words.  For every pixel whose chain is exactly camera -> mirrors... -> target the exact geometry in float64:
    the centre ray reflected at each mirror's plane, its point on the target's plane solved for (u, v) from the point itself,
    carried onto the previous quad, reflected back through the mirrors' planes in reverse order - the exact virtual image of X_prev -
    and projected through the previous pinhole.  -> the reference's deviation from it in pixels (sx, sy) and relative (zp)."""
    cs = s.compile()
    cam = cs.desc.camera
    quads = np.array(cs.quads, F)
    prev_quads = quads.copy()
    prev_quads[target] = moved
    prev = M.Prev(cs, prev_cam, quads=prev_quads)
    got, det = MF.render_motion_followed(cs, prev, W, H, 8, R.oracle_trace(cs), detail=True)
    want_ids = len(cs.spheres) + target
    sel = (det["count"] == len(mirrors)) & ~det["left"] & (MF.ids_of(got).ravel() == want_ids)
    assert sel.sum() >= min_pixels, sel.sum()
    planes = []
    for k in mirrors:
        q = quads[k].astype(np.float64)
        nrm = np.cross(q[4:7], q[8:11])
        planes.append((q[0:3], nrm / np.linalg.norm(nrm)))
    o = np.tile(np.array(list(cam.position)[0:3], np.float64), (W * H, 1))[sel]
    d = _centre_dirs64(cam, W, H)[sel]
    for p0, nrm in planes:
        t = ((p0 - o) @ nrm) / (d @ nrm)
        assert (t > 0).all()
        o = o + t[:, None] * d
        d = d - 2.0 * (d @ nrm)[:, None] * nrm
    q = quads[target].astype(np.float64)
    nrm = np.cross(q[4:7], q[8:11])
    t = ((q[0:3] - o) @ nrm) / (d @ nrm)
    X = o + t[:, None] * d
    uv = np.linalg.lstsq(np.stack([q[4:7], q[8:11]], 1), (X - q[0:3]).T, rcond=None)[0].T
    assert (uv > 0).all() and (uv < 1).all()
    was = np.asarray(moved, np.float64)
    Xp = was[0:3] + uv[:, 0:1] * was[4:7] + uv[:, 1:2] * was[8:11]
    for p0, nrm in reversed(planes):                                   # the virtual image: R_1(R_2(... X_prev))
        Xp = Xp - 2.0 * ((Xp - p0) @ nrm)[:, None] * nrm
    sx, sy, zp = _pinhole64(prev_cam, Xp, W, H)
    g = got.reshape(-1, 4)[sel]
    y, x = np.mgrid[0:H, 0:W]
    shift = np.hypot(g[:, 0] - (x.ravel()[sel] + 0.5), g[:, 1] - (y.ravel()[sel] + 0.5))
    return np.abs(g[:, 0] - sx).max(), np.abs(g[:, 1] - sy).max(), (np.abs(g[:, 2] - zp) / zp).max(), shift, cs, prev, det, sel


# the position's own gradient is 1 pixel a pixel: test_denoise_temporal_host's half-pixel tolerance, |grad| x 1 / 64 pixel
TOL = 1.0 / 64


def _one_mirror():
    """a camera near the origin looking down -z at a mirror quad at z = -4; behind the camera a diffuse quad at z = +3 that the
    mirror shows"""
    s = host.Scene()
    s.set_camera((0.1, -0.05, 0.2), (0, 0, 0, 1), 60.0)
    grey = s.add_diffuse((0.5, 0.5, 0.5))
    s.add_quad((-4, -4, -4), (8, 0, 0), (0, 8, 0), s.add_mirror())
    s.add_quad((-9, -9, 3), (18, 0, 0), (0, 18, 0), grey)
    return s


def test_one_planar_mirror_in_float64(oracle):
    """measured: sx 8.4e-06, sy 8.8e-06 pixels, zp 2.2e-07 relative (tolerance 1 / 64 pixel = 0.0156)"""
    W, H = 48, 36
    prev_cam = T.camera((0.3, 0.1, 0.05), T.axis_angle((0.2, 1.0, 0.1), 4), 60.0)
    moved = [-8.7, -9.2, 3.4, 0, 18.0, 0.3, 0.2, 0, -0.2, 18.0, 0.1, 0]
    ex, ey, ez, shift, cs, prev, det, sel = _judge(oracle, _one_mirror(), [0], 1, moved, prev_cam, W, H, W * H - 8)
    print(f"one mirror: max |sx| error {ex:.3g}, |sy| {ey:.3g} pixels, zp {ez:.3g} relative; the records lie {shift.min():.3g} ... {shift.max():.3g} pixels from their pixels")
    assert ex <= TOL and ey <= TOL and ez <= 1e-5
    assert shift.max() > 1                                              # the camera and the quad did move
    # the check can fail: hj_render_motion's record of the same pixels - the mirror's own point - is somewhere else
    first = M.render_motion(cs, prev, W, H, [det["first"][:, 0].copy().view(np.int32)] + [det["first"][:, k] for k in (1, 2, 3)]).reshape(-1, 4)[sel]
    got = MF.render_motion_followed(cs, prev, W, H, 1, R.oracle_trace(cs)).reshape(-1, 4)[sel]
    assert np.hypot(first[:, 0] - got[:, 0], first[:, 1] - got[:, 1]).max() > 32 * TOL


def _corner():
    """mirror A at z = -4 in front of the camera; behind the camera mirror B, tilted by 45 degrees about y (normal (1, 0, 1) / sqrt 2),
    which turns what A reflects towards -x; a diffuse quad at x = -8.  H_A = diag(1, 1, -1) and H_B swaps x and z with a sign:
    H_A H_B != H_B H_A"""
    s = host.Scene()
    s.set_camera((0, 0, 0), (0, 0, 0, 1), 40.0)
    grey, mirror = s.add_diffuse((0.5, 0.5, 0.5)), s.add_mirror()
    s.add_quad((-3, -3, -4), (6, 0, 0), (0, 6, 0), mirror)
    s.add_quad((-4, -4, 7), (8, 0, -8), (0, 8, 0), mirror)
    s.add_quad((-8, -10, -10), (0, 20, 0), (0, 0, 20), grey)
    return s


def test_two_mirrors_in_a_corner_in_float64(oracle):
    """measured: sx 1.0e-05, sy 6.7e-06 pixels, zp 2.6e-07 relative (tolerance 1 / 64 pixel = 0.0156)"""
    W, H = 40, 30
    prev_cam = T.camera((0.1, -0.1, 0.1), T.axis_angle((1.0, 0.3, -0.2), 3), 40.0)
    moved = [-7.7, -10.2, -9.6, 0, 0.2, 20.0, 0.1, 0, 0.3, -0.2, 20.0, 0]
    ex, ey, ez, shift, cs, prev, det, sel = _judge(oracle, _corner(), [0, 1], 2, moved, prev_cam, W, H, W * H // 2)
    print(f"two mirrors: max |sx| error {ex:.3g}, |sy| {ey:.3g} pixels, zp {ez:.3g} relative; shifts {shift.min():.3g} ... {shift.max():.3g} pixels")
    assert ex <= TOL and ey <= TOL and ez <= 1e-5
    # the order matters here: the product taken the other way round, H_B H_A, misses by many tolerances
    Mat = det["Mat"][sel]
    HA, HB = np.diag([1.0, 1.0, -1.0]), np.array([[0.0, 0, -1], [0, 1, 0], [-1, 0, 0]])
    assert np.abs(Mat - HA @ HB).max() < 1e-5 and np.abs(HA @ HB - HB @ HA).max() == 2
    g = MF.render_motion_followed(cs, prev, W, H, 8, R.oracle_trace(cs)).reshape(-1, 4)[sel]
    cam_pos = np.array(list(cs.desc.camera.position)[0:3], np.float64)
    Pv = cam_pos + det["D"].ravel()[sel, None].astype(np.float64) * det["d0"][sel].astype(np.float64)
    quads = np.array(cs.quads, np.float64)
    last = det["last"][sel].astype(np.float64)
    Xn = quads[2, 0:3] + last[:, 2:3] * quads[2, 4:7] + last[:, 3:4] * quads[2, 8:11]
    was = prev.quads[2].astype(np.float64)
    Xp = was[0:3] + last[:, 2:3] * was[4:7] + last[:, 3:4] * was[8:11]
    sx, sy, _ = _pinhole64(prev.camera, Pv + (Xp - Xn) @ (HB @ HA).T, W, H)
    assert np.hypot(g[:, 0] - sx, g[:, 1] - sy).min() > 32 * TOL


# ------------------------------------------------------------------------------------------------------------------- the anchor

def test_nothing_moved_and_the_same_camera_stays_at_the_pixel_centre(oracle):
    """"rich" - a mirror sphere, clear and tinted glass, specular triangles - with prev equal to the uploaded state: delta is exactly
    0, so (sx, sy) is the pixel centre to 1e-3 pixel on every pixel whose chain ends in a hit (and where it left, too), zp is
    D * |d0| to 1e-5 relative, and word 3 is the last hit's id or HJ_MOTION_LEFT.  Measured: 1.1e-05 and 7.6e-06 pixels, 1.3e-07 relative"""
    W, H = 70, 41
    cs = P.scene("rich")
    cam = cs.desc.camera
    prev = M.Prev(cs, cam, spheres=cs.spheres.copy(), quads=cs.quads.copy(), vertices=cs.vertices.copy())
    got, det = MF.render_motion_followed(cs, prev, W, H, 8, R.oracle_trace(cs), detail=True)
    went, left, length = det["went"], det["left"].reshape(H, W), det["length"].reshape(H, W)
    ends = went & ~left
    assert ends.sum() > 100 and left.sum() >= 1 and length.max() >= 3, (ends.sum(), left.sum(), length.max())
    y, x = np.mgrid[0:H, 0:W]
    ex, ey = np.abs(got[..., 0] - (x + 0.5))[went].max(), np.abs(got[..., 1] - (y + 0.5))[went].max()
    d0 = np.linalg.norm(det["d0"].astype(np.float64), axis=1).reshape(H, W)
    ez = (np.abs(got[..., 2] - det["D"] * d0) / (det["D"] * d0))[went].max()
    print(f"static anchor: max |sx - centre| {ex:.3g}, |sy - centre| {ey:.3g} pixels, zp against D |d0| {ez:.3g} relative")
    assert ex <= 1e-3 and ey <= 1e-3 and ez <= 1e-5
    ids = MF.ids_of(got)
    assert (ids[left] == MF.LEFT).all() and (ids[ends] == det["last"][:, 0].copy().view(U).reshape(H, W)[ends]).all()
    # a pixel that took no continuation holds hj_render_motion's record, and max_follow = 0 is hj_render_motion
    f = det["first"]
    base = M.render_motion(cs, prev, W, H, (f[:, 0].copy().view(np.int32), f[:, 1], f[:, 2], f[:, 3]))
    assert (got.view(U)[~went] == base.view(U)[~went]).all()
    assert (MF.render_motion_followed(cs, prev, W, H, 0, R.oracle_trace(cs)).view(U) == base.view(U)).all()
    # and with followed guides the static record passes the temporal depth test that the first-hit record fails
    assert (np.abs(base[..., 2] - det["D"])[ends] > 0.1 * base[..., 2][ends]).sum() > 50
