"""hj_render_motion and hj_denoise_frame_temporal_motion, the part that needs no GPU: the symbols, the version, the defines and the
contracts' key sentences; every argument refusal of both calls in the header's order without a device, with its message and with
nothing written; the compiler's resource report of the unit; the reference of the GPU tests (motion_ref) on hand-derived values and
against a float64 geometry that does not trust the contract's own arithmetic; and the anchor that ties the motion form of the
temporal reference to the static one word for word."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import temporal_ref as T
from hijiki_amd import abi, device, host
from test_abi import ROOT, declared_functions
from test_aov_host import _in_order, _refused
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_render_motion", "hj_denoise_frame_temporal_motion")


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001D00
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_MOTION_WORDS 4", "#define HJ_MOTION_NONE 0xFFFFFFFFu", "#define HJ_MOTION_DEVICE_SHAPES 1u", "#define HJ_MOTION_DEVICE_OUT    2u",
                 "hj_render_motion (ABI 0.29)", "hj_denoise_frame_temporal_motion (ABI 0.29)", "px = (float)x + 0.5f, py = (float)y + 0.5f",
                 "P = fma(t, d, o)", "n = (P - c) * (1.0f / r)", "Pp = c' + n * r'", "Pp = (o' + e1' * u) + e2' * v", "l0 = (1.0f - u) - v",
                 "Pp = (a' * l0 + b' * u) + c' * v", "vv = Pp - prev.position", "c = rotate(vv, conj(prev.rotation))", "sx = (c.x / -c.z) * k + 0.5f * W",
                 "sy = (-c.y / -c.z) * k + 0.5f * H", "zp = sqrtf(sq(vv))", "(0, 0, 0, HJ_MOTION_NONE)", "that kind did not move",
                 "48 / 16 / 32 bytes per quad / sphere / vertex", "16 bytes a pixel when motion is a host array", "A refused call writes nothing",
                 "rotation of a sphere about its own centre", "what a mirror or glass\n *   shows", "moving lights' shadows on static surfaces",
                 "motion == NULL: the call is hj_denoise_frame_temporal, bit for bit", "everything from fx = sx - 0.5f on is step 2\n *     unchanged",
                 "still validated but not used", "motion vectors for moved shapes: hj_render_motion and hj_denoise_frame_temporal_motion below",
                 "3 x 3 fallback search"):
        assert text in header, text
    assert (abi.MOTION_WORDS, abi.MOTION_NONE, abi.MOTION_DEVICE_SHAPES, abi.MOTION_DEVICE_OUT) == (4, 0xFFFFFFFF, 1, 2)
    assert C.sizeof(abi.TemporalOpts) == 120
    assert '"hj_motion.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "api/motion.hip" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_internal.h")).read()
    assert callable(device.Renderer.render_motion) and device.Renderer.render_motion.__doc__ and callable(device.motion_ids)
    assert "motion" in device.Renderer.denoise_frame_temporal.__code__.co_varnames
    m = np.zeros((2, 3, 4), F)
    m.view(U)[..., 3] = [[0, 1, 0xFFFFFFFF], [7, 8, 9]]
    assert device.motion_ids(m).dtype == U and device.motion_ids(m).tolist() == [[0, 1, 0xFFFFFFFF], [7, 8, 9]]


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    """every test of this file is about the two calls, the reference's self-checks included: none passes without the symbols"""
    assert all(hasattr(device.lib(), n) and n in device.EXPORTS for n in NAMES)


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_render_motion_refusals_come_before_the_device_in_order():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
    W, H = 6, 5
    motion = np.full((H, W, 4), 7.0, F)
    spheres, quads, vertices = np.full((2, 4), 1.0, F), np.full((3, 12), 1.0, F), np.full((4, 8), 1.0, F)
    Mp, Sp, Qp, Vp = (a.ctypes.data for a in (motion, spheres, quads, vertices))
    assert all(p % 16 == 0 for p in (Mp, Sp, Qp, Vp))
    name = NAMES[0]

    def make(p=True, m=Mp, f=0, w=W, h=H, fov=60.0, pos=0.0, rot=0.0, s=Sp, q=Qp, v=Vp):
        d = abi.SceneDesc()
        d.camera = T.camera((pos, 0, 0), (rot, 0, 0, 1), fov)
        d.num_spheres, d.num_quads, d.num_vertices = 2, 3, 4
        d.spheres, d.quads, d.vertices = C.cast(C.c_void_p(s), C.POINTER(abi.Sphere)), C.cast(C.c_void_p(q), C.POINTER(abi.Quad)), C.cast(C.c_void_p(v), C.POINTER(abi.Vertex))
        return lambda: L.hj_render_motion(None, C.byref(d) if p else None, w, h, f, m)

    nan, inf = float("nan"), float("inf")
    _in_order(make, name, [(b"null prev", dict(p=False)), (b"unknown flag bits", dict(f=4)), (b"image 0 x", dict(w=0)), (b"prev->camera", dict(fov=0.0)),
                           (b"16-byte aligned", dict(f=2, m=Mp + 4))])
    for kw, word in ((dict(m=None), b"null motion"), (dict(p=False, m=None), b"null prev"), (dict(f=0x80000000), b"unknown flag bits"), (dict(h=0), b"x 0"),
                     (dict(w=16385), b"image 16385 x"), (dict(h=16385), b"x 16385"), (dict(fov=180.0), b"prev->camera"), (dict(fov=nan), b"prev->camera"),
                     (dict(pos=inf), b"prev->camera"), (dict(rot=nan), b"prev->camera"), (dict(f=1, s=Sp + 4), b"16-byte aligned"),
                     (dict(f=1, q=Qp + 8), b"16-byte aligned"), (dict(f=1, v=Vp + 4), b"16-byte aligned"), (dict(f=3, m=Mp + 8), b"16-byte aligned"),
                     (dict(f=3, fov=0.0, m=Mp + 8), b"prev->camera")):
        _refused(make(**kw), name, word)
    for kw in (dict(), dict(f=1), dict(f=2), dict(f=3), dict(m=Mp + 4), dict(s=Sp + 4, q=Qp + 4, v=Vp + 4), dict(f=2, s=Sp + 4), dict(f=1, m=Mp + 4),
               dict(s=None, q=None, v=None), dict(fov=179.0, w=16384, h=1)):
        _refused(make(**kw), name, gate, status)                        # (host arrays need no alignment; a NULL kind did not move)
    assert (motion == 7.0).all()


def test_temporal_motion_refusals_come_before_the_device_in_order():
    L = device.lib()
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    gate = b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context"
    W, H = 6, 5
    arrays = [np.full((H, W, k), 7.0, F) for k in (4, 12, 12, 12, 4, 4)]
    Bp, Ap, Ip, Hp, Op, Mp = (a.ctypes.data for a in arrays)
    assert all(p % 16 == 0 for p in (Bp, Ap, Ip, Hp, Op, Mp))
    name = NAMES[1]

    def make(o=True, to=True, it=5, sz=1.0, f=0, w=W, h=H, b=Bp, a=Ap, hi=Ip, ho=Hp, out=Op, mo=Mp, tf=1, al=0.2, am=0.2, dt=0.1, nc=0.9, mh=64, fov=60.0, pfov=60.0):
        opts = abi.DenoiseOpts(it, 0.5, sz, 4.0, 0.1, f)
        topts = abi.TemporalOpts(T.camera(fov=fov), T.camera(fov=pfov), al, am, dt, nc, mh, tf)
        return lambda: L.hj_denoise_frame_temporal_motion(None, w, h, b, a, C.byref(opts) if o else None, C.byref(topts) if to else None, mo, hi, ho, out)

    _in_order(make, name, [(b"null opts", dict(o=False)), (b"unknown flag bits", dict(f=2)), (b"9 iterations, at most 8", dict(it=9)),
                           (b"sigma_depth -1", dict(sz=-1.0)), (b"image 0 x", dict(w=0)), (b"unknown temporal flag bits", dict(tf=2)), (b"alpha 2", dict(al=2.0)),
                           (b"alpha_moments -0.5", dict(am=-0.5)), (b"depth_tolerance -1", dict(dt=-1.0)), (b"normal_cos 1.5", dict(nc=1.5)),
                           (b"max_history 0", dict(mh=0)), (b" camera:", dict(fov=0.0)), (b"history_out aliases", dict(ho=Mp)),
                           (b"16-byte aligned", dict(f=1, mo=Mp + 4))])
    for kw, word in ((dict(to=False), b"null topts"), (dict(a=None), b"null aov"), (dict(ho=None), b"null history_out"), (dict(out=None), b"null out"),
                     (dict(pfov=0.0), b"prev_camera:"), (dict(pfov=0.0, mo=None), b"prev_camera:"), (dict(ho=Ap), b"history_out aliases"),
                     (dict(ho=Mp - 48), b"history_out aliases"), (dict(ho=Mp + 16 * W * H - 16), b"history_out aliases"), (dict(f=1, hi=Ip + 4), b"16-byte aligned"),
                     (dict(f=1, ho=Hp + 4), b"16-byte aligned"), (dict(f=1, mo=Mp + 8), b"16-byte aligned")):
        _refused(make(**kw), name, word)
    for kw in (dict(), dict(f=1), dict(mo=None), dict(mo=Mp + 4), dict(f=1, mo=None, b=None, hi=None), dict(it=0, tf=0)):
        _refused(make(**kw), name, gate, status)
    assert all((a == 7.0).all() for a in arrays)


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_motion_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/motion.hip (the Makefile's flags): the two walk instantiations, the resolve and the one
    instantiation of k_dt_accumulate<true> - and nothing else: not the temporal unit's other kernels.  No kernel has scratch and the
    walk spills no register: a reload inside its loops would be a dependent memory trip per node.  LDS only in the walk: the path
    kernels' WgShared.  Registers and occupancy are printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert " motion " in var("HIP_UNITS") + " "
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "mv.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "motion.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_(mv_resolve|mv_walk<\w+>|dt_accumulate<\w+>)", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_dt_accumulate<true>", "k_mv_resolve", "k_mv_walk<false>", "k_mv_walk<true>"] and len(report) == 4, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert (v["LDS Size"] > 16 * 1024) == k.startswith("k_mv_walk") and v["LDS Size"] <= 20 * 1024, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_motion.h")).read()
    assert "atomic" not in src.replace("No global atomics", "") and "asm" not in src and "getenv" not in src
    assert "#pragma clang fp contract(off)" in src and "dt_camera_dir(" in src and "HJ_DEV v3 dt_camera_dir" not in src   # (included, not restated)
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "motion.hip")).read()
    # the walk's shell is hj_walk_segment.h's; k_mv_walk does not restate it
    segment = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_walk_segment.h")).read()
    assert "__shared__ WgShared sh;" in segment and "load_hot_nodes(sc, sh);" in segment and "trace_persistent<MODE, PAIRS>(" in segment
    assert "walk_segment<0, PAIRS>(" in src and "walk_hit_record(h)" in src and "walk_empty_range(" in src
    assert "__shared__ WgShared" not in src and "load_hot_nodes(" not in src and "trace_persistent<" not in src and "hit ? h.t" not in src


# ------------------------------------------------------------------------------------------------- the reference against itself

def _three_shapes(cam_pos=(0, 0, 0), rotation=(0, 0, 0, 1), fov=90.0, apart=0.0):
    """shape 0: a sphere; 1: a quad; 2: a triangle - all in front of a camera that looks down -z; apart: the sphere that far to the
    left and the triangle that far to the right, so that each is seen"""
    s = host.Scene()
    s.set_camera(cam_pos, rotation, fov)
    m = s.add_diffuse((0.5, 0.5, 0.5))
    s.add_sphere((-apart, 0, -3), 1.0, m)
    s.add_quad((-1, -1, -2), (2, 0, 0), (0, 2, 0), m)
    base = s.add_vertices([[-1 + apart, -1, -2], [1 + apart, -1, -2], [apart, 1, -2]], [[0, 0, 1]] * 3)
    s.add_triangle(base, base + 1, base + 2, m)
    return s.compile()


def _one(cs, prev, hit):
    ids, t, u, v = ([x] for x in hit)
    return M.render_motion(cs, prev, 1, 1, (np.array(ids, np.int32), np.array(t, F), np.array(u, F), np.array(v, F)))[0, 0]


def test_one_pixel_by_hand():
    """1 x 1, fov 90 (tan = 1), no rotation: d = (0, 0, -1), k = 0.5, and every number below is exact in float32"""
    cs = _three_shapes()
    assert T.tan_half(cs.desc.camera) == 1 and T.directions(cs.desc.camera, 1, 1)[0, 0].tolist() == [0, 0, -1]
    assert (len(cs.spheres), len(cs.quads), len(cs.triangles)) == (1, 1, 1)
    cam = cs.desc.camera
    # the sphere, hit at t = 2: P = (0, 0, -2), n = (0, 0, 1); before, centre (0, 1, -3) and radius 2: Pp = (0, 1, -1)
    #   c = (0, 1, -1): sx = 0 * 0.5 + 0.5, sy = (-1 / 1) * 0.5 + 0.5 = 0, zp = sqrt(2)
    r = _one(cs, M.Prev(cs, cam, spheres=[[0, 1, -3, 2]]), (0, 2.0, 0, 0))
    assert r[0:3].tolist() == [0.5, 0.0, np.sqrt(F(2))] and r.view(U)[3] == 0
    # the quad at (u, v) = (0.5, 0.5), moved by +0.5 along x: Pp = (0.5, 0, -2): sx = (0.5 / 2) * 0.5 + 0.5 = 0.625, zp = sqrt(4.25)
    r = _one(cs, M.Prev(cs, cam, quads=[[-0.5, -1, -2, 0, 2, 0, 0, 0, 0, 2, 0, 0]]), (1, 2.0, 0.5, 0.5))
    assert r[0:3].tolist() == [0.625, 0.5, np.sqrt(F(4.25))] and r.view(U)[3] == 1
    # ... and sheared: edge2 (1, 2, 0) at v = 0.5 adds 0.5 along x: Pp = (1, 0, -2): sx = 0.75
    r = _one(cs, M.Prev(cs, cam, quads=[[-0.5, -1, -2, 0, 2, 0, 0, 0, 1, 2, 0, 0]]), (1, 2.0, 0.5, 0.5))
    assert r[0:2].tolist() == [0.75, 0.5]
    # the triangle at (u, v) = (0.25, 0.5), l0 = 0.25, all of it pushed back to z = -4: Pp = (0, 0, -4): the centre, zp = 4
    verts = np.array(cs.vertices, F)
    verts[:, 2] = -4
    r = _one(cs, M.Prev(cs, cam, vertices=verts), (2, 2.0, 0.25, 0.5))
    assert r[0:3].tolist() == [0.5, 0.5, 4.0] and r.view(U)[3] == 2
    # a kind that did not move stands still: the quad's centre through an identical camera is the pixel's centre, at its own t
    r = _one(cs, M.Prev(cs, cam), (1, 2.0, 0.5, 0.5))
    assert r[0:3].tolist() == [0.5, 0.5, 2.0]
    # a previous camera the point lies behind, a miss, an id outside the scene: no previous position
    behind = T.camera((0, 0, -10))
    for prev, hit in ((M.Prev(cs, behind), (1, 2.0, 0.5, 0.5)), (M.Prev(cs, cam), (-1, 0, 0, 0)), (M.Prev(cs, cam), (3, 2.0, 0.5, 0.5))):
        assert _one(cs, prev, hit).view(U).tolist() == [0, 0, 0, 0xFFFFFFFF]
    # a previous camera of half the tangent doubles the offset from the centre: fov 2 atan(0.5)
    narrow = T.camera(fov=float(np.degrees(2 * np.arctan(0.5))))
    assert abs(float(T.tan_half(narrow)) - 0.5) < 1e-7
    r = _one(cs, M.Prev(cs, narrow, quads=[[-0.5, -1, -2, 0, 2, 0, 0, 0, 0, 2, 0, 0]]), (1, 2.0, 0.5, 0.5))
    assert abs(r[0] - 0.75) < 1e-6 and r[1] == 0.5


def _rot64(q, v, inverse=False):
    """v + 2 qw (qv x v) + 2 qv x (qv x v), the textbook form, float64"""
    qv, qw = np.array(q[0:3], np.float64) * (-1.0 if inverse else 1.0), np.float64(q[3])
    t = 2.0 * np.cross(qv, v)
    return v + qw * t + np.cross(qv, t)


@pytest.mark.parametrize("camera", ["identical", "translated", "rotated"])
def test_the_geometry_in_float64(oracle, camera):
    """A translated sphere, a quad moved and sheared, a triangle whose three vertices moved independently, seen through previous
    cameras that are identical, translated and rotated.  Per hit pixel the surface point is found from the GEOMETRY in float64 - the
    point on the centre ray at the oracle's t; on the sphere its direction from the centre, on the quad and the triangle its
    coordinates solved from the point itself, not taken from the hit's (u, v) - carried onto the previous shape and through the
    previous pinhole by the textbook rotation: image y downwards, the camera looking down its -z, pixel centres at (x + 1/2,
    y + 1/2).  (sx, sy) must agree to half a pixel - the bound of the static projection's half-pixel test: a wrong convention, axis
    sign or conjugate is off by more - and zp to 1e-4 relative."""
    W, H, fov = 48, 36, 70.0
    q = T.axis_angle((0.2, 1.0, -0.1), -6)
    cs = _three_shapes((0.1, -0.05, 1.5), q, fov, apart=2.0)
    cam = cs.desc.camera
    prev_cam = {"identical": cam, "translated": T.camera((0.5, 0.2, 1.9), q, fov), "rotated": T.camera((0.1, -0.05, 1.5), T.axis_angle((0.5, 1.0, 0.3), 19), 55.0)}[camera]
    verts = np.array(cs.vertices, F)
    verts[:, 0:3] += np.array([[0.3, -0.1, 0.2], [-0.2, 0.25, -0.3], [0.1, 0.1, 0.4]], F)
    prev = M.Prev(cs, prev_cam, spheres=[[-1.7, 0.2, -3.4, 1.0]], quads=[[-1.2, -0.9, -2.3, 0, 2.1, 0.2, 0, 0, 0.4, 1.9, -0.3, 0]], vertices=verts)
    rays = M.centre_rays(cam, W, H)
    ids, t, u, v = oracle.intersect(cs, rays)
    got = M.render_motion(cs, prev, W, H, (ids, t, u, v))
    ids = ids.reshape(H, W)
    assert all((ids == k).sum() > 30 for k in (0, 1, 2)) and (ids < 0).sum() > 30
    # float64, from the geometry
    tan = np.tan(np.radians(fov / 2))
    y, x = np.mgrid[0:H, 0:W]
    local = np.stack([(x + 0.5 - W / 2) * tan / (W / 2), -(y + 0.5 - H / 2) * tan / (W / 2), -np.ones((H, W))], -1)
    d = _rot64(list(cam.rotation), local)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    P = np.array(list(cam.position)[0:3], np.float64) + t.reshape(H, W, 1).astype(np.float64) * d
    Pp = np.zeros((H, W, 3))
    m = ids == 0
    c0, r0, c1, r1 = cs.spheres[0, 0:3].astype(np.float64), float(cs.spheres[0, 3]), prev.spheres[0, 0:3].astype(np.float64), float(prev.spheres[0, 3])
    Pp[m] = c1 + (P[m] - c0) / r0 * r1
    m = ids == 1
    cur, was = cs.quads[0].astype(np.float64), prev.quads[0].astype(np.float64)
    uv = np.linalg.lstsq(np.stack([cur[4:7], cur[8:11]], 1), (P[m] - cur[0:3]).T, rcond=None)[0].T
    Pp[m] = was[0:3] + uv[:, 0:1] * was[4:7] + uv[:, 1:2] * was[8:11]
    m = ids == 2
    a, b, c = (cs.vertices[i, 0:3].astype(np.float64) for i in cs.triangles[0])
    pa, pb, pc = (verts[i, 0:3].astype(np.float64) for i in cs.triangles[0])
    uv = np.linalg.lstsq(np.stack([b - a, c - a], 1), (P[m] - a).T, rcond=None)[0].T
    Pp[m] = pa + uv[:, 0:1] * (pb - pa) + uv[:, 1:2] * (pc - pa)
    ptan = np.tan(np.radians(float(prev_cam.fov) / 2))
    loc = _rot64(list(prev_cam.rotation), Pp - np.array(list(prev_cam.position)[0:3], np.float64), inverse=True)
    with np.errstate(all="ignore"):
        sx = (loc[..., 0] / -loc[..., 2]) * (W / 2) / ptan + W / 2
        sy = (-loc[..., 1] / -loc[..., 2]) * (W / 2) / ptan + H / 2
    zp = np.linalg.norm(Pp - np.array(list(prev_cam.position)[0:3], np.float64), axis=-1)
    hit = ids >= 0
    front = hit & (loc[..., 2] < 0)
    assert front.sum() == hit.sum()                                     # (the three shapes stay in front of every previous camera here)
    none = got.view(U)[..., 3] == M.NONE
    assert (none == ~hit).all() and (got.view(U)[..., 3][hit] == ids[hit]).all() and not got[none][:, 0:3].any()
    ex, ey = np.abs(got[..., 0] - sx)[hit].max(), np.abs(got[..., 1] - sy)[hit].max()
    ez = (np.abs(got[..., 2] - zp) / zp)[hit].max()
    print(f"{camera}: max |sx| error {ex:.3g}, |sy| {ey:.3g} pixels, zp {ez:.3g} relative")
    assert ex <= 0.5 and ey <= 0.5 and ez <= 1e-4
    if camera == "identical":                                           # the shapes did move: the records are not the pixels' own centres
        assert (np.abs(got[..., 0] - (x + 0.5))[hit] > 1).any()
        still = M.render_motion(cs, M.Prev(cs, cam), W, H, (ids.ravel(), t, u, v))
        assert np.abs(still[..., 0] - (x + 0.5))[hit].max() < 0.01 and np.abs(still[..., 1] - (y + 0.5))[hit].max() < 0.01


# ------------------------------------------------------------------------------------------------------------------- the anchor

def test_the_static_projection_s_own_values_give_the_static_result_word_for_word():
    """motion_ref.run, fed an image that holds the static projection's own (sx, sy, zp) - HJ_MOTION_NONE where c.z < 0 is false -,
    equals temporal_ref.run in every word of out and history_out: the two texts of REPROJECT's taps are one"""
    from test_denoise_gpu import frame
    from test_denoise_temporal_gpu import CAM, PREV, history
    for (W, H), names in (((37, 13), sorted(PREV)), ((70, 41), ("translated", "turned"))):
        beauty, aov = frame(W, H)
        z = D.prepare(beauty, aov)[5]
        for name in names:
            motion = M.static_motion(CAM, PREV[name], z, W, H)
            front = T.project(CAM, PREV[name], z, W, H)[0]
            assert ((motion.view(U)[..., 3] == M.NONE) == ~front).all() and front.any() == (name != "turned")
            for it, kw in ((2, {}), (0, dict(feedback=False, max_history=5, depth_tolerance=0.06))):
                want = T.run(beauty, aov, CAM, PREV[name], history(W, H), it, **kw)
                got = M.run(beauty, aov, motion, history(W, H), it, **kw)
                assert (got[0].view(U) == want[0].view(U)).all() and (got[1].view(U) == want[1].view(U)).all(), (W, H, name, it)
        none = np.zeros((H, W, 4), F)
        none.view(U)[..., 3] = M.NONE
        first = T.run(beauty, aov, CAM, CAM, None, 2)
        got = M.run(beauty, aov, none, history(W, H), 2)
        assert (got[0].view(U) == first[0].view(U)).all() and (got[1].view(U) == first[1].view(U)).all()
