"""hj_render_motion and hj_denoise_frame_temporal_motion on the GPU against motion_ref - the two contracts restated in numpy - bit for
bit on every word.  The motion image over the oracle's first hits of the centre rays: every kind moved, a kind unmoved, seven previous
cameras and one that leaves part of the scene behind it, from 1 x 1 to a launch of many workgroups, on each route into an upload and
after hj_scene_update_shapes; centre rays outside general position; the device forms; the unmoved anchor against hj_trace_rays.  The
temporal call over test_denoise_temporal_gpu's fabricated frames and histories with fabricated motion images in the three kernel
forms, its three GPU-to-GPU anchors, and the one behavioural condition: a mover keeps its history, and only with motion."""
import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import temporal_ref as T
from hijiki_amd import abi, device, host
from refit_scenes import Deformation, refit_numpy, shape_boxes
from test_denoise_gpu import BIG, big_frame, frame, same_bits
from test_denoise_temporal_gpu import CAM, FORMS, PREV, forms, history   # noqa: F401  (forms: the fixture)

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SIZES = [(1, 1), (7, 1), (1, 7), (37, 13), (70, 41), (256, 130)]        # 256 x 130: 33280 entries in workgroups of 256 - walk_wg_rays' floor


@pytest.fixture(scope="module")
def r():
    with device.Renderer(0) as ctx:
        yield ctx


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    assert all(hasattr(device.lib(), n) and n in device.EXPORTS for n in ("hj_render_motion", "hj_denoise_frame_temporal_motion"))


def _scene(rotation=None):
    """the box with the two spheres - a triangle mesh - and two quads hung into it: spheres, quads and triangles; rotation: another
    camera rotation"""
    s = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280)
    green = s.add_diffuse((0.2, 0.6, 0.3))
    s.add_quad((-0.8, 1.1, 0.3), (0.6, 0.0, 0.1), (0.05, 0.5, 0.0), green)
    s.add_quad((0.15, 0.7, 0.5), (0.5, 0.1, -0.2), (-0.1, 0.6, 0.1), green)
    if rotation is not None:
        c = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile().desc.camera
        s.set_camera(list(c.position)[0:3], rotation, c.fov)
    cs = s.compile()
    assert len(cs.spheres) and len(cs.quads) and len(cs.triangles)
    return cs


def _cam(cs, position=None, then=None, fov=None):
    """cs's camera with another position, a further rotation (axis, degrees) or another fov"""
    c = cs.desc.camera
    q = np.array(list(c.rotation), np.float64)
    if then is not None:
        t = np.array(T.axis_angle(*then), np.float64)
        q = np.array([*(np.cross(q[0:3], t[0:3]) + t[0:3] * q[3] + q[0:3] * t[3]), q[3] * t[3] - q[0:3] @ t[0:3]])
    return T.camera(list(c.position)[0:3] if position is None else position, [float(F(v)) for v in q], c.fov if fov is None else fov)


def _moved(cs, seed, kinds=("spheres", "quads", "vertices")):
    """previous arrays: every coordinate of the named kinds off by up to 0.03, radii rescaled; the other kinds None (unmoved)"""
    rng = np.random.default_rng(seed)
    out = {}
    for k in kinds:
        a = np.array(getattr(cs, k), F)
        a = a + rng.uniform(-0.03, 0.03, a.shape).astype(F)
        if k == "spheres":
            a[:, 3] = np.array(cs.spheres, F)[:, 3] * rng.uniform(0.8, 1.2, len(a)).astype(F)
        out[k] = a
    return out


def _cameras(cs):
    p = np.array(list(cs.desc.camera.position)[0:3], np.float64)
    return {"identical": _cam(cs), "translated": _cam(cs, position=p + (0.2, -0.1, 0.15)), "about x": _cam(cs, then=((1, 0, 0), 2.0)),
            "about y": _cam(cs, then=((0, 1, 0), -3.0)), "about z": _cam(cs, then=((0, 0, 1), 5.0)), "another fov": _cam(cs, fov=cs.desc.camera.fov + 9.0),
            "turned": _cam(cs, then=((0, 1, 0), 180.0))}


_HITS = {}


def hits_of(oracle, cs, W, H, key):
    """the oracle's first hits of the centre rays, once per (scene state, size)"""
    if (key, W, H) not in _HITS:
        _HITS[(key, W, H)] = oracle.intersect(cs, M.centre_rays(cs.desc.camera, W, H))[0:4]
    return _HITS[(key, W, H)]


def check(r, oracle, cs, prev, W, H, key, what):
    want = M.render_motion(cs, prev, W, H, hits_of(oracle, cs, W, H, key))
    got = r.render_motion(prev, W, H)
    same_bits(got, want, what)
    return want


# -------------------------------------------------------------------------------------------------------------- hj_render_motion

@pytest.mark.parametrize("size", SIZES)
def test_every_size_with_every_kind_moved(r, oracle, size):
    W, H = size
    cs = _scene()
    r.upload_scene(cs)
    prev = M.Prev(cs, _cameras(cs)["translated"], **_moved(cs, 5))
    want = check(r, oracle, cs, prev, W, H, "rest", f"{W} x {H}")
    ids = want.view(U)[..., 3]
    if W * H > 2000:
        ns, nq = len(cs.spheres), len(cs.quads)
        assert (ids < ns).sum() > 50 and ((ids >= ns) & (ids < ns + nq)).sum() > 50 and ((ids >= ns + nq) & (ids != M.NONE)).sum() > 50


def test_every_previous_camera_and_every_unmoved_kind(r, oracle):
    W, H = 70, 41
    cs = _scene()
    r.upload_scene(cs)
    moved = _moved(cs, 6)
    for name, cam in _cameras(cs).items():
        want = check(r, oracle, cs, M.Prev(cs, cam, **moved), W, H, "rest", name)
        none = want.view(U)[..., 3] == M.NONE
        assert none.all() if name == "turned" else (~none).sum() > 1000, name
    for left_out in ("spheres", "quads", "vertices"):
        kept = {k: v for k, v in moved.items() if k != left_out}
        check(r, oracle, cs, M.Prev(cs, _cameras(cs)["about y"], **kept), W, H, "rest", f"{left_out} unmoved")
    check(r, oracle, cs, M.Prev(cs, _cameras(cs)["translated"]), W, H, "rest", "nothing moved")
    # a previous camera inside the box, looking sideways: hits behind it beside hits in front of it
    side = _cam(cs, position=(0.0, 1.0, 0.0), then=((0, 1, 0), 90.0))
    want = check(r, oracle, cs, M.Prev(cs, side, **moved), W, H, "rest", "a camera with hits behind it")
    hit = np.asarray(hits_of(oracle, cs, W, H, "rest")[0]).reshape(H, W) >= 0
    none = want.view(U)[..., 3] == M.NONE
    assert (none & hit).sum() > 100 and (~none).sum() > 100
    edge = (none[:, 1:] != none[:, :-1]) & hit[:, 1:] & hit[:, :-1]
    assert edge.any()                                                   # (a hit behind the camera beside one that is not)


@pytest.mark.parametrize("route", ["host tree", "device-built tree", "resident tree"])
def test_every_route_into_an_upload(r, oracle, route):
    W, H = 70, 41
    cs = _scene()
    if route == "device-built tree":
        cs.set_bvh(r.build_bvh(cs))
        r.upload_scene(cs)
    elif route == "resident tree":
        r.build_bvh(cs, keep_on_device=True)
        cs.set_bvh(r.read_device_bvh().copy())
        r.upload_scene(cs, device_tree=True)
    else:
        r.upload_scene(cs)
    check(r, oracle, cs, M.Prev(cs, _cameras(cs)["about x"], **_moved(cs, 7)), W, H, route, route)


def test_after_an_update_the_current_shapes_are_the_updated_ones(r, oracle):
    """the ordinary frame loop: move, hj_scene_update_shapes, ask for motion against the old arrays and the old camera"""
    W, H = 70, 41
    cs = _scene()
    topo = cs.bvh.copy()
    r.upload_scene(cs)
    old = dict(spheres=cs.spheres.copy(), quads=cs.quads.copy(), vertices=cs.vertices.copy())
    old_cam = _cam(cs)
    rest = check(r, oracle, cs, M.Prev(cs, old_cam), W, H, "rest", "before the update")
    d = Deformation(cs, seed=8)
    d.apply(0.03, t=0.4)
    r.update_shapes(cs)
    cs.set_bvh(refit_numpy(topo, shape_boxes(cs)))                      # (the oracle walks the refitted tree)
    want = check(r, oracle, cs, M.Prev(cs, old_cam, **old), W, H, "updated", "after the update")
    assert (want != rest).any()
    check(r, oracle, cs, M.Prev(cs, old_cam, spheres=old["spheres"]), W, H, "updated", "after the update, spheres alone")
    cs.set_bvh(topo)
    d.restore()


def test_centre_rays_outside_general_position(r, oracle):
    """an identity rotation with odd width and height: the centre column and row have an exactly zero direction component, and those
    rays walk the second copy of the tree"""
    W, H = 37, 13
    cs = _scene(rotation=(0, 0, 0, 1))
    d = T.directions(cs.desc.camera, W, H)
    assert (d[:, W // 2, 0] == 0).all() and (d[H // 2, :, 1] == 0).all()
    r.upload_scene(cs)
    want = check(r, oracle, cs, M.Prev(cs, _cameras(cs)["translated"], **_moved(cs, 9)), W, H, "identity", "identity rotation")
    assert (want.view(U)[:, W // 2, 3] != M.NONE).any() and (want.view(U)[H // 2, :, 3] != M.NONE).any()


def test_device_forms_give_the_same_bits_and_leave_nothing_stale(r, oracle):
    torch = pytest.importorskip("torch")
    cs = _scene()
    r.upload_scene(cs)
    moved = _moved(cs, 10)
    cam = _cameras(cs)["about z"]
    dev = torch.device("cuda", r.device)
    arrays = {k: torch.from_numpy(v.copy()).to(dev) for k, v in moved.items()}
    for W, H in ((70, 41), (37, 13)):                                   # the smaller image after the larger one
        want = check(r, oracle, cs, M.Prev(cs, cam, **moved), W, H, "rest", f"host arrays {W} x {H}")
        bare = M.Prev(cs, cam)                                          # (its host arrays are NOT what the call may read)
        same_bits(r.render_motion(bare, W, H, device_arrays=arrays), want, f"device shapes {W} x {H}")
        out = r.render_motion(bare, W, H, device_arrays=arrays, device=True)
        assert out.is_cuda and tuple(out.shape) == (H, W, 4)
        same_bits(out.cpu().numpy(), want, f"device shapes and device out {W} x {H}")
        same_bits(r.render_motion(M.Prev(cs, cam, **moved), W, H, device=True).cpu().numpy(), want, f"device out {W} x {H}")
        assert (device.motion_ids(out) == want.view(U)[..., 3]).all()
    same_bits(r.render_motion(bare, 37, 13, device_arrays={"spheres": arrays["spheres"]}),
              check(r, oracle, cs, M.Prev(cs, cam, spheres=moved["spheres"]), 37, 13, "rest", "spheres alone"), "device spheres alone")
    assert all((arrays[k].cpu().numpy() == moved[k]).all() for k in moved)


def test_unmoved_anchor(r):
    """prev equal to the uploaded arrays and camera: every hit pixel stays where it is, and word 3 is hj_trace_rays' id of the same ray"""
    W, H = 70, 41
    cs = _scene()
    r.upload_scene(cs)
    ids = r.trace_rays(M.centre_rays(cs.desc.camera, W, H))[0].reshape(H, W)
    y, x = np.mgrid[0:H, 0:W]
    for prev in (M.Prev(cs, _cam(cs)), M.Prev(cs, _cam(cs), spheres=cs.spheres.copy(), quads=cs.quads.copy(), vertices=cs.vertices.copy())):
        got = r.render_motion(prev, W, H)
        hit = ids >= 0
        assert hit.sum() > 2000 and (device.motion_ids(got)[hit] == ids[hit].astype(U)).all() and (device.motion_ids(got)[~hit] == M.NONE).all()
        assert np.abs(got[..., 0] - (x + 0.5))[hit].max() <= 0.5 and np.abs(got[..., 1] - (y + 0.5))[hit].max() <= 0.5


def test_refusals_behind_the_gate(r):
    cs = _scene()
    with device.Renderer(0) as empty:
        with pytest.raises(abi.HijikiError) as e:
            empty.render_motion(M.Prev(cs, _cam(cs)), 8, 8)
        assert e.value.status == abi.HJ_ERR_STATE
    r.upload_scene(cs)
    fewer = M.Prev(cs, _cam(cs))
    fewer.desc.num_vertices -= 1
    bad = np.array(cs.spheres, F)
    bad[0, 3] = np.inf
    for prev, word in ((fewer, "vertices"), (M.Prev(cs, _cam(cs), spheres=bad), "not finite")):
        with pytest.raises(abi.HijikiError) as e:
            r.render_motion(prev, 8, 8)
        assert e.value.status == abi.HJ_ERR_INVALID and "hj_render_motion:" in str(e.value) and word in str(e.value), str(e.value)


# ----------------------------------------------------------------------------------------------- hj_denoise_frame_temporal_motion

_MOTIONS = {}


def motions(W, H):
    """fabricated motion images for frame(W, H): shifts by whole and by fractional pixels, positions outside the image,
    HJ_MOTION_NONE holes, and zp on both sides of the depth tolerance of 0.1 around the history's depths"""
    if (W, H) not in _MOTIONS:
        rng = np.random.default_rng([W, H, 2029])
        z = D.prepare(*frame(W, H))[5]
        y, x = np.mgrid[0:H, 0:W]
        out = {}
        for name, (dx, dy) in (("whole", (2.0, -1.0)), ("fractional", (-1.37, 0.6)), ("outside and holes", (0.25, 0.25))):
            m = np.zeros((H, W, 4), F)
            m[..., 0], m[..., 1] = x + 0.5 + dx, y + 0.5 + dy
            m[..., 2] = np.where(z > 0, z, 4.0) * rng.choice(np.array([1, 1, 1, 1.04, 0.95, 1.2, 0.85], F), (H, W))
            m.view(U)[..., 3] = rng.integers(0, 50, (H, W))
            if name == "outside and holes":
                far = rng.random((H, W)) < 0.2
                m[..., 0][far] = rng.choice(np.array([-40.0, -1.25, -0.5, W + 0.25, W + 30.0], F), int(far.sum()))
                m[..., 1][rng.random((H, W)) < 0.1] = H + 7.5
                holes = rng.random((H, W)) < 0.15
                m[holes] = 0
                m.view(U)[holes, 3] = M.NONE
            out[name] = m
        _MOTIONS[(W, H)] = out
    return _MOTIONS[(W, H)]


def both(got, w, what):
    same_bits(got[0], w[0], what + ": out")
    same_bits(got[1], w[1], what + ": history_out")


@pytest.mark.parametrize("step", FORMS)
@pytest.mark.parametrize("size", [(1, 1), (7, 1), (1, 7), (37, 13), (70, 41)])
def test_temporal_motion_in_every_form(forms, size, step):            # noqa: F811
    W, H = size
    beauty, aov = frame(W, H)
    it = 5 if (W, H) == (70, 41) else 2
    for name, m in motions(W, H).items():
        want = M.run(beauty, aov, m, history(W, H), it)
        both(forms[step].denoise_frame_temporal(aov, CAM, PREV["translated"], history(W, H), beauty, it, motion=m), want, f"{W} x {H}, {name}, form {step}")
        if W * H > 2000:
            s = M.run(beauty, aov, m, history(W, H), 0, keep=True)[2]
            assert 100 < s["has"].sum() < s["G"].sum() - 100, name          # (taps pass and taps fail)


def test_temporal_motion_with_lattice_tiles_beyond_one_a_residue_class(forms):       # noqa: F811
    """test_denoise_gpu's 517 x 131 frame through a motion image, the LDS form at every step up to 16"""
    W, H = BIG
    beauty, aov = big_frame()
    m = motions(W, H)["fractional"]
    out, hist, s = M.run(beauty, aov, m, history(W, H), 5, keep=True)
    assert 10000 < s["has"].sum() < s["G"].sum() - 10000 and s["has"][128:, 480:].any()
    both(forms["128"].denoise_frame_temporal(aov, CAM, PREV["translated"], history(W, H), beauty, 5, motion=m), (out, hist), "517 x 131, fractional, form 128")


def test_temporal_motion_anchors(forms):                               # noqa: F811
    """motion = NULL is hj_denoise_frame_temporal; a motion image of the static projection's own values is it too; an image of
    HJ_MOTION_NONE alone is hj_denoise_frame - GPU against GPU, and device tensors against host arrays"""
    torch = pytest.importorskip("torch")
    W, H = 70, 41
    beauty, aov = frame(W, H)
    z = D.prepare(beauty, aov)[5]
    none = np.zeros((H, W, 4), F)
    none.view(U)[..., 3] = M.NONE
    for step in ("0", "128"):
        r = forms[step]
        for name in ("translated", "about z", "turned"):
            static = r.denoise_frame_temporal(aov, CAM, PREV[name], history(W, H), beauty, 3)
            both(r.denoise_frame_temporal(aov, CAM, PREV[name], history(W, H), beauty, 3, motion=None), static, f"motion None, {name}, form {step}")
            both(r.denoise_frame_temporal(aov, CAM, PREV[name], history(W, H), beauty, 3, motion=M.static_motion(CAM, PREV[name], z, W, H)), static,
                 f"the static projection's own values, {name}, form {step}")
        got = r.denoise_frame_temporal(aov, CAM, CAM, history(W, H), beauty, 5, motion=none)
        same_bits(got[0], r.denoise_frame(aov, beauty, 5), f"all NONE, form {step}")
        same_bits(got[1], r.denoise_frame_temporal(aov, CAM, CAM, None, beauty, 5)[1], f"all NONE: history_out, form {step}")
    r = forms[None]
    m = motions(W, H)["fractional"]
    dev = torch.device("cuda", r.device)
    tb, ta, th, tm = (torch.from_numpy(np.array(a)).to(dev) for a in (beauty, aov, history(W, H), m))
    out, hist = r.denoise_frame_temporal(ta, CAM, CAM, th, tb, 3, device=True, motion=tm)
    both((out.cpu().numpy(), hist.cpu().numpy()), M.run(beauty, aov, m, history(W, H), 3), "device tensors")
    same_bits(tm.cpu().numpy(), m, "the motion tensor afterwards")


# ------------------------------------------------------------------------------------------------------ the behavioural condition

def _mover_scene(k):
    """A wall quad 8 units in front of a camera at the origin (no rotation, fov 90: at 64 x 64 a pixel is 1 / 8 unit at distance 4)
    and a 1 x 1 quad hovering 4 units in front of it - depths 4 and 8, far apart against a tolerance of 0.1 -, which moves 3 pixels
    to the right a frame.  (An emissive quad behind the camera: never seen.)"""
    s = host.Scene()
    s.set_camera((0, 0, 0), (0, 0, 0, 1), 90.0)
    grey, light = s.add_diffuse((0.5, 0.5, 0.5)), s.add_emissive((5, 5, 5))
    s.add_quad((-10, -10, -8), (20, 0, 0), (0, 20, 0), grey)
    s.add_quad((-2.0 + 0.375 * k, -0.5, -4), (1, 0, 0), (0, 1, 0), grey)
    s.add_quad((-1, -1, 5), (2, 0, 0), (0, 2, 0), light)
    return s.compile()


def test_a_mover_keeps_its_history_with_motion_and_loses_it_without(r, oracle):
    W = H = 64
    frames = 4
    rng = np.random.default_rng(11)
    cam = _mover_scene(0).desc.camera
    scenes, masks, aovs, beauties = [], [], [], []
    for k in range(frames):
        cs = _mover_scene(k)
        ids, t, u, v = oracle.intersect(cs, M.centre_rays(cam, W, H))
        assert (ids >= 0).all()
        aov = np.zeros((H, W, 12), F)
        aov[..., 0:3], aov[..., 3], aov[..., 6], aov[..., 7], aov[..., 11] = 0.5, 1, 1, t.reshape(H, W), 1
        beauty = np.concatenate([rng.uniform(0.2, 1.0, (H, W, 3)), np.ones((H, W, 1))], -1).astype(F)
        scenes.append((cs, (ids, t, u, v)))
        masks.append(ids.reshape(H, W) == 1)
        aovs.append(aov)
        beauties.append(beauty)
        assert masks[k].sum() == 64                                       # an 8 x 8 footprint
    # the reference alone, before any GPU is asked
    hm = hs = None
    motion_of = []
    for k in range(frames):
        cs, hits = scenes[k]
        prev = M.Prev(cs, cam, quads=scenes[k - 1][0].quads if k else None)
        m = M.render_motion(cs, prev, W, H, hits)
        motion_of.append(m)
        _, hm, sm = M.run(beauties[k], aovs[k], m, hm, 0, keep=True)
        _, hs, ss = T.run(beauties[k], aovs[k], cam, cam, hs, 0, keep=True)
        if k == 0:
            continue
        fx, fy = np.floor(m[..., 0] - F(0.5)).astype(int), np.floor(m[..., 1] - F(0.5)).astype(int)
        was = masks[k - 1]
        inside = np.zeros((H, W), bool)
        ok = masks[k] & (fx >= 0) & (fx + 1 < W) & (fy >= 0) & (fy + 1 < H)
        inside[ok] = was[fy[ok], fx[ok]] & was[fy[ok], fx[ok] + 1] & was[fy[ok] + 1, fx[ok]] & was[fy[ok] + 1, fx[ok] + 1]
        fresh = inside & ~was                                           # the mover newly covers them in frame k
        assert inside.sum() >= 30 and fresh.sum() >= 10, (k, inside.sum(), fresh.sum())
        assert np.abs(sm["N"][inside] - (k + 1)).max() < 1e-4, (k, sm["N"][inside])
        assert (ss["N"][fresh] == 1).all(), k
    # the GPU: the same motion images, and the same history word for word
    gm = gs = None
    for k in range(frames):
        cs = scenes[k][0]
        r.upload_scene(cs)
        prev = M.Prev(cs, cam, quads=scenes[k - 1][0].quads if k else None)
        m = r.render_motion(prev, W, H)
        same_bits(m, motion_of[k], f"frame {k}: motion")
        _, gm = r.denoise_frame_temporal(aovs[k], cam, cam, gm, beauties[k], 0, motion=m)
        _, gs = r.denoise_frame_temporal(aovs[k], cam, cam, gs, beauties[k], 0)
    same_bits(gm, hm, "the history with motion")
    same_bits(gs, hs, "the history of the static call")
    same_bits(gm[..., 3], hm[..., 3], "the N plane")
