"""hj_render_motion_followed on the GPU against motion_follow_ref - the contract restated in numpy - bit for bit on every word: the
box with the spheres and the "rich" scene (chains up to length 5, chains that leave) with every shape kind moved, from 1 x 1 to a
size above a compaction tile, at max_follow 1, 2 and 8, the chains made by alternating the restatement with hj_trace_rays itself;
the anchors against hj_render_motion; the device forms; the walk's other forms; every route into an upload and the scene after
hj_scene_update_shapes; and the one behavioural condition: with followed guides a mirror keeps its history through the followed
motion image, and loses it through the first-hit one.  No tolerance anywhere."""
import numpy as np
import pytest

import follow_ref as R
import motion_follow_ref as MF
import motion_ref as M
import path_query_ref as P
import temporal_ref as T
from hijiki_amd import abi, device, host
from refit_scenes import Deformation
from test_follow_gpu import gpu_trace, same_bits
from test_motion_gpu import _cam, _cameras, _moved, _mover_scene

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SIZES = [(1, 1), (7, 1), (37, 13), (70, 41), (130, 67)]                 # 130 x 67 = 8710 pixels: 35 compaction tiles, the last one ragged
FOLLOWS = (1, 2, 8)


@pytest.fixture(scope="module")
def r():
    with device.Renderer(0) as ctx:
        yield ctx


@pytest.fixture(autouse=True)
def _the_library_has_the_call():
    assert hasattr(device.lib(), "hj_render_motion_followed") and "hj_render_motion_followed" in device.EXPORTS


def _prev(cs, seed=5, camera="translated"):
    kinds = [k for k in ("spheres", "quads", "vertices") if len(getattr(cs, k))]
    return M.Prev(cs, _cameras(cs)[camera], **_moved(cs, seed, kinds))


def _specular_first(cs, first):
    ids = first[:, 0].copy().view(np.int32).astype(np.int64)
    tag = np.zeros(len(ids), U)
    ok = ids >= 0
    tag[ok] = np.asarray(cs.materials, U)[ids[ok]] >> abi.MATERIAL_TAG_SHIFT
    return ok & ((tag == abi.MAT_MIRROR) | (tag == abi.MAT_DIELECTRIC))


# ------------------------------------------------------------------------------------------------------- against the restatement

def test_the_premise_on_the_reference_alone(oracle):
    """before any GPU is asked: "rich" at 8 reaches a chain length of at least 3, some chain ends with HJ_MOTION_LEFT, and chains end
    on every shape kind; the box has chains, none longer than 1"""
    cs = P.scene("rich")
    want, det = MF.render_motion_followed(cs, _prev(cs), 70, 41, 8, R.oracle_trace(cs), detail=True)
    ids = MF.ids_of(want)[det["went"]]
    ns, nq = len(cs.spheres), len(cs.quads)
    assert det["length"].max() >= 3 and (ids == MF.LEFT).sum() >= 1 and det["left"].sum() == (ids == MF.LEFT).sum()
    assert (ids < ns).any() and ((ids >= ns) & (ids < ns + nq)).any() and ((ids >= ns + nq) & (ids < cs.num_shapes)).any()
    cs = P.scene("cbox")
    det = MF.render_motion_followed(cs, _prev(cs), 70, 41, 8, R.oracle_trace(cs), detail=True)[1]
    assert det["went"].sum() > 50 and det["length"].max() == 1


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", ["cbox", "rich"])
def test_every_size_and_depth_with_every_kind_moved(r, scene, size):
    W, H = size
    cs = P.scene(scene)
    r.upload_scene(cs)
    prev = _prev(cs)
    for mf in FOLLOWS:
        want, det = MF.render_motion_followed(cs, prev, W, H, mf, gpu_trace(r), detail=True)
        same_bits(r.render_motion(prev, W, H, follow=mf), want, f"{scene} {W} x {H}, max_follow {mf}")
        if W * H > 2000:
            assert det["went"].sum() > 50 and (det["count"].max() >= min(mf, 3) or scene == "cbox")   # (no chain of "rich" takes all 8)
            moved = want.view(U)[det["went"]] != MF.render_motion_followed(cs, M.Prev(cs, prev.camera), W, H, mf, gpu_trace(r)).view(U)[det["went"]]
            assert moved.any()                                          # (the previous shapes do show in the followed records)


def test_anchors_against_render_motion(r):
    W, H = 70, 41
    for scene in ("cbox", "rich"):
        cs = P.scene(scene)
        r.upload_scene(cs)
        prev = _prev(cs, 6, "about y")
        base = r.render_motion(prev, W, H)
        same_bits(r.render_motion(prev, W, H, follow=0), base, f"{scene}: follow = 0")
        first = gpu_trace(r)(M.centre_rays(cs.desc.camera, W, H))[0]
        spec = _specular_first(cs, first).reshape(H, W)
        assert 50 < spec.sum() < W * H - 50
        for mf in FOLLOWS:
            got = r.render_motion(prev, W, H, follow=mf)
            same_bits(got[~spec], base[~spec], f"{scene}: the pixels whose first hit is not specular, max_follow {mf}")
            assert (got.view(U)[spec] != base.view(U)[spec]).any()
    cs = _mover_scene(1)                                                # diffuse and emissive quads alone
    r.upload_scene(cs)
    prev = M.Prev(cs, _cam(cs, position=(0.1, 0.0, 0.2)), quads=_mover_scene(0).quads.copy())
    for mf in FOLLOWS:
        same_bits(r.render_motion(prev, 37, 13, follow=mf), r.render_motion(prev, 37, 13), f"no specular surface, max_follow {mf}")


def test_device_forms_give_the_same_bits_and_leave_nothing_stale(r):
    torch = pytest.importorskip("torch")
    cs = P.scene("rich")
    r.upload_scene(cs)
    moved = _moved(cs, 10)
    cam = _cameras(cs)["about z"]
    dev = torch.device("cuda", r.device)
    arrays = {k: torch.from_numpy(v.copy()).to(dev) for k, v in moved.items()}
    for W, H in ((70, 41), (37, 13)):                                   # the smaller image after the larger one
        want = r.render_motion(M.Prev(cs, cam, **moved), W, H, follow=8)
        same_bits(want, MF.render_motion_followed(cs, M.Prev(cs, cam, **moved), W, H, 8, gpu_trace(r)), f"host arrays {W} x {H}")
        bare = M.Prev(cs, cam)                                          # (its host arrays are NOT what the call may read)
        same_bits(r.render_motion(bare, W, H, device_arrays=arrays, follow=8), want, f"device shapes {W} x {H}")
        out = r.render_motion(bare, W, H, device_arrays=arrays, device=True, follow=8)
        assert out.is_cuda and tuple(out.shape) == (H, W, 4)
        same_bits(out.cpu().numpy(), want, f"device shapes and device out {W} x {H}")
        same_bits(r.render_motion(M.Prev(cs, cam, **moved), W, H, device=True, follow=8).cpu().numpy(), want, f"device out {W} x {H}")
        assert (device.motion_ids(out) == want.view(U)[..., 3]).all()
    assert all((arrays[k].cpu().numpy() == moved[k]).all() for k in moved)


@pytest.mark.parametrize("env", [{"HJ_GROUP_TILE": "1"}, {"HJ_PAIR_LEAVES": "0"}, {"HJ_TRACE_WG_RAYS": "100"}], ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_no_result_bit_changes_under_the_walk_switches(r, monkeypatch, env):
    sizes = ((70, 41), (9, 9))
    wants = {}
    for scene in ("cbox", "rich"):
        cs = P.scene(scene)
        r.upload_scene(cs)
        for W, H in sizes:
            wants[scene, W, H] = r.render_motion(_prev(cs), W, H, follow=8)
    for k in ("HJ_GROUP_TILE", "HJ_PAIR_LEAVES", "HJ_TRACE_WG_RAYS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with device.Renderer(0) as other:
        for scene in ("cbox", "rich"):
            cs = P.scene(scene)
            other.upload_scene(cs)
            for W, H in sizes:
                same_bits(other.render_motion(_prev(cs), W, H, follow=8), wants[scene, W, H], f"{scene} {W} x {H} under {env}")


@pytest.mark.parametrize("route", ["host tree", "device-built tree", "resident tree", "after update_shapes"])
def test_every_route_into_an_upload(r, route):
    W, H = 70, 41
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile()
    old = dict(spheres=cs.spheres.copy(), quads=cs.quads.copy(), vertices=cs.vertices.copy())
    if route == "device-built tree":
        cs.set_bvh(r.build_bvh(cs))
        r.upload_scene(cs)
    elif route == "resident tree":
        r.build_bvh(cs, keep_on_device=True)
        cs.set_bvh(r.read_device_bvh().copy())
        r.upload_scene(cs, device_tree=True)
    else:
        r.upload_scene(cs)
    if route == "after update_shapes":                                  # the ordinary frame loop: move, update, ask against the old arrays
        d = Deformation(cs, seed=8)
        d.apply(0.03, t=0.4)
        r.update_shapes(cs)
        prev = M.Prev(cs, _cameras(cs)["about x"], **{k: v for k, v in old.items() if len(v)})
    else:
        prev = _prev(cs, 7, "about x")
    want, det = MF.render_motion_followed(cs, prev, W, H, 2, gpu_trace(r), detail=True)
    assert det["went"].sum() > 50
    same_bits(r.render_motion(prev, W, H, follow=2), want, route)
    if route == "after update_shapes":
        d.restore()


# ------------------------------------------------------------------------------------------------------ the behavioural condition

def _mirror_scene(k):
    """A camera at the origin (no rotation, fov 90, 64 x 64) in front of a mirror quad that fills the view at z = -4.  Behind the camera
    a diffuse wall at z = +6 and a 2.5 x 2.5 diffuse quad at z = +2: the mirror shows them at the depths 14 and 10 - against its own
    4 -, the small quad as an 8 x 8 footprint (a pixel at depth 10 is 0.3125 units) that moves 3 pixels a frame.  An emissive quad
    behind the wall: no chain reaches it."""
    s = host.Scene()
    s.set_camera((0, 0, 0), (0, 0, 0, 1), 90.0)
    grey, light = s.add_diffuse((0.5, 0.5, 0.5)), s.add_emissive((5, 5, 5))
    s.add_quad((-10, -10, -4), (20, 0, 0), (0, 20, 0), s.add_mirror())
    s.add_quad((-40, -40, 6), (80, 0, 0), (0, 80, 0), grey)
    s.add_quad((-5.0 + 0.9375 * k, -1.25, 2), (2.5, 0, 0), (0, 2.5, 0), grey)
    s.add_quad((-1, -1, 20), (2, 0, 0), (0, 2, 0), light)
    return s.compile()


def test_a_mirror_keeps_its_history_with_followed_motion_and_loses_it_with_first_hit_motion(r, oracle):
    W = H = 64
    frames = 4
    rng = np.random.default_rng(12)
    cam = _mirror_scene(0).desc.camera
    scenes = [_mirror_scene(k) for k in range(frames)]                  # (kept: a Prev views its scene's arrays)
    masks, aovs, beauties, followed_of, first_of = [], [], [], [], []
    # the reference alone, before any GPU is asked
    hf = h1 = hs = None
    for k in range(frames):
        cs = scenes[k]
        prev = M.Prev(cs, cam, quads=scenes[k - 1].quads.copy() if k else None)
        mf, det = MF.render_motion_followed(cs, prev, W, H, 2, R.oracle_trace(cs), detail=True)
        assert det["went"].all() and not det["left"].any() and (det["count"] == 1).all()       # every pixel is the mirror's
        f = det["first"]
        m1 = M.render_motion(cs, prev, W, H, (f[:, 0].copy().view(np.int32), f[:, 1], f[:, 2], f[:, 3]))
        mask = MF.ids_of(mf) == 2
        assert mask.sum() == 64 and set(np.round(det["D"][mask]).tolist()) <= {10.0, 11.0} and det["D"][~mask].min() >= 14   # an 8 x 8 footprint
        aov = np.zeros((H, W, 12), F)
        aov[..., 0:3], aov[..., 3], aov[..., 6], aov[..., 7], aov[..., 11] = 0.5, 1, 1, det["D"], 1   # guides with the followed depth
        beauty = np.concatenate([rng.uniform(0.2, 1.0, (H, W, 3)), np.ones((H, W, 1))], -1).astype(F)
        masks.append(mask), aovs.append(aov), beauties.append(beauty), followed_of.append(mf), first_of.append(m1)
        _, hf, sf = M.run(beauty, aov, mf, hf, 0, keep=True)
        _, h1, s1 = M.run(beauty, aov, m1, h1, 0, keep=True)
        _, hs, ss = T.run(beauty, aov, cam, cam, hs, 0, keep=True)
        if k == 0:
            continue
        fx, fy = np.floor(mf[..., 0] - F(0.5)).astype(int), np.floor(mf[..., 1] - F(0.5)).astype(int)
        was = masks[k - 1]
        inside = np.zeros((H, W), bool)
        ok = mask & (fx >= 0) & (fx + 1 < W) & (fy >= 0) & (fy + 1 < H)
        inside[ok] = was[fy[ok], fx[ok]] & was[fy[ok], fx[ok] + 1] & was[fy[ok] + 1, fx[ok]] & was[fy[ok] + 1, fx[ok] + 1]
        fresh = inside & ~was                                           # the mover's image newly covers them in frame k
        assert inside.sum() >= 30 and fresh.sum() >= 10, (k, inside.sum(), fresh.sum())
        assert np.abs(sf["N"][inside] - (k + 1)).max() < 1e-4, (k, sf["N"][inside])             # followed motion: the history follows the image
        assert (s1["N"] == 1).all(), k                                  # first-hit motion: zp is the mirror's 4, the guides say 10 and 14
        assert (ss["N"][fresh] == 1).all(), k                           # no motion: the mover's new pixels start again
    # the GPU: the same motion images, and the same three histories word for word
    gf = g1 = gs = None
    for k in range(frames):
        cs = scenes[k]
        r.upload_scene(cs)
        prev = M.Prev(cs, cam, quads=scenes[k - 1].quads.copy() if k else None)
        mf, m1 = r.render_motion(prev, W, H, follow=2), r.render_motion(prev, W, H)
        same_bits(mf, followed_of[k], f"frame {k}: followed motion")
        same_bits(m1, first_of[k], f"frame {k}: first-hit motion")
        _, gf = r.denoise_frame_temporal(aovs[k], cam, cam, gf, beauties[k], 0, motion=mf)
        _, g1 = r.denoise_frame_temporal(aovs[k], cam, cam, g1, beauties[k], 0, motion=m1)
        _, gs = r.denoise_frame_temporal(aovs[k], cam, cam, gs, beauties[k], 0)
    same_bits(gf, hf, "the history with followed motion")
    same_bits(g1, h1, "the history with first-hit motion")
    same_bits(gs, hs, "the history of the static call")
