"""The two pixel walks - hj_render_motion's k_mv_walk and hj_render_aovs' k_aov_walk - in the forms no scene of test size takes by
itself: the 8 x 8 tile grouping (HJ_GROUP_TILE=1; by default from HJ_STREAM_MIN_NODES nodes on), the plain-leaf instantiations
(HJ_PAIR_LEAVES=0) and workgroup segments of 64 and of 100 entries (HJ_TRACE_WG_RAYS; 100 starts a segment inside a 64-entry group).
The motion image against motion_ref over the oracle's first hits, from 1 x 1 over sizes one pixel into the next tile to the side
limit of 16384; every pixel written exactly once and nothing beyond the image, into a view in the middle of a tensor of sentinels;
the tile form against the row form.  The AOV sums against aov_ref over hj_trace_rays' records of a renderer WITHOUT a switch.
The followed calls - hj_render_motion_followed at max_follow 8, hj_render_aovs_followed and its frame form at 2 - in the same forms,
against motion_follow_ref and follow_ref over that renderer's records: their rounds walk lists in the switched segments.
A switch is in the environment before the test's own renderer is created and its scene uploaded: the table is read there."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_follow_ref as MF
import motion_ref as M
import path_query_ref as P
import test_follow_gpu as FG
import test_motion_follow_gpu as MFG
from hijiki_amd import abi, device, host
from test_abi import ROOT
from test_aov_gpu import expected_aovs, ragged_blocks, same_bits
from test_motion_gpu import _cameras, _moved, _scene, check

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
TILE, PAIRS, WG = "HJ_GROUP_TILE", "HJ_PAIR_LEAVES", "HJ_TRACE_WG_RAYS"
SWITCHES = [{TILE: "1"}, {PAIRS: "0"}, {TILE: "1", PAIRS: "0"}, {TILE: "1", WG: "64"}, {TILE: "1", WG: "100"}, {WG: "100"}]
GROUPINGS = [{}, {TILE: "1"}]                                           # rows of 64 (the default of a small tree), 8 x 8 tiles
SIZES = [(1, 1), (7, 1), (1, 7), (8, 8), (9, 9), (65, 3), (70, 41)]     # 9 x 9: one pixel into the next tile both ways; 65 x 3: a second run of one pixel
SENTINEL = 0x7FC0DEAD                                                   # no record's word 3: an id is below the shape count or 0xFFFFFFFF


def _id(env):
    return ",".join(f"{k.replace('HJ_', '')}={v}" for k, v in env.items()) or "default"


@pytest.fixture(autouse=True)
def _no_switch_from_outside(monkeypatch):
    text = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_tuning.h")).read()
    for name in (TILE, PAIRS, WG):
        assert f'"{name}"' in text, name                               # (a switch the table does not know would switch nothing)
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def plain():
    """the renderer of the expected values: no test puts a switch into the environment before it has used it"""
    with device.Renderer(0) as r:
        yield r


def switch_on(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _prev(cs):
    return M.Prev(cs, _cameras(cs)["translated"], **_moved(cs, 5))


# -------------------------------------------------------------------------------------------------------------- hj_render_motion

@pytest.mark.parametrize("env", SWITCHES, ids=_id)
def test_motion_at_every_size_in_every_form(oracle, monkeypatch, env):
    cs = _scene()
    prev = _prev(cs)
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        for W, H in SIZES:
            want = check(r, oracle, cs, prev, W, H, "rest", f"{W} x {H}, {_id(env)}")
        ids = want.view(U)[..., 3]                                      # (70 x 41)
        ns, nq = len(cs.spheres), len(cs.quads)
        assert (ids < ns).sum() > 50 and ((ids >= ns) & (ids < ns + nq)).sum() > 50 and ((ids >= ns + nq) & (ids != M.NONE)).sum() > 50


def _scene_seen_from_inside():
    """_scene()'s shapes with the camera inside the box, at (0, 1, 0).  The fov spans the width, so the centre rays of a 1 x 16384
    image fan out over almost 180 degrees in a vertical plane: from the camera in front of the box they all miss, from inside
    each one hits the floor, the back wall or the ceiling, at a point of its own."""
    s = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280)
    green = s.add_diffuse((0.2, 0.6, 0.3))
    s.add_quad((-0.8, 1.1, 0.3), (0.6, 0.0, 0.1), (0.05, 0.5, 0.0), green)
    s.add_quad((0.15, 0.7, 0.5), (0.5, 0.1, -0.2), (-0.1, 0.6, 0.1), green)
    c = _scene().desc.camera
    s.set_camera((0.0, 1.0, 0.0), list(c.rotation), c.fov)
    return s.compile()


@pytest.mark.parametrize("env", GROUPINGS, ids=_id)
def test_motion_at_the_side_limit(oracle, monkeypatch, env):
    """16384 x 1 and 1 x 16384: 2048 tiles with one live row or one live column of eight each, or 256 runs of a row and 16384 runs
    of one pixel; one pixel more is refused"""
    cs = _scene()
    prev = _prev(cs)
    inside = _scene_seen_from_inside()
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        for W, H in ((16384, 1), (1, 16384)):
            want = check(r, oracle, cs, prev, W, H, "rest", f"{W} x {H}, {_id(env)}")
            none = want.view(U)[..., 3] == M.NONE
            assert none.all() if W == 1 else ((~none).sum() > 10000 and none.sum() > 1000)
        r.upload_scene(inside)
        want = check(r, oracle, inside, _prev(inside), 1, 16384, "inside", f"1 x 16384 from inside, {_id(env)}")
        assert (want.view(U)[..., 3] != M.NONE).all() and len(np.unique(want[..., 2])) > 8000      # (every pixel a hit; a distance shared by two pixels at most, above and below the camera)
        r.upload_scene(cs)
        for W, H in ((16385, 1), (1, 16385)):
            with pytest.raises(abi.HijikiError) as e:
                r.render_motion(prev, W, H)
            assert e.value.status == abi.HJ_ERR_INVALID and "1 ... 16384 each" in str(e.value), str(e.value)


@pytest.mark.parametrize("env", GROUPINGS, ids=_id)
def test_motion_writes_every_pixel_once_and_nothing_beyond_the_image(oracle, monkeypatch, env):
    """The device-output form into a 16-byte aligned view in the middle of a tensor of sentinels.  The walk writes a pixel's raw hit
    and the resolve reads it back in place, so a pixel no entry maps to keeps the sentinel as its raw hit - an id outside the scene,
    a miss where the reference has a hit -, an entry that maps outside the image writes beside the view, and padding that wrote
    would too: a mapping that skips or repeats a pixel cannot pass."""
    torch = pytest.importorskip("torch")
    cs = _scene()
    prev = _prev(cs)
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        dev = torch.device("cuda", r.device)
        for W, H in ((9, 9), (70, 41)):
            n, front, back = 4 * W * H, 4 * 1027, 4 * 4099             # words; a padded 72 x 48 image would reach 4 * 566 words past the view
            big = torch.full((front + n + back,), SENTINEL, dtype=torch.int32, device=dev)
            view = big[front:front + n]
            assert view.data_ptr() % 16 == 0 and view.data_ptr() == big.data_ptr() + 4 * front
            torch.cuda.synchronize(dev)
            r._check(device.lib().hj_render_motion(r._h, C.byref(prev.desc), W, H, abi.MOTION_DEVICE_OUT, view.data_ptr()))
            words = big.cpu().numpy().view(U)
            assert (words[:front] == SENTINEL).all() and (words[front + n:] == SENTINEL).all(), f"{W} x {H}: words outside the view were written"
            got = words[front:front + n].reshape(H, W, 4)
            assert not (got[..., 3] == SENTINEL).any(), f"{W} x {H}: {int((got[..., 3] == SENTINEL).sum())} pixels were never written"
            host_form = check(r, oracle, cs, prev, W, H, "rest", f"host array {W} x {H}, {_id(env)}")
            same_bits(got.view(F), r.render_motion(prev, W, H), f"the view / the host-array form {W} x {H}, {_id(env)}")
            same_bits(got.view(F), host_form, f"the view / the reference {W} x {H}, {_id(env)}")


def test_motion_in_tiles_equals_motion_in_rows(monkeypatch):
    W, H = 70, 41
    cs = _scene()
    prev = _prev(cs)
    got = {}
    for env in GROUPINGS:
        with monkeypatch.context() as m:
            switch_on(m, env)
            with device.Renderer(0) as r:
                r.upload_scene(cs)
                got[_id(env)] = r.render_motion(prev, W, H)
    same_bits(got["GROUP_TILE=1"], got["default"], "tiles / rows")
    assert (got["default"].view(U)[..., 3] != M.NONE).sum() > 1000


# ------------------------------------------------------------------------------------------------------------------ hj_render_aovs

def overlapping_blocks():
    """test_aov_gpu's rectangles at origins off the block grid: each overlap cuts a run, and samples beyond the image's edge are dropped"""
    blocks = []
    for k, (ox, oy, w, h) in enumerate([(0, 0, 16, 16), (8, 8, 16, 16), (24, 0, 16, 8), (30, 16, 16, 16), (0, 23, 40, 1), (8, 8, 16, 16), (39, 0, 1, 24)]):
        b = abi.ImageBlock()
        b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:] = k, 7 * k, (ox, oy), (w, h), (40, 24)
        b.sample_offset[:] = (0.5, 0.25 + 0.125 * k)
        blocks.append(b)
    return blocks


FRAME = (130, 130, 2, 77)                                               # test_aov_gpu's frame at the 128 boundary: blocks two pixels wide
_EXPECTED = {}


def expected(plain, name):
    """per scene, once, on the renderer without a switch and before any is set: the restatement's images over hj_trace_rays'
    records, and hj_debug_samples' records of the 32 x 32 block"""
    if name not in _EXPECTED:
        assert not any(k in os.environ for k in (TILE, PAIRS, WG))
        cs = P.scene(name)
        plain.upload_scene(cs)
        W, H, spp, seed = FRAME
        out = {"ragged": expected_aovs(plain, cs, 40, 24, ragged_blocks()), "overlapping": expected_aovs(plain, cs, 40, 24, overlapping_blocks()),
               "frame": expected_aovs(plain, cs, W, H, list(host.make_blocks(W, H, spp, seed))), "samples": plain.samples(P.camera_block())}
        w = out["ragged"]
        assert (w[..., 3] == 3).sum() == 40 * 24 - 256 and (w[:16, :16, 3] == 4).all() and (w[..., 11] > 0).any() and (w[..., 11] < w[..., 3]).any()
        w = out["overlapping"]
        assert w[12, 12, 3] == 3 and w[20, 35, 3] == 1 and w[23, 35, 3] == 2 and w[0, 39, 3] == 2 and w[..., 3].sum() == 256 * 3 + 128 + 80 + 40 + 24
        assert (out["frame"][..., 3] == spp).all() and out["frame"][..., 0:3].any()
        for a in out.values():
            a.setflags(write=False)
        _EXPECTED[name] = out
    return _EXPECTED[name]


@pytest.mark.parametrize("env", SWITCHES, ids=_id)
@pytest.mark.parametrize("name", ["cbox", "textured"])
def test_aovs_in_every_form(plain, monkeypatch, name, env):
    want = expected(plain, name)
    cs = P.scene(name)
    what = f"{name}, {_id(env)}"
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        same_bits(r.render_aovs(40, 24, blocks=ragged_blocks()), want["ragged"], f"ragged blocks, {what}")
        same_bits(r.render_aovs(40, 24, blocks=overlapping_blocks()), want["overlapping"], f"overlapping blocks, {what}")
        W, H, spp, seed = FRAME
        same_bits(r.render_aovs(W, H, spp=spp, master_seed=seed), want["frame"], f"frame form, {what}")
        same_bits(r.render_aovs(W, H, blocks=host.make_blocks(W, H, spp, seed)), want["frame"], f"block form of the frame, {what}")
        one = r.render_aovs(32, 32, blocks=[P.camera_block()])
        same_bits(one[..., 4:8], want["samples"][..., 4:8], f"normal and t, {what}")
        assert (one[..., 3] == 1).all() and ((one[..., 11] == 1) == (want["samples"][..., 7] != 0)).all() and (one[..., 11] == 1).any()


# ------------------------------------------------------------------------------------------------------------ the followed calls

FOLLOWED_KEYS = ("ragged", "overlapping", "130")                        # test_follow_gpu.BLOCKS: the two 40 x 24 lists and FRAME
_FOLLOWED_MOTION = {}


def expected_followed_motion(plain, name):
    """once, on the renderer without a switch and before any is set: motion_follow_ref's images at max_follow 8 over hj_trace_rays'
    records, every kind moved -> (prev, {size: image})"""
    if name not in _FOLLOWED_MOTION:
        assert not any(k in os.environ for k in (TILE, PAIRS, WG))
        cs = P.scene(name)
        plain.upload_scene(cs)
        prev = MFG._prev(cs)
        out = {}
        for W, H in SIZES:
            out[W, H], det = MF.render_motion_followed(cs, prev, W, H, 8, FG.gpu_trace(plain), detail=True)
            out[W, H].setflags(write=False)
        assert det["went"].sum() > 50 and (det["count"].max() >= 3 or name == "cbox")         # (70 x 41)
        _FOLLOWED_MOTION[name] = (prev, out)
    return _FOLLOWED_MOTION[name]


@pytest.mark.parametrize("env", SWITCHES, ids=_id)
@pytest.mark.parametrize("name", ["cbox", "rich"])
def test_followed_motion_at_every_size_in_every_form(plain, monkeypatch, name, env):
    """hj_render_motion_followed: k_mv_walk's entries in the switched form, then the rounds' lists in segments of 64 or 100"""
    prev, want = expected_followed_motion(plain, name)
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:
        r.upload_scene(P.scene(name))
        for W, H in SIZES:
            same_bits(r.render_motion(prev, W, H, follow=8), want[W, H], f"followed motion {name} {W} x {H}, {_id(env)}")


@pytest.mark.parametrize("env", SWITCHES, ids=_id)
@pytest.mark.parametrize("name", ["cbox", "rich"])
def test_followed_aovs_in_every_form(plain, monkeypatch, name, env):
    """hj_render_aovs_followed and its frame form at max_follow 2 against follow_ref's chains over the plain renderer's records"""
    wants = {key: FG.expected(plain, name, key, 2)[0] for key in FOLLOWED_KEYS}
    what = f"{name}, {_id(env)}"
    switch_on(monkeypatch, env)
    with device.Renderer(0) as r:
        r.upload_scene(P.scene(name))
        for key in ("ragged", "overlapping"):
            same_bits(r.render_aovs(40, 24, blocks=FG.BLOCKS[key][2](), follow=2), wants[key], f"followed {key} blocks, {what}")
        W, H, spp, seed = FRAME
        same_bits(r.render_aovs(W, H, spp=spp, master_seed=seed, follow=2), wants["130"], f"followed frame form, {what}")
