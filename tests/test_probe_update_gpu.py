"""hj_update_probes and hj_update_probe_visibility on the GPU, bit for bit: with a zero hysteresis over NaN memory the update IS the
existing bake under the frame's seed (a seed sum that passes 2^32); the blend against probe_update_ref with the GPU's own bake as the
fresh half - kept, soft and hard changes, invalid probes, NaN coefficients behind a zero validity -, on device tensors and host
arrays; probe windows that leave a sentinel outside alone; the atlas from a fabricated one with NaN, infinities and mismatched
borders, through a window that crosses slabs; the update after hj_scene_update_shapes; and the purpose: 32 blended updates at 16 spp
come nearer to a 4096 spp bake than a single one."""
import functools

import numpy as np
import pytest

import path_query_ref as R
import probe_ref as P
import probe_update_ref as PU
import probe_vis_ref as V
import update_scenes
from hijiki_amd import abi, device
from refit_scenes import refit_numpy, shape_boxes
from test_probe_vis_gpu import assert_bits_or_nan
from test_probes_gpu import assert_bits

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SEED, STRIDE = 0xFFFFFFF0, 7
FRAME, FRAME_STRIDE = 3, 0x60000001                                     # frame * frame_stride = 0x120000003: beyond 2^32
SEED2 = PU.frame_seed(SEED, FRAME, FRAME_STRIDE)
SPP = 16
INF = float("inf")


@pytest.fixture(scope="module")
def pu():
    with device.Renderer(0) as ctx:
        ctx.upload_scene(R.scene("cbox"))
        yield ctx


def desc_kw(d, seed=SEED, min_distance=0.0):
    """a probe_ref desc as the dict the update wrappers take (and bake_probes' keywords)"""
    return dict(origin=d["origin"], spacing=d["spacing"], count=d["count"], seed=seed, seed_stride=STRIDE, min_distance=min_distance)


@functools.lru_cache(maxsize=None)
def grid(count):
    return P.grid_in_domain(R.scene("cbox"), count, SEED, STRIDE)


def vis_grid_kw(d, seed=SEED):
    """... and bake_probe_visibility's keywords (it has no min_distance)"""
    return dict(origin=d["origin"], spacing=d["spacing"], count=d["count"], seed=seed, seed_stride=STRIDE)


def fresh_volume(pu, d, seed=SEED2):
    """the existing bake under the frame's seed: the fresh half of every blend, (n, 28)"""
    return pu.bake_probes(**desc_kw(d, seed), spp=SPP, opts=R.options(40)).reshape(-1, 28)


def on_gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)).contiguous()


def nan_like(shape):
    a = np.empty(shape, F)
    a.view(U)[...] = 0x7FA12345
    return a


# ----------------------------------------------------------------------------------------------------------- 1. the fresh bake

@pytest.mark.parametrize("count", [(3, 3, 3), (5, 4, 3)])
def test_zero_hysteresis_over_nan_memory_is_the_bake(pu, count):
    d = grid(count)
    assert FRAME * FRAME_STRIDE > 1 << 32 and SEED2 == (SEED + FRAME * FRAME_STRIDE) % (1 << 32)
    want = fresh_volume(pu, d)
    assert np.isfinite(want).all() and (want[:, 0:3] != 0).any()
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0, opts=R.options(40))
    shape = (count[2], count[1], count[0], 28)
    t = on_gpu(nan_like(shape))
    got = pu.update_probes(desc_kw(d), t, SPP, **kw)
    assert got is t
    assert_bits(t.cpu().numpy().reshape(-1, 28), want, f"update {count}, h = 0, device arrays")
    got, stats = pu.update_probes(desc_kw(d), nan_like(shape), SPP, stats=True, **kw)
    assert_bits(got.reshape(-1, 28), want, f"update {count}, h = 0, host arrays")
    assert stats["paths"] > 0
    assert (want.view(U) != fresh_volume(pu, d, SEED).view(U)).any()       # (the frame's seed is another seed)


@pytest.mark.parametrize("res", [4, 16])
def test_zero_hysteresis_over_nan_memory_is_the_visibility_bake(pu, res):
    count = (3, 3, 3)
    d = grid(count)
    vis = dict(res=res, rays_per_texel=2, max_distance=1e18)
    want = pu.bake_probe_visibility(**vis_grid_kw(d, SEED2), **vis)
    shape = want.shape
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0)
    t = on_gpu(nan_like(shape))
    assert pu.update_probe_visibility(desc_kw(d), vis, t, **kw) is t
    assert_bits(t.cpu().numpy().reshape(-1, 2), want.reshape(-1, 2), f"visibility update res {res}, h = 0, device arrays")
    got = pu.update_probe_visibility(desc_kw(d), vis, nan_like(shape), **kw)
    assert_bits(got.reshape(-1, 2), want.reshape(-1, 2), f"visibility update res {res}, h = 0, host arrays")


# -------------------------------------------------------------------------------------------------- 2. the blend and its branches

def old_volume(fresh):
    """per probe p the fresh coefficients times 1.0, 1.1, 1.5, 3, 10 by p % 5 (the constant band then moves by 0, 0.09, 0.33, 0.67, 0.9 of its
    old magnitude: kept, kept, soft, soft, hard); probes 7 and 22 invalid with NaN coefficients, probe 11 invalid with finite ones,
    probes 13 and 14 with validity 0.25"""
    old = fresh.copy()
    factor = np.array([1.0, 1.1, 1.5, 3.0, 10.0], F)[np.arange(len(old)) % 5]
    old[:, 0:27] = fresh[:, 0:27] * factor[:, None]
    old[[7, 22], 0:27] = np.nan
    old[[7, 22, 11], 27] = 0.0
    old[[13, 14], 27] = 0.25
    return old


def test_blend_matches_the_reference_in_every_branch(pu):
    count = (5, 4, 3)
    d = grid(count)
    fresh = fresh_volume(pu, d)
    lit = np.abs(fresh[:, 0:3]).max(1) > 0                              # (the domain reaches out to the camera: probes there see nothing)
    assert (fresh[:, 27] == 1).all() and lit.sum() >= 10
    old = old_volume(fresh)
    shape = (count[2], count[1], count[0], 28)
    for h, change in ((0.7, (0.25, 0.8)), (0.1, (0.25, 0.8)), (0.9, (INF, INF)), (0.7, (0.0, 0.5))):
        want, hh, masks = PU.blend_probes(old, fresh, PU.update(0, len(old), h, *change), detail=True)
        taken = {k: int(v.sum()) for k, v in masks.items()}
        print(f"h {h} change {change}: {taken}")
        if change == (0.25, 0.8):
            assert taken["none"] > 0 and taken["soft"] > 0 and taken["hard"] > 0 and taken["old_invalid"] == 3, taken
        kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=h, change=change, opts=R.options(40))
        t = on_gpu(old.reshape(shape))
        pu.update_probes(desc_kw(d), t, SPP, **kw)
        assert_bits(t.cpu().numpy().reshape(-1, 28), want, f"blend h {h} change {change}, device arrays")
        got = pu.update_probes(desc_kw(d), old.reshape(shape), SPP, **kw)
        assert_bits(got.reshape(-1, 28), want, f"blend h {h} change {change}, host arrays")
        assert np.isfinite(want).all()                                 # (the NaN coefficients stood behind a zero validity: never mixed)


def test_a_probe_that_becomes_invalid_takes_the_fresh_record(pu):
    """A min_distance larger than the room: the fresh bake finds every probe that sees a surface invalid (the probes out by the camera
    see none and stay valid), and each of those takes the fresh record, bit for bit, whatever the hysteresis and the old record."""
    count = (3, 3, 3)
    d = grid(count)
    fresh = pu.bake_probes(**desc_kw(d, SEED2, min_distance=1e6), spp=SPP, opts=R.options(40)).reshape(-1, 28)
    gone = fresh[:, 27] == 0
    assert gone.sum() >= 9 and set(np.unique(fresh[:, 27])) <= {0.0, 1.0}
    old = old_volume(fresh_volume(pu, d, SEED))
    want = PU.blend_probes(old, fresh, PU.update(0, 27, 0.9, 0.25, 0.8))
    assert_bits(want[gone], fresh[gone], "the reference itself")
    got = pu.update_probes(desc_kw(d, min_distance=1e6), old.reshape(3, 3, 3, 28), SPP, frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.9,
                           opts=R.options(40))
    assert_bits(got.reshape(-1, 28), want, "probes that became invalid")


# --------------------------------------------------------------------------------------------------------------------- 3. windows

SENTINEL = 0xDEADBEEF


@pytest.mark.parametrize("num", [1, 7, 22, 0])
def test_windows_leave_everything_outside_alone(pu, num):
    import torch
    count = (3, 3, 3)
    n, first = 27, 5
    d = grid(count)
    fresh = fresh_volume(pu, d)
    old = old_volume(fresh_volume(pu, d, SEED))
    inside = np.zeros(n, bool)
    inside[first:first + num] = True
    old.view(U)[~inside] = SENTINEL
    want = PU.blend_probes(old, fresh, PU.update(first, num, 0.7, 0.25, 0.8))
    assert (want.view(U)[~inside] == SENTINEL).all() and (num == 0 or (want.view(U)[inside] != old.view(U)[inside]).any())
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.7, window=(first, num), opts=R.options(40))
    t = on_gpu(old.reshape(3, 3, 3, 28))
    pu.update_probes(desc_kw(d), t, SPP, **kw)
    assert_bits(t.cpu().numpy().reshape(-1, 28), want, f"window {first} + {num}, device arrays")
    got = pu.update_probes(desc_kw(d), old.reshape(3, 3, 3, 28), SPP, **kw)
    assert_bits(got.reshape(-1, 28), want, f"window {first} + {num}, host arrays")
    if num == 0:                                                       # ... and an empty window at the volume's end
        pu.update_probes(desc_kw(d), t, SPP, **dict(kw, window=(n, 0)))
        assert_bits(t.cpu().numpy().reshape(-1, 28), old, "an empty window")
        vis = dict(res=4, rays_per_texel=1, max_distance=5.0)
        a = on_gpu(V.hashed_atlas(n, 4, 1).reshape(3, 3, 3, 6, 6, 2))
        keep = a.clone()
        pu.update_probe_visibility(desc_kw(d), vis, a, frame=1, hysteresis=0.5, window=(first, 0))
        assert torch.equal(a.view(torch.int32), keep.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ 4. visibility

@pytest.mark.parametrize("count,res,s,window", [((5, 5, 4), 16, 64, (5, 70)), ((3, 3, 3), 4, 3, (0, 27)), ((3, 3, 3), 8, 1, (3, 20))])
def test_visibility_blend_matches_the_reference(pu, count, res, s, window):
    """(5, 5, 4) at res 16 and 64 rays a texel: 32 probes a slab, so the window 5 ... 74 starts inside the first slab of the volume,
    runs over three slabs of its own and ends inside one.  The old atlas holds NaN, infinities and borders that do not match: a NaN the
    blend computes with is a NaN of no defined payload, every other word is compared bit for bit; the two routes on the GPU agree in
    every bit."""
    assert res != 16 or abi.PROBE_VIS_SLAB_RAYS // (res * res * s) == 32
    d = grid(count)
    n = count[0] * count[1] * count[2]
    vis = dict(res=res, rays_per_texel=s, max_distance=1e18)
    fresh = pu.bake_probe_visibility(**vis_grid_kw(d, SEED2), **vis)
    old = V.hashed_atlas(n, res, 5).reshape(fresh.shape)
    h = 0.9
    want = PU.blend_atlas(old, fresh, res, PU.update(*window, h))
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=h, window=window)
    t = on_gpu(old)
    pu.update_probe_visibility(desc_kw(d), vis, t, **kw)
    dev = t.cpu().numpy()
    assert_bits_or_nan(dev.reshape(-1, 2), want.reshape(-1, 2), f"visibility blend {count} res {res} window {window}, device arrays")
    got = pu.update_probe_visibility(desc_kw(d), vis, old, **kw)
    assert_bits(got.reshape(-1, 2), dev.reshape(-1, 2), f"visibility blend {count} res {res}: host arrays against device arrays")
    # the border was repaired inside the window and nowhere else
    T = res + 2
    flat = dev.reshape(n, T * T, 2).view(U)
    copied = dev.reshape(n, T, T, 2)[:, 1:-1, 1:-1].reshape(n, res * res, 2).view(U)[:, V.border_source(res)]
    ok = (flat == copied).all(axis=(1, 2))
    a, b = window[0], window[0] + window[1]
    assert ok[a:b].all() and not ok[:a].any() and not ok[b:].any()
    assert np.isnan(want).any() and np.isinf(want).any()


# ----------------------------------------------------------------------------------------------------------- 5. the current scene

def test_update_sees_the_moved_scene():
    rest, moved = update_scenes.light_show(triangles=150), update_scenes.light_show(moved=True, triangles=150)
    moved.set_bvh(refit_numpy(rest.bvh.copy(), shape_boxes(moved)))
    g = dict(origin=(-1.0, 0.2, -1.0), spacing=(1.0, 0.8, 1.0), count=(3, 3, 3), seed=SEED, seed_stride=STRIDE, min_distance=0.0)
    o = R.options(40)
    with device.Renderer(0) as r:
        r.upload_scene(moved)
        want = r.bake_probes(**dict(g, seed=SEED2), spp=SPP, opts=o)
    with device.Renderer(0) as r:
        r.upload_scene(rest)
        before = r.update_probes(g, nan_like(want.shape), SPP, frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0, opts=o)
        r.update_shapes(moved)
        got = r.update_probes(g, before, SPP, frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0, opts=o)
    assert (before.view(U) != want.view(U)).any()
    assert_bits(got.reshape(-1, 28), want.reshape(-1, 28), "an update after hj_scene_update_shapes against a bake of the moved scene")


# ------------------------------------------------------------------------------------------------------------------ 6. the purpose

def test_blended_updates_beat_a_single_one(pu):
    """32 updates at 16 spp with h = 0.9 (the first with h = 0, thresholds infinite) against a 4096 spp bake: the RMS error of the
    constant band is below the median error of the 32 single updates.  An exponential average of independent estimates has the variance
    (1 - h) / (1 + h) of one (beyond the first's decaying share, 0.9^31 = 0.04): about 4.4 times less error; only "below the median"
    is gated."""
    count = (3, 3, 3)
    d = grid(count)
    truth = pu.bake_probes(**desc_kw(d, 12345), spp=4096, opts=R.options(40)).reshape(-1, 28)[:, 0:3].astype(np.float64)
    rms = lambda v: float(np.sqrt(np.mean((v.reshape(-1, 28)[:, 0:3].astype(np.float64) - truth) ** 2)))      # noqa: E731
    acc = on_gpu(nan_like((3, 3, 3, 28)))
    one = on_gpu(nan_like((3, 3, 3, 28)))
    single = []
    for frame in range(32):
        kw = dict(frame=frame, opts=R.options(40), change=(INF, INF))
        pu.update_probes(desc_kw(d), one, SPP, hysteresis=0.0, **kw)
        single.append(rms(one.cpu().numpy()))
        pu.update_probes(desc_kw(d), acc, SPP, hysteresis=0.0 if frame == 0 else 0.9, **kw)
    blended, median = rms(acc.cpu().numpy()), float(np.median(single))
    print(f"RMS error of the constant band against 4096 spp: blended {blended:.5g}, single updates median {median:.5g} "
          f"(min {min(single):.5g}, max {max(single):.5g}); ratio {median / blended:.3g} (expected about {np.sqrt(1.9 / 0.1):.3g})")
    assert blended < median
