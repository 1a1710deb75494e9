"""hj_place_probes and the placed updates and look-up on the GPU, bit for bit: the step against probe_place_ref fed with the GPU's own
hj_trace_rays hits and surface records for numpy-built placed rays - two volumes, windows around sentinels, slabs of 32 probes, host
and device arrays -; a zero placement makes the three placed calls their unplaced counterparts; a placed update with h = 0 is
hj_trace_irradiance over numpy-built placed points resolved by probe_ref, inactive probes keep a NaN-and-sentinel pattern and stats
counts the active probes alone; an all-inactive window; an active count that crosses one compaction tile; the placed visibility
update against probe_vis_ref over placed rays; the placed look-up on fabricated volumes; and the host test's cube, uploaded."""
import functools

import numpy as np
import pytest

import path_query_ref as R
import probe_place_ref as PP
import probe_ref as P
import probe_update_ref as PU
import probe_vis_ref as V
from hijiki_amd import abi, device, host
from test_probe_update_gpu import FRAME, FRAME_STRIDE, SEED, SEED2, STRIDE, desc_kw, nan_like, on_gpu
from test_probe_vis_gpu import assert_bits_or_nan
from test_probes_gpu import assert_bits

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SPP = 8
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def pp():
    with device.Renderer(0) as ctx:
        ctx.upload_scene(R.scene("cbox"))
        yield ctx


@functools.lru_cache(maxsize=None)
def grid(count):
    return P.grid_in_domain(R.scene("cbox"), count, SEED, STRIDE)


def gpu_trace(ctx):
    def trace(ray):
        ids, t, _, _, surf = ctx.trace_rays(np.ascontiguousarray(ray, F), surface=True)
        return ids, t, surf[:, 3:6]
    return trace


def some_placement(d, seed, asleep=4):
    """offsets within 0.3 spacings from a seeded generator, every `asleep`-th probe inactive -> (n, 4)"""
    nx, ny, nz = d["count"]
    n = nx * ny * nz
    rng = np.random.default_rng(seed)
    pl = PP.zeros(n)
    pl[:, 0:3] = (rng.uniform(-0.3, 0.3, (n, 3)) * np.asarray(d["spacing"], np.float64)).astype(F)
    return PP.with_state(pl, (np.arange(n) % asleep == 1).astype(U))


def shaped(d, a, *tail):
    nx, ny, nz = d["count"]
    return np.ascontiguousarray(a).reshape(nz, ny, nx, *tail)


def vis_kw(v):
    return dict(res=v["res"], rays_per_texel=v["s"], max_distance=v["max_distance"])


# ------------------------------------------------------------------------------------------------------------------ 1. the step

@pytest.mark.parametrize("count,res,s,window", [((3, 3, 3), 4, 1, None), ((4, 3, 2), 4, 2, (5, 13)), ((5, 5, 4), 16, 64, (5, 70))])
def test_place_matches_the_reference(pp, count, res, s, window):
    """(5, 5, 4) at res 16 and 64 rays a texel: 32 probes a slab, so the window 5 ... 74 runs over three slabs.  Outside a window every
    word keeps a sentinel.  The reference takes the GPU's own hits and surface records for rays built in numpy."""
    assert res != 16 or abi.PROBE_VIS_SLAB_RAYS // (res * res * s) == 32
    d = grid(count)
    n = count[0] * count[1] * count[2]
    first, num = window or (0, n)
    spacing = np.asarray(d["spacing"], F)
    v = V.vis(res, s, max_distance=F(1.5) * spacing.max())
    old = some_placement(d, 31)
    outside = np.ones(n, bool)
    outside[first:first + num] = False
    old.view(U)[outside] = SENTINEL
    pl = PP.place(first, num, F(0.2) * spacing.min(), 0.25, 0.45)
    want, masks, inside, st = PP.trace_step(gpu_trace(pp), d, v, pl, old, seed=SEED2, detail=True)
    taken = {k: int(m.sum()) for k, m in masks.items()}
    print(f"{count} res {res} s {s}: {taken}, inactive {int((st != 0).sum())} of {num}")
    assert (want.view(U)[outside] == SENTINEL).all() and (want.view(U)[~outside] != old.view(U)[~outside]).any()
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, min_front_distance=pl["min_front"], window=(first, num))
    t = on_gpu(shaped(d, old, 4))
    assert pp.place_probes(desc_kw(d), vis_kw(v), t, **kw) is t
    assert_bits(t.cpu().numpy().reshape(-1, 4), want, f"place {count} res {res} s {s}, device arrays")
    got = pp.place_probes(desc_kw(d), vis_kw(v), shaped(d, old, 4), **kw)
    assert_bits(got.reshape(-1, 4), want, f"place {count} res {res} s {s}, host arrays")
    if window is None:                                                 # the flags, and an empty window
        for flags, kwf in ((PP.NO_RELOCATE, dict(relocate=False)), (PP.NO_CLASSIFY, dict(classify=False)), (3, dict(relocate=False, classify=False))):
            ref = PP.trace_step(gpu_trace(pp), d, v, dict(pl, flags=flags), old, seed=SEED2)
            assert_bits(pp.place_probes(desc_kw(d), vis_kw(v), shaped(d, old, 4), **dict(kw, **kwf)).reshape(-1, 4), ref, f"place, flags {flags}")
        assert_bits(pp.place_probes(desc_kw(d), vis_kw(v), shaped(d, old, 4), **dict(kw, window=(n, 0))).reshape(-1, 4), old, "an empty window")


# ------------------------------------------------------------------------------------------------------------ 2. a zero placement

def test_a_zero_placement_is_the_unplaced_call(pp):
    count = (3, 3, 3)
    d = grid(count)
    zero = on_gpu(shaped(d, PP.zeros(27), 4))
    vis = dict(res=4, rays_per_texel=2, max_distance=1e18)
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE)
    old_v = P.fabricated_volume(count, 3).reshape(3, 3, 3, 28)
    a, b = on_gpu(old_v), on_gpu(old_v)
    pp.update_probes(desc_kw(d), a, SPP, hysteresis=0.6, opts=R.options(40), **kw)
    pp.update_probes(desc_kw(d), b, SPP, hysteresis=0.6, opts=R.options(40), placement=zero, **kw)
    assert_bits_or_nan(b.cpu().numpy().reshape(-1, 28), a.cpu().numpy().reshape(-1, 28), "placed update, zero placement")
    assert_bits(pp.update_probes(desc_kw(d), nan_like(old_v.shape), SPP, hysteresis=0.0, opts=R.options(40), placement=PP.zeros(27).reshape(3, 3, 3, 4),
                                 **kw).reshape(-1, 28), pp.update_probes(desc_kw(d), nan_like(old_v.shape), SPP, hysteresis=0.0, opts=R.options(40),
                                                                         **kw).reshape(-1, 28), "placed update, zero placement, host arrays")
    old_a = V.hashed_atlas(27, 4, 5).reshape(3, 3, 3, 6, 6, 2)
    a, b = on_gpu(old_a), on_gpu(old_a)
    pp.update_probe_visibility(desc_kw(d), vis, a, hysteresis=0.8, **kw)
    pp.update_probe_visibility(desc_kw(d), vis, b, hysteresis=0.8, placement=zero, **kw)
    assert_bits_or_nan(b.cpu().numpy().reshape(-1, 2), a.cpu().numpy().reshape(-1, 2), "placed visibility update, zero placement")
    host_b = pp.update_probe_visibility(desc_kw(d), vis, old_a, hysteresis=0.8, placement=PP.zeros(27).reshape(3, 3, 3, 4), **kw)
    assert_bits(host_b.reshape(-1, 2), b.cpu().numpy().reshape(-1, 2), "placed visibility update: host arrays against device arrays")
    pts = P.sample_points(d, 700, 9)
    for flags in (dict(), dict(backface=False), dict(chebyshev=False)):
        skw = dict(origin=d["origin"], spacing=d["spacing"], normal_bias=0.02, **flags)
        plain = pp.sample_probes_visible(on_gpu(old_v), on_gpu(old_a), points=on_gpu(pts), **skw).cpu().numpy()
        placed = pp.sample_probes_visible(on_gpu(old_v), on_gpu(old_a), points=on_gpu(pts), placement=zero, **skw).cpu().numpy()
        assert_bits_or_nan(placed, plain, f"placed look-up, zero placement {flags}")
    finite = np.nan_to_num(old_v, nan=0.5, posinf=1.0, neginf=-1.0)
    assert_bits(pp.sample_probes_visible(finite, old_a, d["origin"], d["spacing"], pts, normal_bias=0.02, placement=PP.zeros(27).reshape(3, 3, 3, 4)),
                pp.sample_probes_visible(finite, old_a, d["origin"], d["spacing"], pts, normal_bias=0.02), "placed look-up, zero placement, host arrays")


# ------------------------------------------------------------------------------------------------------------ 3. the placed update

def fresh_active(pp, d, placement, first, num):
    """hj_trace_irradiance over numpy-built placed points of the window's active probes, resolved by probe_ref -> (m, 28), the list"""
    act = PP.active(placement, first, num)
    pts = PP.points(dict(d, seed=SEED2), placement, act)
    rec = pp.trace_irradiance(pts, spp=SPP, sphere=True, sh9=True, opts=R.options(40))
    return P.resolve(rec, SPP, d["min_distance"]), act


@pytest.mark.parametrize("count,window", [((4, 3, 2), None), ((4, 3, 2), (3, 17))])
def test_placed_update_is_the_gather_at_the_placed_points(pp, count, window):
    d = grid(count)
    n = count[0] * count[1] * count[2]
    first, num = window or (0, n)
    placement = some_placement(d, 41)
    fresh, act = fresh_active(pp, d, placement, first, num)
    assert 0 < len(act) < num
    old = nan_like((n, 28))                                              # NaN with a payload everywhere, a sentinel outside the window
    old.view(U)[:first] = SENTINEL
    old.view(U)[first + num:] = SENTINEL
    want = PP.blend_probes(old, fresh, placement, PU.update(first, num, 0.0))
    rest = np.setdiff1d(np.arange(n), act)
    assert (want.view(U)[rest] == old.view(U)[rest]).all() and np.isfinite(want[act]).all()
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0, window=(first, num), opts=R.options(40), stats=True)
    t = on_gpu(shaped(d, old, 28))
    _, stats = pp.update_probes(desc_kw(d), t, SPP, placement=on_gpu(shaped(d, placement, 4)), **kw)
    assert_bits(t.cpu().numpy().reshape(-1, 28), want, f"placed update {count} {window}, device arrays")
    assert stats["paths"] == SPP * len(act)
    got, stats = pp.update_probes(desc_kw(d), shaped(d, old, 28), SPP, placement=shaped(d, placement, 4), **kw)
    assert_bits(got.reshape(-1, 28), want, f"placed update {count} {window}, host arrays")
    assert stats["paths"] == SPP * len(act)
    _, full = pp.update_probes(desc_kw(d), shaped(d, old, 28), SPP, **kw)
    assert full["paths"] == SPP * num > stats["paths"]
    # a blend: the active probes against probe_update_ref, the others untouched
    base = P.fabricated_volume(count, 6).reshape(n, 28)
    want = PP.blend_probes(base, fresh, placement, PU.update(first, num, 0.7, 0.25, 0.8))
    got = pp.update_probes(desc_kw(d), shaped(d, base, 28), SPP, placement=shaped(d, placement, 4), **dict(kw, hysteresis=0.7, stats=False))
    assert_bits_or_nan(got.reshape(-1, 28), want, f"placed blend {count} {window}")


def test_an_all_inactive_window_writes_nothing(pp):
    import torch
    count = (3, 3, 3)
    d = grid(count)
    placement = PP.with_state(some_placement(d, 43), np.r_[np.zeros(4, U), np.ones(9, U), np.zeros(14, U)])
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0, window=(4, 9))
    t, a = on_gpu(nan_like((3, 3, 3, 28))), on_gpu(nan_like((3, 3, 3, 6, 6, 2)))
    keep_t, keep_a = t.clone(), a.clone()
    pl = on_gpu(shaped(d, placement, 4))
    _, stats = pp.update_probes(desc_kw(d), t, SPP, placement=pl, opts=R.options(40), stats=True, **kw)
    pp.update_probe_visibility(desc_kw(d), dict(res=4, rays_per_texel=1, max_distance=5.0), a, placement=pl, **kw)
    assert torch.equal(t.view(torch.int32), keep_t.view(torch.int32)) and torch.equal(a.view(torch.int32), keep_a.view(torch.int32))
    assert stats["paths"] == 0
    # host arrays: the window is staged in and the call ends at the empty list - every word comes back as it went
    vol, atl = nan_like((3, 3, 3, 28)), V.hashed_atlas(27, 4, 7).reshape(3, 3, 3, 6, 6, 2)
    got, stats = pp.update_probes(desc_kw(d), vol, SPP, placement=shaped(d, placement, 4), opts=R.options(40), stats=True, **kw)
    assert got is not vol and (got.view(U) == vol.view(U)).all() and stats["paths"] == 0
    got = pp.update_probe_visibility(desc_kw(d), dict(res=4, rays_per_texel=1, max_distance=5.0), atl, placement=shaped(d, placement, 4), **kw)
    assert got is not atl and (got.view(U) == atl.view(U)).all()


def test_an_active_count_that_crosses_a_compaction_tile(pp):
    """Tiles of 256 probes: a volume of 2 * 256 + 40 probes whose first tile is all active, whose second has 3 active probes and whose
    third has 25 - the list crosses the tile boundaries at ranks 256 and 259.  One sample a probe."""
    tile = 256
    count = (2 * tile + 40, 1, 1)
    d = grid(count)
    n = count[0]
    st = np.ones(n, U)
    st[:tile] = 0
    st[[tile, tile + 100, 2 * tile - 1]] = 0
    st[2 * tile + np.arange(0, 40, 2)[:20]] = 0
    st[2 * tile + np.array([1, 3, 5, 7, 39])] = 0
    placement = PP.with_state(some_placement(d, 47), st)
    act = PP.active(placement, 0, n)
    assert len(act) == tile + 3 + 25
    pts = PP.points(dict(d, seed=SEED2), placement, act)
    fresh = P.resolve(pp.trace_irradiance(pts, spp=1, sphere=True, sh9=True, opts=R.options(40)), 1, d["min_distance"])
    old = nan_like((n, 28))
    want = PP.blend_probes(old, fresh, placement, PU.update(0, n, 0.0))
    t = on_gpu(shaped(d, old, 28))
    _, stats = pp.update_probes(desc_kw(d), t, 1, frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=0.0, opts=R.options(40), stats=True,
                                placement=on_gpu(shaped(d, placement, 4)))
    assert_bits(t.cpu().numpy().reshape(-1, 28), want, "an active list across compaction tiles")
    assert stats["paths"] == len(act)


# ------------------------------------------------------------------------------------------------- 4. the placed visibility update

@pytest.mark.parametrize("count,res,s,window", [((4, 3, 2), 4, 3, None), ((5, 5, 4), 16, 64, (5, 70))])
def test_placed_visibility_update_matches_the_reference(pp, count, res, s, window):
    """(5, 5, 4) at res 16, 64 rays a texel: slabs of 32 LISTED probes.  An inactive probe's texels keep a mismatched border."""
    d = grid(count)
    n = count[0] * count[1] * count[2]
    first, num = window or (0, n)
    v = V.vis(res, s, 1e18)
    placement = some_placement(d, 53, asleep=3)
    act = PP.active(placement, first, num)
    ray = PP.rays(dict(d, seed=SEED2), v, placement, probes=act)
    ids, t, _, _ = pp.trace_rays(ray)
    fresh = V.reduce((ids, t), v)
    old = V.hashed_atlas(n, res, 5)
    h = 0.9
    want = PP.blend_atlas(old, fresh, res, placement, PU.update(first, num, h))
    kw = dict(frame=FRAME, frame_stride=FRAME_STRIDE, hysteresis=h, window=(first, num))
    tt = on_gpu(shaped(d, old, res + 2, res + 2, 2))
    pp.update_probe_visibility(desc_kw(d), vis_kw(v), tt, placement=on_gpu(shaped(d, placement, 4)), **kw)
    dev = tt.cpu().numpy()
    assert_bits_or_nan(dev.reshape(-1, 2), want.reshape(-1, 2), f"placed visibility update {count} res {res}, device arrays")
    got = pp.update_probe_visibility(desc_kw(d), vis_kw(v), shaped(d, old, res + 2, res + 2, 2), placement=shaped(d, placement, 4), **kw)
    assert_bits(got.reshape(-1, 2), dev.reshape(-1, 2), f"placed visibility update {count} res {res}: host arrays against device arrays")
    T = res + 2
    flat = dev.reshape(n, T * T, 2).view(U)
    copied = dev.reshape(n, T, T, 2)[:, 1:-1, 1:-1].reshape(n, res * res, 2).view(U)[:, V.border_source(res)]
    ok = (flat == copied).all(axis=(1, 2))
    rest = np.setdiff1d(np.arange(n), act)
    assert ok[act].all() and not ok[rest].any() and (flat[rest] == old.reshape(n, T * T, 2).view(U)[rest]).all()


# ------------------------------------------------------------------------------------------------------------ 5. the placed look-up

@pytest.mark.parametrize("count,res", [((3, 2, 2), 4), ((5, 4, 3), 8), ((1, 3, 2), 16)])
def test_placed_look_up_matches_the_reference(pp, count, res):
    """Fabricated volumes (invalid probes with NaN coefficients among them) and hashed atlases; a third of the probes asleep with
    records of NaN: nothing of them may reach a result."""
    n = count[0] * count[1] * count[2]
    d = P.desc((0.25, -1.0, 2.0), (0.5, 1.25, 0.75), count)
    vol = np.array(P.fabricated_volume(count, 8), F).reshape(n, 28)
    placement = some_placement(d, 59, asleep=3)
    vol[PP.state(placement) != 0] = np.nan
    atl = V.hashed_atlas(n, res, 4)
    pts = P.sample_points(d, 900, 13)
    for flags in (dict(), dict(backface=False), dict(chebyshev=False), dict(backface=False, chebyshev=False)):
        v = V.vis(res=res, normal_bias=0.03, **flags)
        want = PP.sample(d, v, vol, atl, pts, placement)
        assert (want[:, 3] > 0).any()
        got = pp.sample_probes_visible(on_gpu(shaped(d, vol, 28)), on_gpu(shaped(d, atl, res + 2, res + 2, 2)), d["origin"], d["spacing"], on_gpu(pts),
                                       normal_bias=0.03, placement=on_gpu(shaped(d, placement, 4)), **flags).cpu().numpy()
        assert_bits_or_nan(got, want, f"placed look-up {count} res {res} {flags}, device arrays")
    finite = np.where(np.isfinite(vol), vol, F(0.5)).astype(F)            # (host arrays: the same records without the poison)
    want = PP.sample(d, V.vis(res=res, normal_bias=0.03), finite, atl, pts, placement)
    got = pp.sample_probes_visible(shaped(d, finite, 28), shaped(d, atl, res + 2, res + 2, 2), d["origin"], d["spacing"], pts, normal_bias=0.03,
                                   placement=shaped(d, placement, 4))
    assert_bits_or_nan(got, want, f"placed look-up {count} res {res}, host arrays")


# ------------------------------------------------------------------------------------------------------------------ 6. the purpose

def cube_scene():
    """test_probe_place_host's cube of width 0.8 with its -x face at x = -0.1, outward normals (edge1 x edge2); a small emitter three
    spacings above, outside every probe's cells"""
    s = host.Scene()
    s.set_camera((2.5, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 60.0)
    white, light = s.add_diffuse((0.7, 0.7, 0.7)), s.add_emissive((10.0, 10.0, 10.0))
    x0, x1, y0, y1 = -0.1, 0.7, -0.4, 0.4
    w = 0.8
    s.add_quad((x0, y0, y0), (0, 0, w), (0, w, 0), white)               # x = x0, -x
    s.add_quad((x1, y0, y0), (0, w, 0), (0, 0, w), white)               # x = x1, +x
    s.add_quad((x0, y0, y0), (w, 0, 0), (0, 0, w), white)               # y = y0, -y
    s.add_quad((x0, y1, y0), (0, 0, w), (w, 0, 0), white)               # y = y1, +y
    s.add_quad((x0, y0, y0), (0, w, 0), (w, 0, 0), white)               # z = y0, -z
    s.add_quad((x0, y0, y1), (w, 0, 0), (0, w, 0), white)               # z = y1, +z
    s.add_quad((0.9, 3.0, -0.1), (0.2, 0, 0), (0, 0, 0.2), light)       # the emitter, -y
    return s.compile()


def test_the_cube_end_to_end():
    """The outcome test_probe_place_host predicts from a brute-force trace: probe 0 leaves the cube in one step and is awake after the
    next; probe 1 stands outside and stays; probe 2 has no surface within a spacing and sleeps - and the placed update then traces two
    probes, not three."""
    desc = dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(3, 1, 1), seed=11, seed_stride=5)
    vis = dict(res=8, rays_per_texel=2, max_distance=10.0)
    with device.Renderer(0) as r:
        r.upload_scene(cube_scene())
        p1 = r.place_probes(desc, vis, r.new_placement((3, 1, 1)), frame=0, frame_stride=1, min_front_distance=0.2)
        assert PP.state(p1).tolist() == [1, 0, 1]
        o = p1.reshape(3, 4)
        assert o[0, 0] < -0.1 and np.abs(o[0, 0:3]).max() <= 0.45 and not o[1:, 0:3].any()
        p2 = r.place_probes(desc, vis, p1, frame=1, frame_stride=1, min_front_distance=0.2)
        assert PP.state(p2).tolist() == [0, 0, 1]
        vol, stats = r.update_probes(desc, nan_like((1, 1, 3, 28)), SPP, frame=0, hysteresis=0.0, placement=p2, stats=True)
        assert stats["paths"] == 2 * SPP and np.isfinite(vol.reshape(3, 28)[0:2]).all() and (vol.reshape(3, 28).view(U)[2] == 0x7FA12345).all()
