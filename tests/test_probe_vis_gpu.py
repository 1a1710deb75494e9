"""hj_probe_visibility_rays, hj_bake_probe_visibility and hj_sample_probes_visible on the GPU, bit for bit against probe_vis_ref: the
rays of every map size at 1, 3 and 64 rays a texel through a probe window that does not start at 0; the bake as rays -> trace_rays ->
reduce on two scenes, with hits, misses and clamps, and over more than one slab; the look-up on fabricated volumes and atlases - moments
with m2 < m1^2, zeros, an infinity, a NaN - at points inside, on probes, one bias behind a probe, on cell faces and outside, with every
combination of the two switches; with both off the plain look-up; guard words and refused calls; and a light leak through a thin
wall, closed end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import path_query_ref as R
import probe_ref as P
import probe_vis_ref as V
from hijiki_amd import abi, device, host
from test_probes_gpu import assert_bits, grid_kw

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SEED, STRIDE = 0xFFFFFFF0, 7                                            # (the seed wraps inside the second probe's rays at the latest)
DEV = abi.PROBE_VIS_DEVICE_ARRAYS


@pytest.fixture(scope="module")
def pv():
    with device.Renderer(0) as ctx:
        yield ctx


def assert_bits_or_nan(got, want, what):
    """assert_bits where a NaN stands for any NaN: the words that are NaN are the same words, every other word is equal bit for bit.
    IEEE 754 leaves the sign and payload of a NaN an operation makes to the machine (x86 makes 0xFFC00000, the GPU 0x7FC00000), so
    the header defines a NaN result - a point with a non-finite position on the device route - as a NaN and no further."""
    got, want = np.array(got, F), np.array(want, F)
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), (what, np.flatnonzero(np.isnan(got) != np.isnan(want))[:8])
    got[np.isnan(got)] = 0
    want[np.isnan(want)] = 0
    assert_bits(got, want, what)


def vis_kw(v):
    return dict(res=v["res"], rays_per_texel=v["s"], max_distance=v["max_distance"])


# ------------------------------------------------------------------------------------------------------------------------ rays

@pytest.mark.parametrize("s", [1, 3, 64])
@pytest.mark.parametrize("res", [4, 8, 16])
def test_rays_match_the_reference(pv, res, s):
    """a 2 x 2 x 3 grid, the probes 3 ... 9 of it: host arrays, device arrays, and through the raw entry point into the middle of a
    larger device buffer whose words before and behind stay as they were.  No scene is needed."""
    import torch
    d = P.desc((-1.25, 0.5, 3.0), (0.3, 0.7, 0.011), (2, 2, 3), SEED, STRIDE)
    v = V.vis(res, s, 2.5)
    first, num = 3, 7
    want = V.rays(d, v, first, num)
    assert want.shape == (num * res * res * s, 8) and (want[:, 6] == 0).all() and (want[:, 7] == F(2.5)).all()
    kw = dict(grid_kw(d, seed=SEED, seed_stride=STRIDE), **vis_kw(v), first_probe=first, num_probes=num)
    assert_bits(pv.probe_visibility_rays(**kw), want, f"rays res {res} s {s}, host arrays")
    t = pv.probe_visibility_rays(**kw, device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert_bits(t.cpu().numpy(), want, f"rays res {res} s {s}, device arrays")
    guard = 64
    buf = torch.full((len(want) + 2 * guard, 8), 7.0, dtype=torch.float32, device=t.device)
    torch.cuda.synchronize()
    dd, vv = P.abi_desc(tuple(d["origin"]), tuple(d["spacing"]), d["count"], SEED, STRIDE, 0.0, abi.PROBES_DEVICE_ARRAYS), V.abi_vis(res, s, 2.5, 0.0, DEV)
    assert device.lib().hj_probe_visibility_rays(pv._h, C.byref(dd), C.byref(vv), first, num, buf.data_ptr() + guard * 32) == abi.HJ_OK
    got = buf.cpu().numpy()
    assert_bits(got[guard:-guard], want, f"rays res {res} s {s}, raw call")
    assert (got[:guard] == 7.0).all() and (got[-guard:] == 7.0).all()
    # nothing to do: HJ_OK, nothing touched, no array needed
    assert device.lib().hj_probe_visibility_rays(pv._h, C.byref(dd), C.byref(vv), 12, 0, None) == abi.HJ_OK
    if s == 64:
        assert pv.probe_visibility_rays(**dict(kw, first_probe=12, num_probes=0)).shape == (0, 8)


# ------------------------------------------------------------------------------------------------------------------------ bake

@pytest.mark.parametrize("name,count,res,s,far", [("cbox", (3, 2, 2), 4, 3, 0.75), ("rich", (2, 3, 2), 16, 1, 0.75), ("cbox", (2, 2, 3), 16, 1, 1e18),
                                                  ("rich", (3, 2, 2), 4, 3, 1e18)])
def test_bake_matches_rays_trace_reduce(pv, name, count, res, s, far):
    """The atlas against probe_vis_ref.rays -> Renderer.trace_rays -> probe_vis_ref.reduce.  max_distance = `far` of the domain's
    smallest extent (0.75: shorter than the room, so rays end in the air and hits beyond do not count), or the largest allowed."""
    cs = R.scene(name)
    pv.upload_scene(cs)
    d = P.grid_in_domain(cs, count, SEED, STRIDE)
    lo, hi = R.domain(cs)
    md = far if far > 1e17 else float((hi - lo).min()) * far
    v = V.vis(res, s, md)
    rays = V.rays(d, v)
    ids, t = pv.trace_rays(rays)[0:2]
    want = V.reduce((ids, t), v)
    got = pv.bake_probe_visibility(**grid_kw(d, seed=SEED, seed_stride=STRIDE), **vis_kw(v))
    assert got.shape == (count[2], count[1], count[0], res + 2, res + 2, 2)
    assert_bits(got.reshape(-1, 2), want.reshape(-1, 2), f"bake {name} res {res} s {s} max_distance {md}, host arrays")
    tt = pv.bake_probe_visibility(**grid_kw(d, seed=SEED, seed_stride=STRIDE), **vis_kw(v), device=True)
    assert_bits(tt.cpu().numpy().reshape(-1, 2), want.reshape(-1, 2), f"bake {name} res {res} s {s}, device arrays")
    hit = (ids >= 0).reshape(-1, s)
    print(f"{name} {count} res {res} s {s} max_distance {md:g}: {int(hit.sum())} of {hit.size} rays hit; m1 in {want[..., 0].min():g} ... {want[..., 0].max():g}")
    if far < 1e17:
        interior = got[..., 1:-1, 1:-1, :].reshape(-1, 2)
        full_miss, some_hit = (interior[:, 0] == F(md)), (interior[:, 0] < F(md))
        assert hit.any() and (~hit).any() and full_miss.any() and some_hit.any()
        assert (got[..., 0] <= F(md)).all() and (got[..., 0] > 0).all()
    else:
        assert hit.any() and np.isfinite(got).all()                    # (a miss: 1e18 and its square, finite in float32)


def test_bake_over_several_slabs_is_the_composition_by_windows(pv):
    """res 16 at 64 rays a texel: 16384 rays a probe, so a slab of HJ_PROBE_VIS_SLAB_RAYS rays holds `per` probes; 2 per + 5 probes are two
    full slabs and a partial one.  Against rays -> trace_rays on the device -> reduce for probe windows that are no slabs."""
    res, s = 16, 64
    per = abi.PROBE_VIS_SLAB_RAYS // (res * res * s)
    n = 2 * per + 5
    assert per >= 1 and n <= 1024
    cs = R.scene("cbox")
    pv.upload_scene(cs)
    d = P.grid_in_domain(cs, (n, 1, 1), SEED, STRIDE)
    v = V.vis(res, s, 1e18)
    kw = dict(grid_kw(d, seed=SEED, seed_stride=STRIDE), **vis_kw(v))
    got = pv.bake_probe_visibility(**kw)
    cuts = [0, per - 3, 2 * per + 1, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        rays = pv.probe_visibility_rays(**kw, first_probe=a, num_probes=b - a, device=True)
        ids, t = pv.trace_rays(rays)[0:2]
        parts.append(V.reduce((ids.cpu().numpy(), t.cpu().numpy()), v))
    want = np.concatenate(parts, 0)
    assert_bits(got.reshape(-1, 2), want.reshape(-1, 2), f"bake of {n} probes in slabs of {per}")
    tt = pv.bake_probe_visibility(**kw, device=True)
    assert_bits(tt.cpu().numpy().reshape(-1, 2), want.reshape(-1, 2), f"bake of {n} probes in slabs of {per}, device arrays")
    assert len(np.unique(got.reshape(n, -1), axis=0)) == n               # (every probe its own map: no slab written twice)


def test_bake_needs_a_scene_and_sample_does_nothing_with_no_points():
    import torch
    with device.Renderer(0) as r:
        atlas = np.full((8, 72), 7.0, F)
        dd, vv = P.abi_desc(), V.abi_vis(4, 1, 5.0)
        assert device.lib().hj_bake_probe_visibility(r._h, C.byref(dd), C.byref(vv), atlas.ctypes.data) == abi.HJ_ERR_STATE
        assert b"hj_bake_probe_visibility" in device.lib().hj_last_error(r._h) and (atlas == 7.0).all()
        assert device.lib().hj_sample_probes_visible(r._h, C.byref(dd), C.byref(vv), None, None, None, 0, None) == abi.HJ_OK
        vol, out = np.full((8, 28), 7.0, F), np.full((4, 4), 7.0, F)
        assert device.lib().hj_sample_probes_visible(r._h, C.byref(dd), C.byref(vv), vol.ctypes.data, atlas.ctypes.data, out.ctypes.data, 0, out.ctypes.data) == abi.HJ_OK
        assert (out == 7.0).all() and (vol == 7.0).all()
        t = r.sample_probes_visible(torch.zeros((2, 2, 2, 28), device="cuda:0"), torch.zeros((2, 2, 2, 6, 6, 2), device="cuda:0"), (0, 0, 0), (1, 1, 1),
                                    torch.zeros((0, 8), device="cuda:0"))
        assert tuple(t.shape) == (0, 4)


# --------------------------------------------------------------------------------------------------------------------- look-up

def lookup_points(d, bias, n=390, seed=3):
    """probe_ref.sample_points with non-finite positions, and by hand: exactly on probes (every normal axis), exactly one bias behind
    a probe (x = P - nn * bias in float32, so that xb lands on or within an ulp of the probe), on cell faces, outside on every side"""
    pts = [P.sample_points(d, n, seed, nonfinite=True)]
    cnt = np.array(d["count"])
    probes = P.points(d)[:, 0:3]
    rng = np.random.default_rng([seed, 99])
    pick = probes[rng.integers(0, len(probes), 12)]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    hand = np.zeros((12 + 12 + 12 + 6, 8), F)
    hand[0:12, 0:3], hand[0:12, 3:6] = pick, axes[np.arange(12) % 6]
    nn = axes[np.arange(12) % 6]
    hand[12:24, 0:3], hand[12:24, 3:6] = (pick - nn * F(bias)).astype(F), nn
    face = probes[rng.integers(0, len(probes), 12)].astype(np.float64)
    face[:, 1:3] += rng.uniform(0.1, 0.9, (12, 2)) * d["spacing"][1:3]                    # on an x plane, inside a cell in y and z
    hand[24:36, 0:3], hand[24:36, 3:6] = face, rng.normal(size=(12, 3))
    hi = d["origin"] + (cnt - 1) * d["spacing"]
    mid = (d["origin"] + hi) / 2
    for k in range(6):
        p = mid.astype(np.float64).copy()
        p[k // 2] = (d["origin"][k // 2] - 2.5 * d["spacing"][k // 2]) if k % 2 == 0 else (hi[k // 2] + 2.5 * d["spacing"][k // 2])
        hand[36 + k, 0:3], hand[36 + k, 3:6] = p, axes[k]
    pts.append(hand)
    return np.concatenate(pts, 0)


@functools.lru_cache(maxsize=None)
def lookup_case(count, res):
    d = P.desc((0.5, -1.0, 2.0), (0.5, 0.25, 1.5), count)
    n = count[0] * count[1] * count[2]
    vol = P.fabricated_volume(count, 9)
    vol2 = P.hashed_records(np.arange(n)).reshape(count[2], count[1], count[0], 28)
    atlas = V.hashed_atlas(n, res, 5).reshape(count[2], count[1], count[0], res + 2, res + 2, 2)
    pts = lookup_points(d, 0.125)
    for a in (vol, vol2, atlas, pts):
        a.setflags(write=False)
    return d, vol, vol2, atlas, pts


@pytest.mark.parametrize("count", [(5, 4, 3), (3, 1, 4)])
@pytest.mark.parametrize("res", [4, 8, 16])
def test_lookup_matches_the_reference(pv, res, count):
    """every combination of the two switches, on device arrays (with NaN and infinite positions) and on host arrays (the finite rows)"""
    import torch
    d, vol, vol2, atlas, pts = lookup_case(count, res)
    finite = np.isfinite(pts[:, 0:3]).all(1)
    dev = torch.device("cuda", 0)
    for volume in (vol, vol2):
        tv, ta, tp = (torch.from_numpy(np.array(a)).to(dev).contiguous() for a in (volume, atlas, pts))
        for backface in (True, False):
            for chebyshev in (True, False):
                v = V.vis(res, normal_bias=0.125, backface=backface, chebyshev=chebyshev)
                want, wb, wv = V.sample(d, v, volume, atlas, pts, detail=True)
                what = f"look-up {count} res {res} backface {backface} chebyshev {chebyshev}"
                got = pv.sample_probes_visible(tv, ta, d["origin"], d["spacing"], tp, normal_bias=0.125, backface=backface, chebyshev=chebyshev)
                assert_bits_or_nan(got.cpu().numpy(), want, what + ", device arrays")
                got = pv.sample_probes_visible(volume, atlas, d["origin"], d["spacing"], pts[finite], normal_bias=0.125, backface=backface,
                                               chebyshev=chebyshev)
                assert_bits(got, want[finite], what + ", host arrays")
                assert np.isfinite(want[finite]).all(), what              # (a NaN result only where the position is none)
                if chebyshev:
                    assert (wv == F(0.05)).any() and (wv == 1).any() and ((wv > F(0.05)) & (wv < 1)).any(), what
    # the hand-made rows did what they are for: on a probe wb = 1 for that corner and wv = 1 one bias behind it
    v = V.vis(res, normal_bias=0.125)
    _, wb, wv = V.sample(d, v, vol, atlas, pts, detail=True)
    base = len(pts) - 42
    assert ((wb[base:base + 12] == 1).sum(1) >= 1).all()


@pytest.mark.parametrize("count", [(5, 4, 3), (3, 1, 4)])
def test_both_factors_off_is_the_plain_lookup(pv, count):
    """with both NO_ flags and no atlas at all: Renderer.sample_probes, bit for bit, on both routes"""
    import torch
    d, vol, vol2, atlas, pts = lookup_case(count, 8)
    finite = np.isfinite(pts[:, 0:3]).all(1)
    dev = torch.device("cuda", 0)
    for volume in (vol, vol2):
        tv, tp = (torch.from_numpy(np.array(a)).to(dev).contiguous() for a in (volume, pts))
        plain = pv.sample_probes(tv, d["origin"], d["spacing"], tp).cpu().numpy()
        got = pv.sample_probes_visible(tv, None, d["origin"], d["spacing"], tp, normal_bias=0.5, backface=False, chebyshev=False)
        assert_bits(got.cpu().numpy(), plain, f"both factors off {count}, device arrays")
        plain = pv.sample_probes(volume, d["origin"], d["spacing"], pts[finite])
        got = pv.sample_probes_visible(volume, None, d["origin"], d["spacing"], pts[finite], normal_bias=0.5, backface=False, chebyshev=False)
        assert_bits(got, plain, f"both factors off {count}, host arrays")


def test_lookup_leaves_the_words_around_its_output_alone(pv):
    import torch
    d, vol, _, atlas, pts = lookup_case((5, 4, 3), 8)
    dev = torch.device("cuda", 0)
    tv, ta, tp = (torch.from_numpy(np.array(a)).to(dev).contiguous() for a in (vol, atlas, pts))
    guard = 16
    buf = torch.full((len(pts) + 2 * guard, 4), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    dd = P.abi_desc(tuple(d["origin"]), tuple(d["spacing"]), d["count"], 0, 1, 0.0, abi.PROBES_DEVICE_ARRAYS)
    vv = V.abi_vis(8, 1, 1.0, 0.125, DEV)
    rc = device.lib().hj_sample_probes_visible(pv._h, C.byref(dd), C.byref(vv), tv.data_ptr(), ta.data_ptr(), tp.data_ptr(), len(pts), buf.data_ptr() + guard * 16)
    assert rc == abi.HJ_OK
    got = buf.cpu().numpy()
    assert_bits_or_nan(got[guard:-guard], V.sample(d, V.vis(8, normal_bias=0.125), vol, atlas, pts), "look-up, raw call")
    assert (got[:guard] == 7.0).all() and (got[-guard:] == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------ light leak

def two_rooms():
    """A closed box 4 x 2 x 2 cut in two at x = 2 by a wall 0.1 thick; an emitter under the ceiling of the room x < 2 alone."""
    s = host.Scene()
    s.set_camera((1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0), 60.0)
    white, light = s.add_diffuse((0.7, 0.7, 0.7)), s.add_emissive((12.0, 12.0, 12.0))
    # every face looks into its room: edge1 x edge2 is the normal
    s.add_quad((0, 0, 0), (0, 0, 2), (4, 0, 0), white)                  # floor, +y
    s.add_quad((0, 2, 0), (4, 0, 0), (0, 0, 2), white)                  # ceiling, -y
    s.add_quad((0, 0, 0), (4, 0, 0), (0, 2, 0), white)                  # z = 0, +z
    s.add_quad((0, 0, 2), (0, 2, 0), (4, 0, 0), white)                  # z = 2, -z
    s.add_quad((0, 0, 0), (0, 2, 0), (0, 0, 2), white)                  # x = 0, +x
    s.add_quad((4, 0, 0), (0, 0, 2), (0, 2, 0), white)                  # x = 4, -x
    s.add_quad((1.95, 0, 0), (0, 0, 2), (0, 2, 0), white)               # the wall's two faces: -x into the lit room,
    s.add_quad((2.05, 0, 0), (0, 2, 0), (0, 0, 2), white)               # +x into the dark one
    s.add_quad((0.6, 1.99, 0.6), (0.8, 0, 0), (0, 0, 0.8), light)       # the emitter, -y
    return s.compile()


def test_visibility_closes_a_light_leak_through_a_thin_wall(pv):
    """Probes 1 apart at x = 0.5, 1.5 | 2.5, 3.5: the wall (0.1 thick, thinner than the spacing) stands between the second and the
    third plane.  At points of the dark room within one spacing of the wall the plain look-up shows light - the lit room's probes,
    interpolated through the wall -, the visible one less at every point, with the Chebyshev factor of every corner across the wall at
    its floor 0.05 and 1 for the corners in the room; in the lit room, more than a spacing from the wall, every corner's is 1.  (The
    geometry was chosen with probe_vis_ref over an analytic trace of these boxes: the cubed bound stays below 0.01 across the wall.)"""
    pv.upload_scene(two_rooms())
    grid = dict(origin=(0.5, 0.5, 0.5), spacing=(1.0, 1.0, 1.0), count=(4, 2, 2))
    d = P.desc(grid["origin"], grid["spacing"], grid["count"], seed=11, seed_stride=1000003)
    v = V.vis(16, 4, 8.0, normal_bias=0.02)
    volume = pv.bake_probes(**grid, spp=512, seed=5, seed_stride=977, opts=R.options(40))
    atlas = pv.bake_probe_visibility(**grid, **vis_kw(v), seed=11, seed_stride=1000003)
    assert (volume[..., 27] == 1).all()
    lum = lambda o: 0.2126 * o[:, 0].astype(np.float64) + 0.7152 * o[:, 1] + 0.0722 * o[:, 2]      # noqa: E731
    rng = np.random.default_rng(3)
    n = 64
    dark = np.zeros((n, 8), F)
    dark[:, 0], dark[:, 1:3] = rng.uniform(2.25, 2.45, n), rng.uniform(0.7, 1.3, (n, 2))
    dark[:n // 2, 3], dark[n // 2:3 * n // 4, 4], dark[3 * n // 4:, 5] = 1.0, 1.0, -1.0    # facing away from the wall (+x), and along it (+y, -z)
    plain = pv.sample_probes(volume, grid["origin"], grid["spacing"], dark)
    seen = pv.sample_probes_visible(volume, atlas, grid["origin"], grid["spacing"], dark, normal_bias=0.02)
    want, wb, wv = V.sample(d, v, volume, atlas, dark, detail=True)
    assert_bits(seen, want, "the dark room's points")
    print("dark room: plain luminance", lum(plain).min(), "...", lum(plain).max(), "visible", lum(seen).min(), "...", lum(seen).max())
    assert (lum(plain) > 0).all(), "no leak to close: the plain look-up is dark already"
    assert (lum(seen) < lum(plain)).all()
    assert (wv[:, 0::2] == F(0.05)).all()                               # dx = 0: the probes at x = 1.5, across the wall
    assert (wv[:, 1::2] == 1).all()                                     # dx = 1: the probes at x = 2.5, in the room
    lit = np.zeros((n, 8), F)
    lit[:, 0], lit[:, 1:3], lit[:, 3:6] = rng.uniform(0.55, 0.9, n), rng.uniform(0.7, 1.3, (n, 2)), rng.normal(size=(n, 3))
    got = pv.sample_probes_visible(volume, atlas, grid["origin"], grid["spacing"], lit, normal_bias=0.02)
    want, wb, wv = V.sample(d, v, volume, atlas, lit, detail=True)
    assert_bits(got, want, "the lit room's points")
    assert (wv == 1).all()
