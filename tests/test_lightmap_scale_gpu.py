"""The light-map texel kernels at mesh scale and at the atlas limits, bit for bit against lightmap_ref: a mesh sized from the card's
compute units so that both owner kernels take a second trip of their outer loops (default launch, a sub-range, every box by
waves, every box by one lane); the edge scene re-laid for 16384 texels on atlases 16384 long and 1, 3 and 5 wide; an atlas at both
limits at once (16384 x 4096 = 2^26 texels, 262 144 scan tiles); the dilation and both forms of the filter at 16384 x 1 and
1 x 16384.  The arithmetic of each docstring is for a card of 256 compute units (MI355X); the tests take the count from the card."""
import time

import numpy as np
import pytest

import lightmap_filter_ref as FR
import lightmap_ref as LR
import lightmap_scenes as LS
import path_query_ref as R
from hijiki_amd import device
from test_lightmap_filter_gpu import assert_image
from test_lightmap_gpu import assert_texels, compose

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
NONE = LR.NONE
SIDE = 1024                                                              # the mesh-scale atlas: 2^20 texels, 4096 scan tiles


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_scale = {}


def scale_case(sub=False):
    """-> (shapes, (points, owner) of the batched reference, keywords of the call); sub: the range [69, 69 + trip + 30)"""
    if "scene" not in _scale:
        n, trip = LS.scale_count(cus())
        assert n > 64 * 2048, f"{n} triangles on a card of {cus()} compute units: k_lm_owner_wide would take one trip"
        _scale["scene"] = LS.scale_scene(n, SIDE, trip, LS.scale_large(trip)) + (n, trip)
    cs, where, n, trip = _scale["scene"]
    if sub not in _scale:
        first, num = (64 * 1 + 5, trip + 30) if sub else (0, 0)
        t0 = time.time()
        want = LR.texels(cs.triangles, cs.vertices, SIDE, SIDE, first=first, num=num, batched=True)
        count = LS.check_scale_conditions(want[1], first, first + num if num else n, trip, where)
        print(f"{n} triangles, range from {first}, {num or n} long: {count} owned texels, reference {time.time() - t0:.2f} s")
        assert count == len(want[0])                                    # (no normal of this scene drops a texel)
        for a in want:
            a.setflags(write=False)
        _scale[sub] = want
    return cs, _scale[sub], dict(first_triangle=64 * 1 + 5, num_triangles=trip + 30) if sub else {}


def upload(r, cs):
    """The tree is built on the device and stays there (tens of milliseconds at this size; the host's builder takes seconds for
    half a million shapes, and the texel kernels read no tree - a query just needs a scene uploaded)."""
    r.build_bvh(cs, keep_on_device=True)
    r.upload_scene(cs, device_tree=True)


@pytest.fixture(scope="module")
def lm():
    with device.Renderer(0) as ctx:
        yield ctx


@pytest.mark.parametrize("sub", [False, True], ids=["all", "from 69"])
def test_both_owner_kernels_take_a_second_trip(lm, sub):
    """n = 64 * 4 * 8 * cus + 64 + 37 triangles (cus = 256: 524 389, in 8194 groups of 64) on 1024 x 1024.
    k_lm_owner: gx = min(ceil(8194 / 4), 8 * 256) = 2048 workgroups, waves = 8192, so waves 0 and 1 take a second trip
    (base += waves * 64): group 8192, whole, and group 8193, 37 lanes - masks[base >> 6] is stored at 8192 and 8193, and the
    two-centre triangles there own texels only if a.first + (uint32_t)j is right on that trip.
    k_lm_owner_wide: wx = min(ceil(8194 / 256), 8) = 8, waves = 32 a row, 2048 groups a trip, five trips (g0 += waves * 64); the last
    starts at g0 = 8192 where g0 + lane < groups holds for lanes 0 and 1 alone.  Large triangles (box 14 x 14 > 64 texels) are
    marked in groups 0, 2047 (last of the first trip), 2048 (first of the second), 8192 and 8193; each loses a centre to triangle
    L - 1 and takes one from L + 1.
    'from 69': first_triangle = 64 * 1 + 5, num_triangles = trip + 30, 8193 groups - gx is still 2048 and the second trip is group
    8192 with 30 lanes, five wide trips; a.first is not 0 and no group of the range is a group of the scene."""
    cs, want, kw = scale_case(sub)
    upload(lm, cs)
    got = lm.lightmap_texels(SIDE, SIDE, owner=True, **kw)
    assert_texels(got, want, f"{len(cs.triangles)} triangles, {kw}")


@pytest.mark.parametrize("switch", ["HJ_LIGHTMAP_LANE_TEXELS=0", "HJ_LIGHTMAP_LANE_TEXELS=268435456"])
def test_the_split_never_shows_at_mesh_scale(monkeypatch, switch):
    """0: every box is marked - every mask word of the 8194 groups is full (the last: 37 bits) - and k_lm_owner_wide walks all 524 389
    triangles in its five trips.  2^28: no box is marked, the 14 x 14 boxes too are walked by their lanes, on both trips of
    k_lm_owner.  A context created under the setting against the reference computed on the host."""
    cs, want, _ = scale_case()
    monkeypatch.setenv(*switch.split("="))
    with device.Renderer(0) as r:
        upload(r, cs)
        assert_texels(r.lightmap_texels(SIDE, SIDE, owner=True), want, switch)


# ---------------------------------------------------------------------------------------------------------------- the atlas limits

N = 16384
_narrow = {}


def narrow_reference(W, H):
    if (W, H) not in _narrow:
        cs = LS.edge_scene_at(N, 0 if W == N else 1)[0]
        _narrow[W, H] = LR.texels(cs.triangles, cs.vertices, W, H, offset=1e-3)
        for a in _narrow[W, H]:
            a.setflags(write=False)
    return _narrow[W, H]


@pytest.mark.parametrize("W,H", [(16384, 1), (1, 16384), (16384, 3), (5, 16384)])
def test_edge_cases_on_atlases_16384_long(lm, W, H):
    """lm_axis_range at n = 16384: vmin * 16384 is exact (a power of two) and loses its low bits in the - 0.5 (an ulp of 2^-10 texel
    at 8192 ... 16384); the claim is that floor - 1 ... ceil + 1 still holds every centre the closed comparison accepts.  Sides one
    and two ulps before, on and behind the centres of texels 0, 1, 8191, 8192, 16382 and 16383, as a box's minimum and as its
    maximum: the owner says which of them covered.  The 19 named cases, huge finite uv among them, at this size; the other axis
    1, 3 or 5 texels, where every box is clamped on that axis."""
    cs = LS.edge_scene_at(N, 0 if W == N else 1)[0]
    lm.upload_scene(cs)
    want = narrow_reference(W, H)
    line = want[1][H // 2] if W == N else want[1][:, W // 2]
    assert [int(line[i]) for i in LS.CENTRE_TEXELS(N)] == [10 * k + 4 for k in range(6)] and len(want[0]) > 1000
    assert_texels(lm.lightmap_texels(W, H, offset=1e-3, owner=True), want, f"{W} x {H}")


def test_an_atlas_at_both_limits(lm):
    """16384 x 4096 = 2^26 texels, the most lightmap_atlas_check lets through: 262 144 scan tiles, so each of k_lm_scan's 256 threads
    owns a run of 1024 counts; y * W + x and the texel word up to 2^26 - 1, which is owned, as is texel 0; the first and the last
    scan tile hold texels, nearly all of the quarter million between them none; seed + t * seed_stride = 0xFFFFFFF0 + t * 0x10000001
    wraps 2^32 many times over.  The reference is the per-triangle route: it evaluates each of the 8 triangles on the centres of its
    own closed box alone (rows and columns by comparison, W + H values), and leaves NONE elsewhere."""
    cs = LS.limit_scene()
    lm.upload_scene(cs)
    W, H = 16384, 4096
    kw = dict(seed=0xFFFFFFF0, seed_stride=0x10000001)
    t0 = time.time()
    want = LR.texels(cs.triangles, cs.vertices, W, H, **kw)
    t1 = time.time()
    t = want[0].view(U)[:, 7]
    assert t[0] == 0 and t[-1] == W * H - 1 and (t < 256).sum() >= 20 and (t >= W * H - 256).sum() == 256 and 1000 < len(t) < 5000
    assert ((t > (1 << 25) - 2 * W) & (t < 1 << 25)).any() and ((t >= 1 << 25) & (t < (1 << 25) + 2 * W)).any()
    got = lm.lightmap_texels(W, H, owner=True, **kw)
    print(f"2^26 texels: {len(t)} owned, reference {t1 - t0:.2f} s, device (two passes, the 256 MB map to the host) {time.time() - t1:.2f} s")
    assert_texels(got, want, "16384 x 4096")


@pytest.mark.parametrize("gutter", [0, 1, 3])
@pytest.mark.parametrize("W,H", [(16384, 1), (1, 16384)])
def test_bake_on_an_atlas_one_texel_wide(lm, W, H, gutter):
    """k_lm_scatter and k_lm_dilate where one axis has no neighbour at all: 64 workgroups in a line, x + dx or y + dy outside the atlas
    for six of the eight neighbours of every texel.  hj_bake_lightmap (spp 2) against texels -> trace_irradiance -> the reference's
    scatter and dilation; the box scene's charts leave gaps of hundreds of texels along either axis, so gutter texels exist."""
    lm.upload_scene(LS.bake_scene())
    kw = dict(seed=11, seed_stride=7, offset=1e-3)
    want, _, n = compose(lm, W, H, 2, gutter, R.options(12), **kw)
    got = lm.bake_lightmap(W, H, 2, gutter=gutter, opts=R.options(12), **kw)
    assert_image(got, want, f"{W} x {H}, gutter {gutter}")
    assert 8000 < n < W * H and (got[:, :, 3] == 1).sum() == n and ((got[:, :, 3] == 0.5).sum() > 0) == (gutter > 0)


@pytest.mark.parametrize("step", ["0", "128"])
@pytest.mark.parametrize("W,H", [(16384, 1), (1, 16384)])
def test_filter_on_an_atlas_one_texel_wide(monkeypatch, W, H, step):
    """Both forms of the a-trous filter (HJ_LIGHTMAP_FILTER_LDS_STEP=0: direct at every step, 128: the LDS form, which stages a 32 x 8
    tile and its apron, at every step) on an image 1 texel high (512 tiles in a row, seven of a tile's eight rows outside) and 1 texel
    wide (2048 tiles in a column, 31 of 32 columns outside): three iterations, and eight, whose steps 1 ... 128 all exceed the short
    side.  Guides: the re-laid edge scene's texels; the image is fabricated."""
    cs = LS.edge_scene_at(N, 0 if W == N else 1)[0]
    pts = narrow_reference(W, H)[0]
    img = np.random.default_rng([W, H]).uniform(0.0, 2.0, (H, W, 4)).astype(F)
    monkeypatch.setenv("HJ_LIGHTMAP_FILTER_LDS_STEP", step)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        for f in ((3, 0.3, 0.5, 0.4), (8, 0.3, 0.5, 0.4)):
            assert_image(r.filter_lightmap(img, pts, *f), FR.run(img, pts, *f), f"HJ_LIGHTMAP_FILTER_LDS_STEP={step}, {W} x {H}, filter {f}")
