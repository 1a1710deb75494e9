"""The reference of the mesh-scale light-map tests, without a GPU: lightmap_ref.coverage_owner_batched (vectorised over triangles,
candidates by np.searchsorted on the centres) equals coverage_owner (one triangle at a time, the closed box by comparing every
centre) word for word on every scene the GPU tests use it or its sibling on; the mesh-scale scene holds what
test_lightmap_scale_gpu.py needs of it, on the reference alone; and the time the batched reference takes there is printed."""
import time

import numpy as np
import pytest

import lightmap_ref as LR
import lightmap_scenes as LS

U, F = np.uint32, np.float32
NONE = LR.NONE

NARROW = [(16384, 1), (1, 16384), (16384, 3), (5, 16384)]


def both(cs, W, H, **kw):
    a = LR.coverage_owner(cs.triangles, cs.vertices, W, H, **kw)
    b = LR.coverage_owner_batched(cs.triangles, cs.vertices, W, H, **kw)
    assert a.dtype == b.dtype == U and a.shape == b.shape == (H, W)
    assert np.array_equal(a, b), (W, H, kw, int((a != b).sum()), np.argwhere(a != b)[:4].tolist())
    return a


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (64, 64), (257, 131)])
def test_batched_equals_per_triangle_on_the_edge_scene(W, H):
    """Every named case - NaN, inf and huge finite uv, boxes that end outside the atlas - and both parts of the batched route: with
    small = 64 the large footprints go through covers, with small = 2^30 every triangle is a batch of pairs, with small = 0 none is."""
    cs, case = LS.edge_scene()
    want = both(cs, W, H)
    for small in (0, 1 << 30):
        assert np.array_equal(LR.coverage_owner_batched(cs.triangles, cs.vertices, W, H, small=small), want), small
    both(cs, W, H, first=3, num=11)
    both(cs, W, H, first=len(LS.EDGE_CASES) - 1)
    owned = lambda name: int((want == case[name]).sum())  # noqa: E731
    assert owned("huge finite uv 3e38") == 0                            # inf - inf in its edge values: nothing is >= 0 or <= 0
    if (W, H) == (257, 131):                                            # the two wedges: the last and the first column alone
        assert (want[:, 256] == case["huge finite uv 1e30"]).sum() == owned("huge finite uv 1e30") >= 4
        assert (want[:, 0] == case["huge negative uv"]).sum() == owned("huge negative uv") >= 4
    if (W, H) == (64, 64):
        assert (want[63] == case["just outside"]).sum() > 50            # the top row, the corners or all but them
        pts, owner = LR.texels(cs.triangles, cs.vertices, W, H)
        assert np.isfinite(pts[:, 0:6]).all()
        for a, b in zip((pts, owner), LR.texels(cs.triangles, cs.vertices, W, H, batched=True)):
            assert np.array_equal(a.view(U), b.view(U))


def test_batched_equals_per_triangle_on_20000_sub_texel_triangles():
    cs = LS.tiny_scene()
    want = both(cs, 512, 512)
    assert 500 < (want != NONE).sum() < 10000
    both(cs, 512, 512, first=64 * 100 + 5, num=6000)


@pytest.mark.parametrize("W,H", NARROW)
def test_batched_equals_per_triangle_on_the_edge_scene_laid_out_for_16384(W, H):
    """... and the per-centre cases do what edge_scene_at says: at each listed texel of the long axis the owner along that axis is
    the FIRST triangle with d = 0 (the fifth of the texel's ten), whose side lies exactly on the centre - the four before it
    have their side one or two ulps past the centre and must not cover it."""
    n = 16384
    cs, case = LS.edge_scene_at(n, 0 if W == n else 1)
    want = both(cs, W, H)
    line = want[H // 2] if W == n else want[:, W // 2]                  # the middle centre of the short axis is 0.5
    for k, i in enumerate(LS.CENTRE_TEXELS(n)):
        assert line[i] == 10 * k + 4, (k, i, int(line[i]))
    assert case["quad lower"] == 10 * 6 and (want != NONE).sum() > 1000
    if (W, H) == (16384, 3):                                            # the wedges at this size: 82 columns of the rows v = 1 / 2 and 1 / 6
        assert (want[1, 16302:16380] == case["huge finite uv 1e30"]).all() and (want[0, 2:82] == case["huge negative uv"]).all()


def test_the_mesh_scale_scene_and_the_time_of_its_reference():
    """The scene of test_lightmap_scale_gpu.py for a card of 256 compute units (524 389 triangles) on 1024 x 1024: batched equals
    per-triangle on a range that holds large, sub-texel and two-centre triangles; the conditions the GPU test re-checks for its own
    card hold on the reference alone; the batched reference's time is printed (a few seconds: the GPU test computes it once)."""
    n, trip = LS.scale_count(256)
    large = LS.scale_large(trip)
    side = 1024
    uv, where = LS.scale_scene_uv(n, side, trip, large)
    vt = np.zeros((3 * n, 8), F)
    vt[:, 3], vt[:, 7] = uv[:, :, 0].ravel(), uv[:, :, 1].ravel()
    tri = np.arange(3 * n).reshape(-1, 3)
    t0 = time.time()
    owner = LR.coverage_owner_batched(tri, vt, side, side)
    dt = time.time() - t0
    print(f"{n} triangles on {side} x {side}: batched reference {dt:.2f} s, {(owner != NONE).sum()} owned texels")
    lo = 2047 * 64                                                       # groups 2047 and 2048 with their two large triangles
    a = LR.coverage_owner(tri, vt, side, side, first=lo, num=3000)
    assert np.array_equal(a, LR.coverage_owner_batched(tri, vt, side, side, first=lo, num=3000))
    assert {large[1], large[2]} <= set(np.unique(a).tolist())
    LS.check_scale_conditions(owner, 0, n, trip, where)
