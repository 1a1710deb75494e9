"""hj_render_direct_lit, HJ_GATHER_INDIRECT and HJ_PROBES_INDIRECT_ONLY on the GPU, bit for bit against direct_lit_ref - the contract
restated in numpy over hj_trace_rays' own records and the oracle's shade step: the indirect gather, its adaptive form and the indirect
bake; the frames on three scenes under every lighting, spp and max_follow; the hj_trace_paths corollary; a scene without light against
hj_render_probe_lit; shadow-ray lists of exactly 0, 1, 255, 256, 257 and 513 entries, over several walk launches and two runs; an
occluder whose shadow is decided in float64 from the geometry; refusals and the empty list.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import direct_lit_ref as DL
import gather_ref as G
import path_query_ref as P
import probe_lit_ref as PL
import probe_ref as PR
from hijiki_amd import abi, device, host
from test_follow_gpu import block_list, gpu_trace, same_bits
from test_probe_lit_gpu import RES, sample_pixels, volume
from test_probes_gpu import SEED, STRIDE, assert_bits, grid_kw

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
GRID = "5x4x3"
KINDS = ("none", "plain", "visible", "placed")


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    assert all(hasattr(device.lib(), n) for n in ("hj_render_direct_lit", "hj_render_direct_lit_frame")) and hasattr(abi, "GATHER_INDIRECT")


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as r:
        yield r


def gpu_occluded(r):
    """the reference's occlusion test: hj_trace_rays any-hit over the shadow ray's range (the scene is uploaded on r)"""
    return lambda rays: r.trace_rays(np.ascontiguousarray(rays, F), any_hit=True)[0] >= 0


# ---------------------------------------------------------------------------------------------------------------------- gather

@functools.lru_cache(maxsize=None)
def expected_indirect(name, mode):
    spp, sphere, sh = G.MODES[mode]
    out, counts = DL.gather_indirect(P.scene(name), G.point_set(name), spp, sphere, sh, P.options(40))
    out.setflags(write=False)
    return out, counts


@pytest.mark.parametrize("mode", ["hemisphere-1", "sphere-sh9-4"])
@pytest.mark.parametrize("name", G.SCENES)
def test_the_indirect_gather_is_the_reference(rq, name, mode):
    spp, sphere, sh = G.MODES[mode]
    want, counts = expected_indirect(name, mode)
    rq.upload_scene(P.scene(name))
    pts = np.array(G.point_set(name))
    got, stats = rq.trace_irradiance(pts, spp=spp, sphere=sphere, sh9=sh, opts=P.options(40), stats=True, indirect=True)
    assert_bits(got, want, f"indirect gather, {name}, {mode}")
    assert {k: stats[k] for k in G.COUNTS} == {k: counts[k] for k in G.COUNTS}
    full = rq.trace_irradiance(pts, spp=spp, sphere=sphere, sh9=sh, opts=P.options(40))
    assert_bits(full, G.expected(name, mode)[0], f"without the flag, {name}, {mode}")                 # (one spot check of the unchanged gather)
    assert (got[:, 3:8].view(U) == full[:, 3:8].view(U)).all() and (got[:, 0:3] != full[:, 0:3]).any()


@pytest.mark.parametrize("name", G.SCENES)
def test_the_adaptive_indirect_gather_is_the_fixed_one_at_the_spp_each_point_got(rq, name):
    rq.upload_scene(P.scene(name))
    pts = np.array(G.point_set(name))
    got = rq.trace_irradiance_adaptive(pts, spp_min=4, spp_step=4, spp_max=16, rel_error=0.1, floor=0.05, opts=P.options(40), indirect=True)
    n = got[:, 3].astype(np.int64)
    print(f"{name}: samples a point {np.unique(n, return_counts=True)}")
    assert set(np.unique(n).tolist()) <= {4, 8, 12, 16}
    for c in np.unique(n):
        sel = n == c
        assert_bits(got[sel], rq.trace_irradiance(pts[sel], spp=int(c), opts=P.options(40), indirect=True), f"{name}: the points that got {c} samples")
    plain = rq.trace_irradiance_adaptive(pts, spp_min=4, spp_step=4, spp_max=16, rel_error=0.1, floor=0.05, opts=P.options(40))
    assert (plain[:, 0:3] != got[:, 0:3]).any()


def test_the_indirect_bake_is_the_resolve_of_the_indirect_gather(rq):
    cs = P.scene("cbox")
    d = PR.grid_in_domain(cs, (3, 3, 3), seed=SEED, seed_stride=STRIDE)
    spp = 4
    rec, counts = DL.gather_indirect(cs, PR.points(d), spp, True, True, P.options(40))
    want = PR.resolve(rec, spp, d["min_distance"])
    rq.upload_scene(cs)
    got, stats = rq.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=spp, opts=P.options(40), stats=True, indirect_only=True)
    assert got.shape == (3, 3, 3, 28)
    assert_bits(got.reshape(-1, 28), want, "indirect-only bake")
    assert {k: stats[k] for k in G.COUNTS} == {k: counts[k] for k in G.COUNTS}
    t = rq.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=spp, opts=P.options(40), device=True, indirect_only=True)
    assert_bits(t.cpu().numpy().reshape(-1, 28), want, "indirect-only bake, device arrays")
    # an update with hysteresis 0 writes the fresh bake: the flag reaches hj_update_probes' gather too (frame 0: the bake's seed)
    up = rq.update_probes(dict(grid_kw(d, seed=SEED, seed_stride=STRIDE)), np.zeros((3, 3, 3, 28), F), spp, frame=0, hysteresis=0.0, opts=P.options(40),
                          indirect_only=True)
    assert_bits(up.reshape(-1, 28), want, "hj_update_probes with HJ_PROBES_INDIRECT_ONLY, hysteresis 0")
    # without the flag: the bake it always was
    plain = rq.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=spp, opts=P.options(40))
    assert_bits(plain.reshape(-1, 28), PR.bake(cs, d, spp, P.options(40))[0], "the unchanged bake")
    assert (plain != got).any()


# ---------------------------------------------------------------------------------------------------------------------- frames

def passes(spp):
    return [(11 + 7 * k, (0.5 if k == 0 else 0.125 + 0.25 * k, 0.5 if k == 0 else 0.875 - 0.25 * k)) for k in range(spp)]


def lighting(kind):
    """-> (the reference's look-up or None, the wrapper's keywords)"""
    if kind == "none":
        return None, dict()
    d, v, vol, atlas, place = volume(GRID)
    n = vol.size // 28
    kw = dict(volume=vol, origin=d["origin"], spacing=d["spacing"], normal_bias=0.02)
    if kind == "plain":
        return PL.lookup(d, vol), kw
    if kind == "visible":
        return PL.lookup(d, vol, v, atlas.reshape(n, RES + 2, RES + 2, 2)), dict(kw, atlas=atlas)
    return PL.lookup(d, vol, v, atlas.reshape(n, RES + 2, RES + 2, 2), place.reshape(n, 4)), dict(kw, atlas=atlas, placement=place)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", G.SCENES)
def test_every_word_equals_the_restatement(rq, name, kind):
    cs = P.scene(name)
    W = H = 32
    look, kw = lighting(kind)
    env = rq.env_lookup if name == "env" else None
    for spp in (1, 3):
        blocks = block_list(W, H, 16, passes(spp))
        for follow in (0, 2):
            rq.upload_scene(cs)
            want, det = DL.render(cs, blocks, W, H, follow, gpu_trace(rq), gpu_occluded(rq), look, env, detail=True)
            wants, counts = det["wants"], det["counts"]
            if kind == "none":
                print(f"{name} x {spp} spp, max_follow {follow}: {int(wants.sum())} of {len(wants)} samples want a shadow ray, {int(counts.sum())} count")
            assert counts.sum() > 20 and (wants & ~counts).sum() > 0
            if name == "env":                                           # environment next-event samples: the shadow ray runs to infinity
                far = wants & (det["rays"][:, 7] == np.inf)
                assert far.sum() > 10 and (far & counts).sum() > 0
            rq.upload_scene(cs)
            same_bits(rq.render_direct_lit(W, H, blocks=blocks, follow=follow, **kw), want, f"{name} / {kind} / {spp} spp / max_follow {follow}")
    if kind == "placed":                                                # device arrays and the frame form, once a scene
        import torch
        dev = {k: torch.from_numpy(np.array(a)).to(f"cuda:{rq.device}") if k in ("volume", "atlas", "placement") else a for k, a in kw.items()}
        out = rq.render_direct_lit(W, H, blocks=blocks, follow=2, **dev)
        assert out.is_cuda
        same_bits(out.cpu().numpy(), want, f"{name} / device arrays")
        frame_blocks = list(host.make_blocks(W, H, 2, 21))
        same_bits(rq.render_direct_lit(W, H, spp=2, master_seed=21, follow=2, **kw), rq.render_direct_lit(W, H, blocks=frame_blocks, follow=2, **kw), "frame form")


@pytest.mark.parametrize("name", G.SCENES)
def test_without_a_volume_a_sample_is_hj_trace_paths_at_one_bounce(rq, name):
    """max_follow = 0, lighting NULL or an all-zero volume, 1 spp on disjoint blocks: a pixel IS its sample, and the sample is
    hj_trace_paths' radiance for its camera ray under its own seed at spp = 1, max_bounces = 1"""
    cs = P.scene(name)
    W = H = 32
    blocks = block_list(W, H, 16, passes(1))
    rq.upload_scene(cs)
    rays = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    paths = rq.trace_paths(rays, spp=1, opts=P.options(1))
    px = sample_pixels(blocks)
    want = np.zeros((H, W, 4), F)
    want[px[:, 0], px[:, 1], 0:3], want[..., 3] = paths[:, 0:3], 1.0
    assert (paths[:, 0:3] != 0).any(1).sum() > 100
    same_bits(rq.render_direct_lit(W, H, blocks=blocks), want, f"{name}: lighting NULL")
    d, v, vol, atlas, place = volume(GRID)
    same_bits(rq.render_direct_lit(W, H, volume=np.zeros_like(vol), origin=d["origin"], spacing=d["spacing"], blocks=blocks), want, f"{name}: an all-zero volume")


def test_a_scene_without_light_gives_hj_render_probe_lits_bits(rq):
    s = host.Scene()
    s.set_camera((0.0, 1.0, 3.0), (0, 0, 0, 1), 60.0)
    s.add_quad((-4, 0, 4), (8, 0, 0), (0, 0, -8), s.add_diffuse_cboard((0.9, 0.8, 0.2), 0.13, (0.1, 0.2, 0.8), 0.21))
    s.add_quad((-4, 0, -4), (8, 0, 0), (0, 8, 0), s.add_diffuse((0.5, 0.6, 0.7)))
    s.add_sphere((0.0, 1.0, 0.0), 0.8, s.add_mirror())
    cs = s.compile()
    W = H = 32
    blocks = block_list(W, H, 16, passes(2))
    _, kw = lighting("placed")
    rq.upload_scene(cs)
    vol_kw = {k: a for k, a in kw.items() if k not in ("volume", "origin", "spacing")}
    lit = rq.render_probe_lit(kw["volume"], kw["origin"], kw["spacing"], W, H, blocks=blocks, follow=2, **vol_kw)
    assert lit[..., 0:3].any()
    same_bits(rq.render_direct_lit(W, H, blocks=blocks, follow=2, **kw), lit, "no emitter, no environment")
    assert not rq.render_direct_lit(W, H, blocks=blocks, follow=2)[..., 0:3].any()


# ------------------------------------------------------------------------------------------------------------------ list edges

@functools.lru_cache(maxsize=None)
def half_floor_scene():
    """the camera looks straight down: the left half of the image sees a lit floor (every sample there faces the emitter, which hangs
    above the camera, outside its view), the right half sees nothing"""
    s = host.Scene()
    r = float(np.sqrt(0.5))
    s.set_camera((0.0, 1.5, 0.0), (-r, 0.0, 0.0, r), 60.0)
    s.add_quad((-4, 0, -4), (0, 0, 8), (4, 0, 0), s.add_diffuse((0.7, 0.6, 0.5)))
    s.add_quad((-2.5, 2.0, -0.5), (1, 0, 0), (0, 0, 1), s.add_emissive((20.0, 20.0, 20.0)))
    return s.compile()


def _blk(k, origin, dim, W, H, seed=900):
    b = abi.ImageBlock()
    b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:], b.sample_offset[:] = k, seed + 131 * k, origin, dim, (W, H), (0.5, 0.5)
    return b


EDGE_LISTS = {0: [((40, 0), (8, 8))], 1: [((40, 8), (8, 8)), ((3, 3), (1, 1))], 255: [((0, 0), (15, 17)), ((40, 0), (8, 8))], 256: [((0, 0), (16, 16))],
              257: [((0, 0), (16, 16)), ((40, 30), (4, 4)), ((20, 20), (1, 1))], 513: [((0, 0), (19, 27)), ((33, 0), (31, 64))]}


@pytest.mark.parametrize("count", sorted(EDGE_LISTS))
def test_lists_of_exactly_n_shadow_rays(rq, count):
    """one walk launch whose slots that want a shadow ray number exactly `count`: below, at and above one compaction tile and two"""
    cs = half_floor_scene()
    W = H = 64
    blocks = [_blk(k, o, dm, W, H) for k, (o, dm) in enumerate(EDGE_LISTS[count])]
    rq.upload_scene(cs)
    want, det = DL.render(cs, blocks, W, H, 0, gpu_trace(rq), gpu_occluded(rq), detail=True)
    assert int(det["wants"].sum()) == count and int(det["counts"].sum()) == count          # (nothing stands between the floor and the emitter)
    rq.upload_scene(cs)
    same_bits(rq.render_direct_lit(W, H, blocks=blocks), want, f"{count} shadow rays in the launch")


def test_the_list_over_three_walk_launches_and_two_runs(rq, monkeypatch):
    cs = half_floor_scene()
    W = H = 64
    three = [_blk(k, o, dm, W, H) for k, (o, dm) in enumerate([((0, 0), (19, 27)), ((33, 0), (31, 64)), ((0, 30), (16, 16))])]
    two = [_blk(0, (0, 0), (19, 27), W, H), _blk(1, (10, 10), (16, 16), W, H, seed=5)]          # overlapping: two runs
    rq.upload_scene(cs)
    wants = {}
    for key, blocks in (("three", three), ("two", two)):
        img, det = DL.render(cs, blocks, W, H, 0, gpu_trace(rq), gpu_occluded(rq), detail=True)
        wants[key] = (img, [int(det["wants"][a:b].sum()) for a, b in zip(np.cumsum([0] + [bl.dimension[0] * bl.dimension[1] for bl in blocks])[:-1],
                                                                              np.cumsum([bl.dimension[0] * bl.dimension[1] for bl in blocks]))])
    assert wants["three"][1] == [513, 0, 256] and wants["two"][1] == [513, 256] and wants["two"][0][..., 3].max() == 2
    rq.upload_scene(cs)
    same_bits(rq.render_direct_lit(W, H, blocks=three), wants["three"][0], "one launch")
    same_bits(rq.render_direct_lit(W, H, blocks=two), wants["two"][0], "two runs")
    monkeypatch.setenv("HJ_TRACE_CHUNK", "16384")                         # a block a launch: lists of 513, 0 and 256 entries
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        same_bits(r.render_direct_lit(W, H, blocks=three), wants["three"][0], "three walk launches")
        same_bits(r.render_direct_lit(W, H, blocks=two), wants["two"][0], "two launches, a run each")


# ------------------------------------------------------------------------------------------------------------------- occlusion

CAM_Y, SLAB_Y, LIGHT_Y = 0.8, 1.0, 2.0
LIGHT_X, LIGHT_Z = (-0.01, 0.01), (-0.5, 0.5)
SLAB_X, SLAB_Z = (0.0, 1.5), (-3.0, 3.0)


def slab_scene():
    """a floor seen from straight above, a narrow quad emitter high over the camera, and between them an opaque slab over the x > 0 half"""
    s = host.Scene()
    r = float(np.sqrt(0.5))
    s.set_camera((0.0, CAM_Y, 0.0), (-r, 0.0, 0.0, r), 60.0)
    s.add_quad((-4, 0, -4), (0, 0, 8), (8, 0, 0), s.add_diffuse((0.7, 0.6, 0.5)))
    s.add_quad((SLAB_X[0], SLAB_Y, SLAB_Z[0]), (0, 0, SLAB_Z[1] - SLAB_Z[0]), (SLAB_X[1] - SLAB_X[0], 0, 0), s.add_diffuse((0.3, 0.3, 0.3)))
    s.add_quad((LIGHT_X[0], LIGHT_Y, LIGHT_Z[0]), (LIGHT_X[1] - LIGHT_X[0], 0, 0), (0, 0, LIGHT_Z[1] - LIGHT_Z[0]), s.add_emissive((400.0, 300.0, 200.0)))
    return s.compile()


def shadow_classes(W, H):
    """float64, from the geometry: per pixel whether EVERY segment from its floor point to the emitter passes through the slab
    (covered), NONE does (open), for the pixel's centre and its four corners alike - a margin of one pixel at the shadow's edge"""
    half = np.tan(np.radians(30.0))
    covered, opened = np.ones((H, W), bool), np.ones((H, W), bool)
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    for dx, dy in ((0.5, 0.5), (0, 0), (1, 0), (0, 1), (1, 1), (-0.5, 0.5), (1.5, 0.5), (0.5, -0.5), (0.5, 1.5)):
        x = (px + dx - 0.5 * W) * half / (0.5 * W) * CAM_Y              # the floor point under the pixel: the camera looks along -y
        z = (py + dy - 0.5 * H) * half / (0.5 * W) * CAM_Y
        f = (SLAB_Y - 0.0) / (LIGHT_Y - 0.0)                            # where a segment floor -> emitter crosses the slab's plane
        xs = [x + f * (ex - x) for ex in LIGHT_X]
        zs = [z + f * (ez - z) for ez in LIGHT_Z]
        inside = lambda a, lohi: (a > lohi[0]) & (a < lohi[1])                                   # noqa: E731
        covered &= inside(xs[0], SLAB_X) & inside(xs[1], SLAB_X) & inside(zs[0], SLAB_Z) & inside(zs[1], SLAB_Z)
        opened &= (np.maximum(xs[0], xs[1]) < SLAB_X[0]) | (np.minimum(xs[0], xs[1]) > SLAB_X[1])
    return covered, opened


def test_a_slab_shadows_exactly_the_covered_part_of_the_floor(rq):
    cs = slab_scene()
    W = H = 64
    blocks = block_list(W, H, 32, passes(1))
    covered, opened = shadow_classes(W, H)
    left_out = 1.0 - (covered.sum() + opened.sum()) / (W * H)
    print(f"slab: {int(covered.sum())} pixels covered, {int(opened.sum())} open, {100 * left_out:.1f} % left out at the edge")
    assert covered.sum() > 1000 and opened.sum() > 1000 and not (covered & opened).any()
    rq.upload_scene(cs)
    want, det = DL.render(cs, blocks, W, H, 0, gpu_trace(rq), gpu_occluded(rq), detail=True)
    px = sample_pixels(blocks)
    ids = rq.trace_rays(det["camera"])[0]
    assert (ids >= 0).all() and (ids == ids[0]).all()                    # every pixel is a floor pixel
    assert left_out <= 0.10 and det["wants"].all()
    rq.upload_scene(cs)
    got = rq.render_direct_lit(W, H, blocks=blocks)
    same_bits(got, want, "the slab scene")
    assert not got[covered][:, 0:3].any()                                # L = Lp exactly: Lp is 0 without a lighting
    assert (got[opened][:, 0:3] > 0).all()
    cnt = np.zeros((H, W), bool)
    cnt[px[:, 0], px[:, 1]] = det["counts"]
    assert not cnt[covered].any() and cnt[opened].all()
    # with a volume: on the covered part the pixel is hj_render_probe_lit's, bit for bit
    look, kw = lighting("plain")
    lit = rq.render_probe_lit(kw["volume"], kw["origin"], kw["spacing"], W, H, blocks=blocks)
    both = rq.render_direct_lit(W, H, blocks=blocks, **kw)
    assert (both[covered].view(U) == lit[covered].view(U)).all() and (both[opened][:, 0:3] != lit[opened][:, 0:3]).any(1).all()


# -------------------------------------------------------------------------------------------------------- refusals, empty lists

def test_a_refused_call_writes_nothing_and_no_blocks_give_zeros(rq):
    cs = half_floor_scene()
    rq.upload_scene(cs)
    L = device.lib()
    W = H = 16
    image = np.full((H, W, 4), 7.0, F)
    blocks = (abi.ImageBlock * 1)(_blk(0, (0, 0), (16, 16), W, H))
    assert L.hj_render_direct_lit(rq._h, blocks, 1, W, H, 9, 0, None, image.ctypes.data) == abi.HJ_ERR_INVALID
    assert L.hj_render_direct_lit(rq._h, blocks, 1, W, H, 0, 2, None, image.ctypes.data) == abi.HJ_ERR_INVALID
    assert L.hj_render_direct_lit_frame(rq._h, W, H, 1, 0, 1, 0, 0, 0, None, image.ctypes.data) == abi.HJ_ERR_INVALID
    assert (image == 7.0).all()
    assert L.hj_render_direct_lit(rq._h, None, 0, W, H, 0, 0, None, image.ctypes.data) == abi.HJ_OK and not image.any()
    assert not rq.render_direct_lit(W, H, blocks=[]).any() and not rq.render_direct_lit(W, H, spp=3, passes=(2, 2)).any()
    assert rq.render_direct_lit(W, H, spp=1)[..., 0:3].any()
