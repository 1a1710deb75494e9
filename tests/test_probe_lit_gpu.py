"""hj_render_probe_lit and hj_render_probe_lit_frame on the GPU against probe_lit_ref - the contract restated in numpy over
hj_trace_rays' own records - bit for bit on every word of every pixel: the three look-ups at max_follow 0, 2 and 8 from host and from
device arrays; an all-zero volume against hj_render_aovs_followed's emission words; the per-sample composition over the PUBLIC placed
look-up at points rebuilt with hj_trace_rays and hj_follow_specular; overlapping and out-of-order block lists; several walk launches;
the environment behind a miss and behind glass; the cap on a mirror; the frame form.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import probe_lit_ref as PL
import probe_place_ref as PP
import probe_ref as PR
import probe_vis_ref as PV
import path_query_ref as P
from hijiki_amd import abi, device, host
from test_follow_gpu import block_list, gpu_trace, same_bits

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
RES = 4
SIZES = {"48x40": (48, 40), "33x17": (33, 17)}
GRIDS = {"2x2x2": (2, 2, 2), "5x4x3": (5, 4, 3)}


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    assert all(hasattr(device.lib(), n) for n in ("hj_render_probe_lit", "hj_render_probe_lit_frame"))


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as r:
        yield r


@functools.lru_cache(maxsize=None)
def lit_scene():
    """the box with its mirror and glass spheres, and a checkerboard quad in front of its back wall"""
    s = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES)
    s.add_quad((-0.6, 0.2, 0.4), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0), s.add_diffuse_cboard((0.9, 0.8, 0.2), 0.13, (0.1, 0.2, 0.8), 0.21))
    return s.compile()


@functools.lru_cache(maxsize=None)
def volume(grid):
    """a fabricated volume on a grid that covers the middle of the scene's box, so that hit points on the walls lie outside it:
    (desc, vis, volume (nz, ny, nx, 28), atlas (nz, ny, nx, 6, 6, 2) of finite moments, placement (nz, ny, nx, 4) with offsets and
    about a quarter of the probes asleep)"""
    count = GRIDS[grid]
    d = PR.grid_in_domain(lit_scene(), count)
    nx, ny, nz = count
    n = nx * ny * nz
    vol = PR.fabricated_volume(count, 11)
    atlas = PV.hashed_atlas(n, RES, 3)
    atlas = np.where(np.isfinite(atlas), atlas, F(1.5)).astype(F).reshape(nz, ny, nx, RES + 2, RES + 2, 2)
    rng = np.random.default_rng([5, n])
    place = PP.zeros(n)
    place[:, 0:3] = (rng.uniform(-0.3, 0.3, (n, 3)) * d["spacing"]).astype(F)
    asleep = (rng.uniform(size=n) < 0.25).astype(U)
    asleep[0], asleep[n // 2] = 0, 1                                     # (whatever the draw: one awake, one asleep)
    place = PP.with_state(place, asleep).reshape(nz, ny, nx, 4)
    assert 0 < (PP.state(place) != 0).sum() < n
    for a in (vol, atlas, place):
        a.setflags(write=False)
    return d, PV.vis(res=RES, normal_bias=0.02), vol, atlas, place


def ragged(size, spp):
    W, H = SIZES[size]
    return block_list(W, H, 16, [(11 + 7 * k, (0.5 if k == 0 else 0.125 + 0.25 * k, 0.5 if k == 0 else 0.875 - 0.25 * k)) for k in range(spp)])


def look(grid, kind):
    d, v, vol, atlas, place = volume(grid)
    n = vol.size // 28
    if kind == "plain":
        return PL.lookup(d, vol)
    if kind == "visible":
        return PL.lookup(d, vol, v, atlas.reshape(n, RES + 2, RES + 2, 2))
    return PL.lookup(d, vol, v, atlas.reshape(n, RES + 2, RES + 2, 2), place.reshape(n, 4))


def call(r, grid, kind, W, H, on_gpu=False, **kw):
    """Renderer.render_probe_lit with the grid's volume and the look-up `kind` selects"""
    d, v, vol, atlas, place = volume(grid)
    arrays = dict(volume=vol, atlas=None if kind == "plain" else atlas, placement=place if kind == "placed" else None)
    if on_gpu:
        import torch
        arrays = {k: None if a is None else torch.from_numpy(np.array(a)).to(f"cuda:{r.device}") for k, a in arrays.items()}
    out = r.render_probe_lit(arrays["volume"], d["origin"], d["spacing"], W, H, atlas=arrays["atlas"], placement=arrays["placement"], normal_bias=0.02, **kw)
    if on_gpu:
        assert out.is_cuda
        return out.cpu().numpy()
    return out


_WANT = {}


def expected(r, cs, key, blocks, W, H, follow, grid, kind, env=None):
    """the restatement over hj_trace_rays' own records, once per case on a renderer without a switch, never written to"""
    k = (key, follow, grid, kind)
    if k not in _WANT:
        r.upload_scene(cs)
        img, ch, L = PL.render(cs, blocks, W, H, follow, gpu_trace(r), look(grid, kind), env, detail=True)
        img.setflags(write=False)
        _WANT[k] = (img, ch, L)
    return _WANT[k]


def sample_pixels(blocks):
    """(y, x) of every sample of blocks that lie inside the image, in the samples' order"""
    return np.concatenate([np.stack(np.mgrid[b.origin[1]:b.origin[1] + b.dimension[1], b.origin[0]:b.origin[0] + b.dimension[0]], -1).reshape(-1, 2) for b in blocks])


# ------------------------------------------------------------------------------------------------- 1. against the restatement

@pytest.mark.parametrize("kind", ["plain", "visible", "placed"])
@pytest.mark.parametrize("size,spp,grid", [("48x40", 3, "5x4x3"), ("33x17", 1, "2x2x2")])
def test_every_word_equals_the_restatement(rq, kind, size, spp, grid):
    cs = lit_scene()
    W, H = SIZES[size]
    blocks = ragged(size, spp)
    d = volume(grid)[0]
    for follow in (0, 2, 8):
        want, ch, _ = expected(rq, cs, ("ragged", size, spp), blocks, W, H, follow, grid, kind)
        if follow == 2 and size == "48x40":
            outside = ((ch["points"][:, 0:3] < d["origin"]) | (ch["points"][:, 0:3] > d["origin"] + d["spacing"] * (np.array(d["count"]) - 1))).any(1)
            kinds = np.bincount(ch["kind"], minlength=3)
            print(f"{size} x {spp} spp: kinds {kinds.tolist()}, chain lengths {np.bincount(ch['length']).tolist()}, points outside the grid {int(outside.sum())}")
            assert outside.sum() > 100 and (~outside).sum() > 100 and kinds[PL.DIFFUSE] > 1000 and (ch["length"] > 0).sum() > 64
            assert len(np.unique(ch["albedo"][ch["kind"] == PL.DIFFUSE], axis=0)) >= 5                 # the walls, both checkerboard colours
        rq.upload_scene(cs)
        same_bits(call(rq, grid, kind, W, H, blocks=blocks, follow=follow), want, f"{kind} / {size} / {grid} / max_follow {follow} / host arrays")
        same_bits(call(rq, grid, kind, W, H, on_gpu=True, blocks=blocks, follow=follow), want, f"{kind} / {size} / {grid} / max_follow {follow} / device arrays")
    # the cap decides: at max_follow 0 every sample on a sphere is cut there and gives 0
    zero, two = expected(rq, cs, ("ragged", size, spp), blocks, W, H, 0, grid, kind)[1], expected(rq, cs, ("ragged", size, spp), blocks, W, H, 2, grid, kind)[1]
    assert (zero["kind"] == PL.SPECULAR).sum() > (two["kind"] == PL.SPECULAR).sum()


# ------------------------------------------------------------------------------------------------------ 2. zero-volume identity

@pytest.mark.parametrize("kind", ["plain", "placed"])
def test_an_all_zero_volume_leaves_the_emission(rq, kind):
    cs = lit_scene()
    W, H = SIZES["48x40"]
    blocks = ragged("48x40", 3) + ragged("48x40", 1)[:2]
    d, v, vol, atlas, place = volume("5x4x3")
    rq.upload_scene(cs)
    for follow in (0, 2):
        aov = rq.render_aovs(W, H, blocks=blocks, follow=follow)
        got = rq.render_probe_lit(np.zeros_like(vol), d["origin"], d["spacing"], W, H, atlas=None if kind == "plain" else atlas,
                                  placement=place if kind == "placed" else None, blocks=blocks, follow=follow)
        same_bits(got[..., 0:3], aov[..., 8:11], f"{kind} / max_follow {follow}: the emission words")
        cover = np.zeros((H, W), F)
        for b in blocks:
            cover[b.origin[1]:b.origin[1] + b.dimension[1], b.origin[0]:b.origin[0] + b.dimension[0]] += 1
        same_bits(got[..., 3], cover, "the sample count")
        same_bits(got[..., 3], aov[..., 3], "... which is hj_render_aovs_followed's")
        assert got[..., 0:3].any() and cover.max() == 4 and cover.min() == 3


# ------------------------------------------------------------------------------------------------- 3. per-sample composition

def test_one_sample_is_the_public_look_up_composed(rq):
    """1 spp, disjoint blocks: every pixel holds one sample, whose chain is rebuilt here with hj_trace_rays and hj_follow_specular
    and whose E comes from a separate hj_sample_probes_visible_placed call - the staged look-up is the public one"""
    cs = lit_scene()
    W, H = SIZES["48x40"]
    blocks = ragged("48x40", 1)
    d, v, vol, atlas, place = volume("5x4x3")
    rq.upload_scene(cs)
    rays = PL.camera_rays(cs, blocks)
    n = len(rays)
    ids, t, u, vv, surf = rq.trace_rays(rays, surface=True)
    hits = np.stack([ids.view(F), t, u, vv], 1)
    live = np.arange(n)
    cur, cur_hits = rays, hits
    for _ in range(2):
        nxt = rq.follow_specular(cur, cur_hits)
        go = nxt[:, 6] != np.inf
        if not go.any():
            break
        live, cur = live[go], nxt[go]
        i2, t2, u2, v2, s2 = rq.trace_rays(cur, surface=True)
        cur_hits = np.stack([i2.view(F), t2, u2, v2], 1)
        hits[live], surf[live] = cur_hits, s2
    mat = rq.eval_materials(hits, surf)
    word = mat.view(U)[:, 3]
    tag = word >> abi.MATERIAL_TAG_SHIFT
    diffuse = (word != abi.MATERIAL_MISS) & (tag != abi.MAT_MIRROR) & (tag != abi.MAT_DIELECTRIC)
    pts = np.zeros((n, 8), F)
    pts[:, 0:6] = surf[:, 0:6]
    E = rq.sample_probes_visible(vol, atlas, d["origin"], d["spacing"], pts[diffuse], normal_bias=0.02, placement=place)[:, 0:3]
    L = np.zeros((n, 3), F)
    L[diffuse] = mat[diffuse, 4:7] + (mat[diffuse, 0:3] * E) * PL.INV_PI
    L[~diffuse & (word != abi.MATERIAL_MISS)] = mat[~diffuse & (word != abi.MATERIAL_MISS), 4:7]
    want = PL.accumulate(W, H, blocks, L)
    assert diffuse.sum() > 1500 and (want[..., 3] == 1).all()
    same_bits(call(rq, "5x4x3", "placed", W, H, blocks=blocks, follow=2), want, "Le + (albedo * E) * (1 / pi) over the public look-up")


# ------------------------------------------------------------------------------------------------------------ 4. block lists

def shuffled_overlapping():
    """48 x 40: two passes of 16-pixel blocks in a shuffled order with three blocks repeated, one block that hangs over the right edge
    and one whose origin lies outside the image"""
    blocks = ragged("48x40", 2)
    order = np.random.default_rng(4).permutation(len(blocks))
    out = [blocks[i] for i in order] + [blocks[0], blocks[7], blocks[0]]
    for k, (ox, oy, w, h) in enumerate([(40, 30, 16, 16), (48, 0, 8, 8)]):
        b = abi.ImageBlock()
        b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:], b.sample_offset[:] = 100 + k, 77 + k, (ox, oy), (w, h), (48, 40), (0.25, 0.75)
        out.insert(5 + 9 * k, b)
    return out


def test_overlapping_and_out_of_order_block_lists(rq):
    cs = lit_scene()
    W, H = SIZES["48x40"]
    blocks = shuffled_overlapping()
    want, _, _ = expected(rq, cs, "shuffled", blocks, W, H, 2, "5x4x3", "visible")
    assert want[..., 3].max() >= 4                                      # at least four samples on one pixel: at least three cuts
    rq.upload_scene(cs)
    same_bits(call(rq, "5x4x3", "visible", W, H, blocks=blocks, follow=2), want, "shuffled, overlapping blocks")
    assert not call(rq, "5x4x3", "visible", W, H, blocks=[], follow=2).any()


# ---------------------------------------------------------------------------------------------------------- 5. walk launches

def test_several_walk_launches_give_the_same_bits(rq, monkeypatch):
    """HJ_TRACE_CHUNK = 4 blocks: the 23 blocks of the shuffled list take launches of 4, 4, 4, 4, 4 and 3 blocks, runs cut across
    them; = 1 block: 23 launches.  A context reads the switch when it is created (the edge tests' way)."""
    cs = lit_scene()
    W, H = SIZES["48x40"]
    blocks = shuffled_overlapping()
    assert len(blocks) == 23
    want, _, _ = expected(rq, cs, "shuffled", blocks, W, H, 2, "5x4x3", "visible")
    for chunk in (4 * 16384, 16384):
        monkeypatch.setenv("HJ_TRACE_CHUNK", str(chunk))
        with device.Renderer(0) as r:
            r.upload_scene(cs)
            same_bits(call(r, "5x4x3", "visible", W, H, blocks=blocks, follow=2), want, f"HJ_TRACE_CHUNK {chunk}")
            same_bits(call(r, "5x4x3", "visible", W, H, on_gpu=True, blocks=blocks, follow=2), want, f"HJ_TRACE_CHUNK {chunk}, device arrays")


# ------------------------------------------------------------------------------------------------------------ 6. environment

def test_a_miss_and_a_chain_that_leaves_the_glass_carry_the_environment(rq):
    cs = P.scene("env")                                                 # open: floor, a wall, a mirror sphere, a tinted glass sphere, a sky
    W, H = SIZES["48x40"]
    blocks = ragged("48x40", 1)
    rq.upload_scene(cs)
    want, ch, L = PL.render(cs, blocks, W, H, 8, gpu_trace(rq), look("5x4x3", "plain"), env=rq.env_lookup, detail=True)
    miss = ch["kind"] == PL.MISS
    tags = cs.materials >> abi.MATERIAL_TAG_SHIFT
    first = rq.trace_rays(PL.camera_rays(cs, blocks))[0]
    through_glass = miss & ch["left"] & (first >= 0) & (tags[np.maximum(first, 0)] == abi.MAT_DIELECTRIC)
    print(f"environment: {int((miss & ~ch['left']).sum())} camera misses, {int(ch['left'].sum())} chains left a specular surface, {int(through_glass.sum())} through the glass")
    assert (miss & ~ch["left"]).sum() > 50 and through_glass.sum() > 10 and L[miss].any(1).sum() > 50
    same_bits(L[miss], rq.env_lookup(ch["direction"][miss]), "the texel of the last segment's direction")
    rq.upload_scene(cs)
    got = call(rq, "5x4x3", "plain", W, H, blocks=blocks, follow=8)
    same_bits(got, want, "under an environment")
    # 1 spp, disjoint blocks: a pixel IS its sample
    px = sample_pixels(blocks)
    same_bits(got[px[miss, 0], px[miss, 1], 0:3], rq.env_lookup(ch["direction"][miss]), "the pixels of the misses")


# -------------------------------------------------------------------------------------------------------- 7. cap on a mirror

def test_samples_cut_on_the_second_mirror_count_and_add_nothing(rq):
    """two mirrors in a corner in front of a lit diffuse wall: at max_follow 1 a chain camera -> mirror A -> mirror B is cut on B"""
    s = host.Scene()
    s.set_camera((0, 0, 0), (0, 0, 0, 1), 40.0)
    grey, mirror = s.add_diffuse((0.5, 0.6, 0.7)), s.add_mirror()
    s.add_quad((-3, -3, -4), (6, 0, 0), (0, 6, 0), mirror)
    s.add_quad((-4, -4, 7), (8, 0, -8), (0, 8, 0), mirror)
    s.add_quad((-8, -10, -10), (0, 20, 0), (0, 0, 20), grey)
    cs = s.compile()
    W, H = SIZES["33x17"]
    blocks = ragged("33x17", 1)
    d = PR.desc((-9, -4, -4), (2.5, 4.0, 4.0), (2, 2, 2))
    vol = np.zeros((2, 2, 2, 28), F)
    vol[..., 0:3], vol[..., 27] = (1.0, 2.0, 3.0), 1.0
    rq.upload_scene(cs)
    px = sample_pixels(blocks)
    cut = None
    for follow in (1, 2):
        want, ch, L = PL.render(cs, blocks, W, H, follow, gpu_trace(rq), PL.lookup(d, vol), detail=True)
        rq.upload_scene(cs)
        got = rq.render_probe_lit(vol, d["origin"], d["spacing"], W, H, blocks=blocks, follow=follow)
        same_bits(got, want, f"two mirrors, max_follow {follow}")
        assert (got[..., 3] == 1).all()                                 # every sample is counted, the cut ones too
        if follow == 1:
            cut = (ch["kind"] == PL.SPECULAR) & (ch["length"] == 1)
            assert cut.sum() > 100 and not got[px[cut, 0], px[cut, 1], 0:3].any()     # cut on B: black
        else:
            seen = cut & (ch["kind"] == PL.DIFFUSE) & (ch["length"] == 2)
            assert seen.sum() > 100 and got[px[seen, 0], px[seen, 1], 0:3].all()      # one more continuation: B shows the lit wall


# ----------------------------------------------------------------------------------------------------------- 8. the frame form

def test_the_frame_form_is_the_block_form_over_the_frames_blocks(rq):
    cs = lit_scene()
    rq.upload_scene(cs)
    for (W, H), passes in (((130, 60), (0, 2)), ((48, 40), (1, 3))):
        blocks = list(host.make_blocks(W, H, 3, 21, passes[0], passes[1]))
        frame = call(rq, "5x4x3", "placed", W, H, spp=3, master_seed=21, passes=passes, follow=2)
        same_bits(frame, call(rq, "5x4x3", "placed", W, H, blocks=blocks, follow=2), f"{W} x {H}, passes {passes}")
        assert (frame[..., 3] == passes[1] - passes[0]).all()
    assert not call(rq, "5x4x3", "placed", 48, 40, spp=3, master_seed=21, passes=(2, 2), follow=2).any()
    same_bits(call(rq, "5x4x3", "placed", 48, 40, on_gpu=True, spp=2, master_seed=21, follow=8), call(rq, "5x4x3", "placed", 48, 40, spp=2, master_seed=21, follow=8),
              "device arrays")
