"""Image textures on the MI355X: the lookup probe against its numpy restatement, textured frames bit for bit against the unchanged
oracle rendering the diffuse twin (every route of the renderer), the resident-tree upload, a bilinear white furnace, the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes
import texture_scenes as ts
from hijiki_amd import abi, device, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def opts(flags=0):
    o = device.default_opts()
    o.flags = flags
    return o


def frame(r, cs, W, H, spp, seed, flags=0, device_tree=False, textures=None):
    r.upload_scene(cs, device_tree=device_tree, textures=textures)
    r.create_framebuffer(W, H)
    st = r.render_frame(spp, seed, opts=opts(flags))
    return r.read(), st


def test_lookup_probe_is_bit_exact(gpu_renderer):
    rng = np.random.default_rng(11)
    s = host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=64)
    texs = []
    for w, h in ((1, 1), (1, 7), (7, 1), (13, 9), (2048, 3)):
        for filt in (abi.TEX_NEAREST, abi.TEX_BILINEAR):
            t = rng.uniform(-2, 2, (h, w, 4)).astype(np.float32)
            texs.append((s.add_texture(t, filt), t, filt))
    cs = s.compile()
    r = gpu_renderer
    r.upload_scene(cs)
    ints = np.arange(-3, 4, dtype=np.float32)
    edge = np.concatenate([ints, ints + np.float32(1e-9), ints - np.float32(1e-9), [1e6, -1e6, np.nan, np.inf, -np.inf, 0.5]])
    a, b = np.meshgrid(edge.astype(np.float32), edge.astype(np.float32))
    uv = np.concatenate([np.stack([a.ravel(), b.ravel()], 1), rng.uniform(-3, 3, (20000, 2))]).astype(np.float32)
    for idx, t, filt in texs:
        got = r.texture_lookup(idx, uv)
        want = ts.lookup(t, filt, uv)
        bad = (bits(got) != bits(want)).any(axis=1)
        assert not bad.any(), f"texture {t.shape[1]}x{t.shape[0]} filter {filt}: {int(bad.sum())} lookups differ, first uv {uv[bad][0]}"
    with pytest.raises(abi.HijikiError) as e:
        r.texture_lookup(len(texs), uv[:1])
    assert e.value.status == abi.HJ_ERR_INVALID


def test_upload_rejects_bad_texture_sets():
    tex, _, _ = ts.textured_cbox(extra=False)
    cs = tex.compile()
    with device.Renderer(0) as r:
        _rejects(r, cs)


def _rejects(r, cs):
    good = cs.texture_set

    def expect(status, t):
        with pytest.raises(abi.HijikiError) as e:
            r.upload_scene(cs, textures=t)
        assert e.value.status == status

    L = device.lib()
    assert L.hj_scene_upload(r._h, C.byref(cs.desc)) == abi.HJ_ERR_INVALID     # tag 5 without textures
    expect(abi.HJ_ERR_INVALID, abi.TextureSet())                               # index >= num_textures
    rec = (abi.Texture * 1)()
    for w, h, f, first in ((0, 4, 0, 0), (4, 0, 0, 0), (16, 8, 2, 0), (16, 8, 0, 1)):
        rec[0] = abi.Texture(w, h, f, first)
        expect(abi.HJ_ERR_INVALID, abi.TextureSet(rec, 1, good.texels, good.num_texels))
    expect(abi.HJ_ERR_UNSUPPORTED, abi.TextureSet(good.textures, 1, good.texels, (1 << 32) + 1))
    with pytest.raises(abi.HijikiError) as e:                                   # no scene after a failed upload
        r.texture_lookup(0, np.zeros((1, 2), np.float32))
    assert e.value.status == abi.HJ_ERR_STATE
    r.upload_scene(cs)
    assert r.texture_lookup(0, np.array([[0.5 / 16, 1 - 0.5 / 8]], np.float32)).shape == (1, 3)


@pytest.mark.parametrize("flags", [0, abi.RENDER_SPLIT_KERNELS, abi.RENDER_NO_LIGHT_GRID])
def test_textured_frame_matches_oracle_twin(gpu_renderer, oracle, flags):
    """Nearest lookups at texel centres give exactly the twin's diffuse colours: the frame is the oracle's frame of the twin."""
    tex, twin, _ = ts.textured_cbox(seed=3)
    a, b = tex.compile(), twin.compile()
    b.set_bvh(a.bvh)                                             # the same tree in both (the compiler votes them equal anyway)
    assert (a.bvh == b.bvh).all()
    W, H, spp, seed = 96, 64, 4, 7
    got, st = frame(gpu_renderer, a, W, H, spp, seed, flags)
    want, ctr, _ = oracle.render_blocks(b, host.make_blocks(W, H, spp, seed), W, H)
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} pixels differ from the oracle's twin"
    assert st["closest_rays"] == ctr["closest_calls"] and st["shadow_rays"] == ctr["shadow_calls"]
    want_tex, ctr_tex, _ = oracle.render_blocks(a, host.make_blocks(W, H, spp, seed), W, H)     # the oracle's own textured frame
    assert (bits(want_tex) == bits(want)).all() and ctr_tex == ctr
    twin_img, st2 = frame(gpu_renderer, b, W, H, spp, seed, flags)
    assert (bits(twin_img) == bits(got)).all()
    assert st["shadow_rays_proven_free"] == st2["shadow_rays_proven_free"]
    if flags != abi.RENDER_NO_LIGHT_GRID:
        assert st["shadow_rays_proven_free"] > 0
    if flags == 0:                                               # hj_debug_samples: the intermediate image of one block
        blk = host.make_blocks(W, H, 1, seed)[0]
        gpu_renderer.upload_scene(a)
        s1 = gpu_renderer.samples(blk)
        gpu_renderer.upload_scene(b)
        assert (bits(s1) == bits(gpu_renderer.samples(blk))).all()


def test_device_vote_treats_textured_as_diffuse(gpu_renderer):
    tex, twin, _ = ts.textured_cbox(seed=4)
    a, b = tex.compile(), twin.compile()
    assert (gpu_renderer.tune_bvh_device(a, 20000) == gpu_renderer.tune_bvh_device(b, 20000)).all()


def test_resident_tree_route(gpu_renderer):
    """build_bvh(keep_on_device=True) + a textured upload with bvh == NULL: the bits of the same tree through the host.  A rejected
    texture set leaves the tree on the device for the retry."""
    tex, _, _ = ts.textured_cbox(seed=9)
    r = gpu_renderer
    shapes = tex.compile(with_tree=False)
    nodes = r.build_bvh(shapes)
    W, H, spp, seed = 80, 48, 3, 2
    full = tex.compile()
    full.set_bvh(nodes)
    want, st_w = frame(r, full, W, H, spp, seed)
    assert r.build_bvh(shapes, keep_on_device=True) == len(nodes)
    with pytest.raises(abi.HijikiError) as e:
        r.upload_scene(shapes, device_tree=True, textures=abi.TextureSet())
    assert e.value.status == abi.HJ_ERR_INVALID
    assert (r.read_device_bvh() == nodes).all()
    got, st = frame(r, shapes, W, H, spp, seed, device_tree=True)
    assert (bits(got) == bits(want)).all()
    assert st["closest_rays"] == st_w["closest_rays"] and st["shadow_rays"] == st_w["shadow_rays"]


def test_bilinear_white_furnace(gpu_renderer):
    """tests/scenes.py's furnace with the sphere's albedo from a constant 3 x 5 bilinear texture: rho * L on the sphere."""
    s = host.Scene()
    s.set_camera((0.0, 0.0, 2.5), (0.0, 0.0, 0.0, 1.0), 40.0)
    lamp = s.add_emissive((scenes.FURNACE_L,) * 3)
    a = 3.0
    s.add_quad((-a, -a, -a), (0, 0, 2 * a), (2 * a, 0, 0), lamp)
    s.add_quad((-a, a, -a), (2 * a, 0, 0), (0, 0, 2 * a), lamp)
    s.add_quad((-a, -a, -a), (2 * a, 0, 0), (0, 2 * a, 0), lamp)
    s.add_quad((-a, -a, a), (0, 2 * a, 0), (2 * a, 0, 0), lamp)
    s.add_quad((-a, -a, -a), (0, 2 * a, 0), (0, 0, 2 * a), lamp)
    s.add_quad((a, -a, -a), (0, 0, 2 * a), (0, 2 * a, 0), lamp)
    t = s.add_texture(np.full((5, 3, 3), scenes.FURNACE_RHO, np.float32), abi.TEX_BILINEAR)
    s.add_sphere((0.0, 0.0, 0.0), 0.6, s.add_diffuse_textured(t))
    W = H = 128
    r = gpu_renderer
    r.upload_scene(s.compile())
    r.create_framebuffer(W, H)
    r.render_frame(1024, 5)
    acc = r.read().astype(np.float64)
    img = acc[..., :3] / acc[..., 3:4]
    disc, wall = scenes.furnace_masks(W, H)
    assert np.abs(img[wall] - scenes.FURNACE_L).max() < 1e-5
    want = scenes.FURNACE_RHO * scenes.FURNACE_L
    assert abs(img[disc].mean() - want) < 5e-4 * want
    assert np.abs(img[disc] - want).max() < 0.2 * want


def test_cli_textures_renders_like_the_library(tmp_path):
    pfm = np.random.default_rng(5).uniform(0, 1, (4, 5, 3)).astype(np.float32)
    obj = ts.write_obj_files(tmp_path, pfm)
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    out = str(tmp_path / "o.pfm")
    r = subprocess.run([exe, "--textures", "--use-bvh", "-w", "96", "-h", "64", "-s", "3", "--seed", "6", "-o", out, obj],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    head = b"PF\n96 64\n-1.0\n"
    got = np.frombuffer(raw, np.float32, offset=len(head)).reshape(64, 96, 3)[::-1]
    cs = host.Scene.from_obj(obj, textures=True).compile()
    with device.Renderer(0) as rr:
        rr.upload_scene(cs)
        rr.create_framebuffer(96, 64)
        rr.render_frame(3, 6)
        want = rr.resolve()
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # without the flag the same files render as today: map_Kd ignored
    out2 = str(tmp_path / "o2.pfm")
    r = subprocess.run([exe, "--use-bvh", "-w", "96", "-h", "64", "-s", "3", "--seed", "6", "-o", out2, obj],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = np.frombuffer(open(out2, "rb").read(), np.float32, offset=len(head)).reshape(64, 96, 3)[::-1]
    with device.Renderer(0) as rr:
        rr.upload_scene(host.Scene.from_obj(obj).compile())
        rr.create_framebuffer(96, 64)
        rr.render_frame(3, 6)
        want2 = rr.resolve()
    assert (plain.view(np.uint32) == want2.view(np.uint32)).all()
    assert not (plain.view(np.uint32) == got.view(np.uint32)).all()


# ------------------------------------------------------------------ frames whose colour varies across surfaces, against the oracle

ROUTES = ("default", "split-kernels", "no-light-grid", "linear-scan", "device-re-layout", "device-built-tree", "resident-tree")


def render_route(r, cs, route, W, H, spp, seed, monkeypatch):
    """cs on one route of the renderer -> (frame, stats, the oracle's RenderOpts for the same frame)."""
    o = opts({"split-kernels": abi.RENDER_SPLIT_KERNELS, "no-light-grid": abi.RENDER_NO_LIGHT_GRID}.get(route, 0))
    if route == "linear-scan":
        o.use_bvh = 0
    if route == "device-re-layout":
        monkeypatch.setenv("HJ_UPLOAD_DEVICE", "1")
    else:
        monkeypatch.delenv("HJ_UPLOAD_DEVICE", raising=False)
    on_device = False
    if route == "device-built-tree":
        cs.set_bvh(r.build_bvh(cs))
    elif route == "resident-tree":                    # hj_scene_upload_textured takes the tree over; the oracle walks its copy
        r.build_bvh(cs, keep_on_device=True)
        cs.set_bvh(r.read_device_bvh())
        on_device = True
    r.upload_scene(cs, device_tree=on_device)
    r.create_framebuffer(W, H)
    st = r.render_frame(spp, seed, opts=o)
    return r.read(), st, o


def assert_oracle_frame(oracle, cs, got, st, o, W, H, spp, seed, what, blocks=None):
    blocks = host.make_blocks(W, H, spp, seed) if blocks is None else blocks
    want, ctr, _ = oracle.render_blocks(cs, blocks, W, H, opts=o)
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ from the oracle"
    assert (st["closest_rays"], st["shadow_rays"], st["hits"], st["paths"]) == \
        (ctr["closest_calls"], ctr["shadow_calls"], ctr["hits"], ctr["paths"]), what


@pytest.mark.parametrize("route", ROUTES)
def test_textured_scenes_match_the_oracle(gpu_renderer, oracle, monkeypatch, route):
    """Textured random scenes (tests/texture_scenes.py: both filters, a 1024 x 1024 texture in front of the small ones, uv in
    [-3, 3] on integers and texel edges, textured quads and spheres) and the mixed-bin mesh (checkerboard, textured and plain
    triangles side by side) bit for bit against the oracle, counters included, on every route of the renderer."""
    linear = route == "linear-scan"
    W, H, spp = (64, 40, 2) if linear else (96, 64, 3)
    for name, cs, seed in (("random textured 1", ts.random_textured_scene(1), 5), ("random textured 2", ts.random_textured_scene(2), 6),
                           ("mixed bin, bilinear", ts.mixed_bin_scene(0), 7),
                           ("mixed bin, nearest", ts.mixed_bin_scene(1, filt=abi.TEX_NEAREST), 8)):
        got, st, o = render_route(gpu_renderer, cs, route, W, H, spp, seed, monkeypatch)
        assert_oracle_frame(oracle, cs, got, st, o, W, H, spp, seed, f"{name}, {route}")


def test_textured_tile_sharding(gpu_renderer, oracle):
    """Each rank's share of a textured frame is the oracle's render of that rank's blocks, the shares sum to the 1-GPU frame
    (to rounding on the block aprons, as tests/test_gpu_parity.py test_tile_sharding_sums_to_the_full_frame), and that frame
    is the oracle's."""
    cs = ts.random_textured_scene(3)
    W, H, spp, seed = 288, 160, 3, 4
    r = gpu_renderer
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    st_full = r.render_frame(spp, seed)
    full = r.read().copy()
    assert_oracle_frame(oracle, cs, full, st_full, device.default_opts(), W, H, spp, seed, "full frame")
    L = host.lib()
    blocks = host.make_blocks(W, H, spp, seed)
    per = host.blocks_per_pass(W, H)
    world = 3
    parts, paths = [], 0
    for rank in range(world):
        r.clear()
        st = r.render_frame(spp, seed, rank=rank, world=world)
        paths += st["paths"]
        part = r.read().copy()
        mine = [b for k, b in enumerate(blocks) if L.hj_block_owner(W, H, k // per, k % per, world) == rank]
        assert_oracle_frame(oracle, cs, part, st, device.default_opts(), W, H, spp, seed, f"rank {rank} of {world}",
                            blocks=(abi.ImageBlock * len(mine))(*mine))
        parts.append(part.astype(np.float64))
    assert paths == st_full["paths"]
    np.testing.assert_allclose(np.sum(parts, axis=0), full, rtol=3e-6, atol=1e-6)


def test_non_finite_texels(gpu_renderer, oracle):
    """A texture holding NaN and +-Inf texels: the paths that meet them carry NaN / Inf, the reconstruction skips NaN taps -
    the frame is still the oracle's, bit for bit, with both filters."""
    for filt in (abi.TEX_NEAREST, abi.TEX_BILINEAR):
        rng = np.random.default_rng(17)
        t = ts.random_texels(rng, 6, 5)
        t[1, 1, 0], t[2, 3, 1], t[4, 0, 2], t[5, 4, :3] = np.nan, np.inf, -np.inf, np.nan
        s = host.Scene()
        s.set_camera_cbox()
        m = s.add_diffuse_textured(s.add_texture(t, filt))
        s.add_quad((-1.2, 0, 1.2), (2.4, 0, 0), (0, 0, -2.4), m)
        s.add_quad((-1.2, 0, -1.2), (2.4, 0, 0), (0, 2.0, 0), s.add_diffuse((0.5, 0.5, 0.5)))
        s.add_quad((-0.4, 1.99, -0.4), (0.8, 0, 0), (0, 0, 0.8), s.add_emissive((12.0, 12.0, 12.0)))
        s.add_sphere((0.0, 0.5, 0.0), 0.4, m)
        cs = s.compile()
        W, H, spp, seed = 96, 64, 2, 3
        r = gpu_renderer
        r.upload_scene(cs)
        r.create_framebuffer(W, H)
        st = r.render_frame(spp, seed)
        got = r.read()
        assert_oracle_frame(oracle, cs, got, st, device.default_opts(), W, H, spp, seed, f"non-finite texels, filter {filt}")
        assert not np.isfinite(got).all()              # (the texels did reach the frame)
