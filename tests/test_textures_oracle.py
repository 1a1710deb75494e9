"""Image textures in the C oracle (no GPU): its lookup bit for bit against the numpy restatement of DESIGN.md "Image textures"
(tests/texture_scenes.py lookup, the same definition the kernels' probe is pinned to), the texel-centre cbox rendered as its
diffuse twin, textured frames against the float64 restatement (tests/golden/glsl_f64.py), and the texture sets it refuses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import glsl_f64 as G  # noqa: E402
import texture_scenes as ts  # noqa: E402
from hijiki_amd import abi, host  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def edge_uv(rng):
    """The grid of test_textures_gpu.py test_lookup_probe_is_bit_exact: integers, one ulp-ish either side, huge, non-finite."""
    ints = np.arange(-3, 4, dtype=np.float32)
    edge = np.concatenate([ints, ints + np.float32(1e-9), ints - np.float32(1e-9), [1e6, -1e6, np.nan, np.inf, -np.inf, 0.5]])
    a, b = np.meshgrid(edge.astype(np.float32), edge.astype(np.float32))
    return np.concatenate([np.stack([a.ravel(), b.ravel()], 1), rng.uniform(-3, 3, (20000, 2))]).astype(np.float32)


def test_oracle_lookup_is_bit_exact(oracle):
    """hjo_texture_lookup == ts.lookup on the probe test's shapes and grid, plus texel edges k / W, k / H of each texture and
    texels that are NaN or infinite."""
    rng = np.random.default_rng(11)
    s = host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=64)
    texs = []
    for w, h in ((1, 1), (1, 7), (7, 1), (13, 9), (2048, 3)):
        for filt in (abi.TEX_NEAREST, abi.TEX_BILINEAR):
            t = rng.uniform(-2, 2, (h, w, 4)).astype(np.float32)
            texs.append((s.add_texture(t, filt), t, filt))
    t = rng.uniform(0, 1, (5, 6, 4)).astype(np.float32)
    t[1, 2, 0], t[3, 4, 1], t[0, 5, 2] = np.nan, np.inf, -np.inf
    for filt in (abi.TEX_NEAREST, abi.TEX_BILINEAR):
        texs.append((s.add_texture(t, filt), t, filt))
    cs = s.compile()
    tset = cs.texture_set
    base = edge_uv(rng)
    for idx, t, filt in texs:
        h, w = t.shape[:2]
        k = np.arange(-2 * max(w, h), 2 * max(w, h) + 1, dtype=np.float32)
        on = np.stack(np.meshgrid(k / np.float32(w), k / np.float32(h)), -1).reshape(-1, 2)[:50000]
        uv = np.concatenate([base, on]).astype(np.float32)
        got = oracle.texture_lookup(tset, idx, uv)
        want = ts.lookup(t, filt, uv)
        bad = (bits(got) != bits(want)).any(axis=1)
        assert not bad.any(), f"texture {w}x{h} filter {filt}: {int(bad.sum())} lookups differ, first uv {uv[bad][0]}"
    with pytest.raises(abi.HijikiError) as e:
        oracle.texture_lookup(tset, len(texs), base[:1])
    assert e.value.status == abi.HJ_ERR_INVALID


def test_oracle_renders_texel_centre_cbox_as_its_twin(oracle):
    """Nearest lookups at texel centres are the twin's diffuse colours: same frame, same counters."""
    tex, twin, _ = ts.textured_cbox(seed=3)
    a, b = tex.compile(), twin.compile()
    b.set_bvh(a.bvh)
    W, H, spp, seed = 96, 64, 4, 7
    blocks = host.make_blocks(W, H, spp, seed)
    got, c1, _ = oracle.render_blocks(a, blocks, W, H)
    want, c2, _ = oracle.render_blocks(b, blocks, W, H)
    assert (bits(got) == bits(want)).all() and c1 == c2
    s1, _ = oracle.integrate_block(a, blocks[0])
    s2, _ = oracle.integrate_block(b, blocks[0])
    assert (bits(s1) == bits(s2)).all()


def _close(a32, a64, frac):
    close = (np.abs(a64 - a32) <= 1e-4 * np.maximum(1.0, np.abs(a32))).all(-1)
    assert close.mean() > frac, close.mean()
    np.testing.assert_allclose(a64[..., 3], a32[..., 3], rtol=3e-4)
    s32, s64 = a32[..., :3].sum(), a64[..., :3].sum()
    assert abs(s64 - s32) < 0.03 * abs(s32)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_textured_random_scenes_oracle_vs_float64(oracle, seed):
    """random_textured_scene (both filters in every scene, a 1024 x 1024 texture first, textured quads, spheres and triangles)
    at test_glsl_f64.py's tolerances, and the colour does change across the frame."""
    cs = ts.random_textured_scene(seed)
    W, H = 80, 48
    blocks = host.make_blocks(W, H, 2, seed)
    a32, ctr, _ = oracle.render_blocks(cs, blocks, W, H)
    sc = G.Scene(cs)
    assert len(sc.textures) == 7 and {f for _, f in sc.textures} == {abi.TEX_NEAREST, abi.TEX_BILINEAR}
    _close(a32, G.render_blocks(sc, blocks, W, H), 0.95)
    assert ctr["nee_evals"] > 0 and len(np.unique(bits(a32[..., :3]))) > 1000


def test_mixed_bin_scene_oracle_vs_float64(oracle):
    cs = ts.mixed_bin_scene()
    W, H = 80, 48
    blocks = host.make_blocks(W, H, 2, 5)
    a32, _, _ = oracle.render_blocks(cs, blocks, W, H)
    _close(a32, G.render_blocks(G.Scene(cs), blocks, W, H), 0.95)


def test_textured_shading_step_vectors(oracle):
    """hjo_shade_probe on a textured scene: the NEE term and the bounce weight of textured hits are the float64 albedo's."""
    cs = ts.random_textured_scene(5, big=False)
    sc = G.Scene(cs)
    rs = np.random.RandomState(3)
    n = 20000
    o = rs.uniform((-1.1, 0.05, -1.1), (1.1, 1.9, 1.1), (n, 3))
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.concatenate([o, d, np.full((n, 1), 1e-4), np.full((n, 1), np.inf)], 1).astype(np.float32)
    rng0 = G.seed_rng(np.arange(n, dtype=np.uint32) * 5 + 1)
    out, ids, _ = oracle.shade_probe(cs, rays, rng0)
    r = rays.astype(np.float64)
    its = G.intersect_scene(sc, r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7])
    idx = np.nonzero((its.id == ids) & (ids >= 0))[0]
    mat = sc.materials[its.id[idx]]
    tag, midx = mat >> G.TAG_SHIFT, mat & ((1 << G.TAG_SHIFT) - 1)
    mt = tag == G.TEXTURED
    assert mt.sum() > 3000
    want = G.albedo(sc, tag[mt], midx[mt], its.u[idx[mt]], its.v[idx[mt]])
    got = out[idx[mt], 11:14]
    ok = (np.abs(got - want) <= 1e-4 * np.maximum(1.0, np.abs(want))).all(1)
    assert ok.mean() > 0.99, ok.mean()                # (a texel edge that float64 uv put on the other side)
    assert (out[idx[mt], 14] == 1).all()              # a textured bounce continues
    assert (out[idx[mt], 1:4] != 0).any(axis=1).sum() > 1000   # ... and takes a next-event sample


def _render_raw(oracle, cs, tset, W=32, H=16):
    """hjo_render_blocks with an explicit texture set (None: no textures) -> (status, accum)."""
    L = oracle.lib()
    blocks = host.make_blocks(W, H, 1, 3)
    acc = np.zeros((H, W, 4), np.float32)
    L.hjo_set_textures(C.byref(tset) if tset is not None else None)
    try:
        rc = L.hjo_render_blocks(C.byref(cs.desc), blocks, len(blocks), C.byref(abi.RenderOpts.default()), W, H,
                                 acc.ctypes.data_as(C.POINTER(C.c_float)), 2, None, None)
    finally:
        L.hjo_set_textures(None)
    return rc, acc


def test_oracle_refuses_bad_texture_sets(oracle):
    """What hj_scene_upload_textured refuses (tests/test_textures_gpu.py _rejects), the oracle refuses: no frame, an error."""
    tex, _, _ = ts.textured_cbox(extra=False)
    cs = tex.compile()
    good = cs.texture_set

    def refused(t, status=abi.HJ_ERR_INVALID):
        rc, acc = _render_raw(oracle, cs, t)
        assert rc == status and not acc.any()

    refused(None)                                            # tag 5 without textures
    refused(abi.TextureSet())                                # index >= num_textures
    rec = (abi.Texture * 1)()
    for w, h, f, first in ((0, 4, 0, 0), (4, 0, 0, 0), (16, 8, 2, 0), (16, 8, 0, 1)):
        rec[0] = abi.Texture(w, h, f, first)
        bad = abi.TextureSet(rec, 1, good.texels, good.num_texels)
        refused(bad)
        with pytest.raises(abi.HijikiError) as e:
            oracle.texture_lookup(bad, 0, np.zeros((1, 2), np.float32))
        assert e.value.status == abi.HJ_ERR_INVALID
    refused(abi.TextureSet(good.textures, 1, good.texels, (1 << 32) + 1), abi.HJ_ERR_UNSUPPORTED)
    L = oracle.lib()                                         # a block and a shading step without textures
    out = np.zeros((16, 16, 8), np.float32)
    blk = host.make_blocks(16, 16, 1, 3)[0]
    assert L.hjo_integrate_block(C.byref(cs.desc), C.byref(blk), C.byref(abi.RenderOpts.default()),
                                 out.ctypes.data_as(C.POINTER(C.c_float)), None) == abi.HJ_ERR_INVALID
    rays = np.array([[0, 1, 3, 0, 0, -1, 1e-4, np.inf]], np.float32)
    assert L.hjo_shade_probe(C.byref(cs.desc), rays.ctypes.data_as(C.POINTER(C.c_float)),
                             np.zeros(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), 1,
                             np.zeros(20, np.float32).ctypes.data_as(C.POINTER(C.c_float))) == abi.HJ_ERR_INVALID
    rc, acc = _render_raw(oracle, cs, good)                  # and the good set renders
    assert rc == abi.HJ_OK and (acc[..., 3] > 0).all()
