"""Image textures on the host (no GPU): the compiler's tag-5 words and texture table, the tree of a textured scene, the textured
OBJ/MTL loader with its PFM and P6 readers, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import texture_scenes as ts
from hijiki_amd import abi, device, host


def test_compile_emits_texture_words_and_table():
    s = host.Scene()
    s.set_camera_cbox()
    rgb = np.random.default_rng(3).uniform(0, 1, (3, 5, 3)).astype(np.float32)          # 5 wide, 3 high, RGB
    rgba = np.random.default_rng(4).uniform(0, 1, (2, 7, 4)).astype(np.float32)
    t0 = s.add_texture(rgb, abi.TEX_NEAREST)
    t1 = s.add_texture(rgba, abi.TEX_BILINEAR)
    assert (t0, t1) == (0, 1)
    m1 = s.add_diffuse_textured(t1)
    m0 = s.add_diffuse_textured(t0)
    d = s.add_diffuse((0.5, 0.5, 0.5))
    lamp = s.add_emissive((1, 1, 1))
    s.add_sphere((0, 0, 0), 1.0, m0)
    s.add_sphere((3, 0, 0), 1.0, m1)
    s.add_quad((0, 5, 0), (1, 0, 0), (0, 0, 1), lamp)
    s.add_quad((0, -5, 0), (1, 0, 0), (0, 0, 1), d)
    cs = s.compile()
    words = cs.materials.tolist()
    assert words[:2] == [(abi.MAT_DIFFUSE_TEXTURED << 24) + 0, (abi.MAT_DIFFUSE_TEXTURED << 24) + 1]
    assert words[2] >> 24 == abi.MAT_EMISSIVE and words[3] >> 24 == abi.MAT_DIFFUSE
    table, texels = cs.textures
    assert table == [(5, 3, abi.TEX_NEAREST, 0), (7, 2, abi.TEX_BILINEAR, 15)]
    assert texels.shape == (15 + 14, 4)
    want0 = np.concatenate([rgb, np.ones((3, 5, 1), np.float32)], axis=2).reshape(-1, 4)      # RGB -> RGBA, rows top first
    assert (texels[:15].view(np.uint32) == want0.view(np.uint32)).all()
    assert (texels[15:].view(np.uint32) == rgba.reshape(-1, 4).view(np.uint32)).all()
    # the reference's packed buffer has no place for textures
    with pytest.raises(abi.HijikiError) as e:
        cs.packed()
    assert e.value.status == abi.HJ_ERR_UNSUPPORTED
    # an untextured scene still packs, and its texture view is empty
    s2 = host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=64)
    c2 = s2.compile()
    assert c2.textures[0] == [] and c2.texture_set.num_textures == 0 and len(c2.packed()) > 0


def test_textured_scene_compiles_to_the_tree_of_its_diffuse_twin():
    """The ray vote (host) treats a textured hit as diffuse: same number of draws, same bounce - the tree is the twin's."""
    tex, twin, _ = ts.textured_cbox(seed=5)
    a, b = tex.compile(), twin.compile()
    assert len(a.bvh) == len(b.bvh) > 600
    assert (a.bvh == b.bvh).all()
    assert (a.triangles == b.triangles).all() and (a.vertices.view(np.uint32) == b.vertices.view(np.uint32)).all()
    # the tree passes on an installed tree (scene_of + vote) agree as well
    a.tune_bvh(0, 20000)
    b.tune_bvh(0, 20000)
    assert (a.bvh == b.bvh).all()


def test_textured_obj_loading(tmp_path):
    pfm = np.random.default_rng(7).uniform(0, 4, (4, 5, 3)).astype(np.float32)
    path = ts.write_obj_files(tmp_path, pfm)
    cs = host.Scene.from_obj(path, textures=True).compile()
    table, texels = cs.textures
    assert [(w, h, f) for w, h, f, _ in table] == [(3, 2, abi.TEX_BILINEAR), (5, 4, abi.TEX_BILINEAR)]
    ppm = texels[table[0][3]:table[0][3] + 6].reshape(2, 3, 4)
    assert np.allclose(ppm[..., :3], ts.srgb_to_linear(ts.PPM_PIX), rtol=1e-6, atol=0) and (ppm[..., 3] == 1).all()
    back = texels[table[1][3]:table[1][3] + 20].reshape(4, 5, 4)
    assert (back[..., :3].view(np.uint32) == pfm.view(np.uint32)).all()      # PFM round trip: linear, row 0 on top
    tags = (cs.materials >> 24).tolist()
    # floor (2 triangles: wood), back wall (2: backwall), side (plain), lamp
    assert tags == [abi.MAT_DIFFUSE_TEXTURED] * 4 + [abi.MAT_DIFFUSE, abi.MAT_EMISSIVE]
    assert ((cs.materials[:4] & 0xFFFFFF).tolist()) == [0, 0, 1, 1]
    v = cs.vertices
    uv = set(zip(v[:, 3].tolist(), v[:, 7].tolist()))
    assert {(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)} <= uv
    # without textures=True the loader is today's: map_Kd ignored, Kd diffuse, no textures
    plain = host.Scene.from_obj(path).compile()
    (tmp_path / "tex.mtl").write_text("\n".join(l for l in ts.MTL.splitlines() if not l.startswith("map_Kd")) + "\n")
    no_map = host.Scene.from_obj(path).compile()
    assert plain.textures[0] == []
    assert ((plain.materials >> 24).tolist()) == [abi.MAT_DIFFUSE] * 5 + [abi.MAT_EMISSIVE]
    for name in ("materials", "bvh", "triangles", "emitters"):
        assert (getattr(plain, name) == getattr(no_map, name)).all(), name
    assert (plain.vertices.view(np.uint32) == no_map.vertices.view(np.uint32)).all()
    assert (plain.packed() == no_map.packed()).all()


def test_texture_files_big_endian_pfm_and_bad_formats(tmp_path):
    rgb = np.random.default_rng(2).uniform(-1, 1, (3, 2, 3)).astype(np.float32)
    ts.write_pfm_big_endian(str(tmp_path / "be.pfm"), rgb)
    s = host.Scene()
    t = s.add_texture_file(str(tmp_path / "be.pfm"), abi.TEX_NEAREST)
    s.add_sphere((0, 0, 0), 1, s.add_diffuse_textured(t))
    s.add_sphere((3, 0, 0), 1, s.add_emissive((1, 1, 1)))
    cs = s.compile()
    table, texels = cs.textures
    assert table == [(2, 3, abi.TEX_NEAREST, 0)]
    assert (texels[:, :3].reshape(3, 2, 3).view(np.uint32) == rgb.view(np.uint32)).all()
    (tmp_path / "x.png").write_bytes(b"\x89PNG\r\n\x1a\n" + bytes(32))
    (tmp_path / "p3.ppm").write_text("P3\n1 1\n255\n1 2 3\n")
    (tmp_path / "deep.ppm").write_bytes(b"P6\n1 1\n65535\n" + bytes(6))
    (tmp_path / "short.ppm").write_bytes(b"P6\n4 4\n255\n" + bytes(5))
    for name in ("x.png", "p3.ppm", "deep.ppm", "short.ppm", "missing.pfm"):
        with pytest.raises(abi.HijikiError) as e:
            s.add_texture_file(str(tmp_path / name))
        assert e.value.status == abi.HJ_ERR_INVALID and str(e.value), name


def test_texture_errors(tmp_path):
    pfm = np.ones((2, 2, 3), np.float32)
    path = ts.write_obj_files(tmp_path, pfm)
    # a missing texture file
    (tmp_path / "wood.ppm").unlink()
    with pytest.raises(abi.HijikiError, match="wood.ppm"):
        host.Scene.from_obj(path, textures=True)
    host.Scene.from_obj(path)                                           # (ignored without textures)
    # map_Kd with option flags is an error, not silently ignored
    ts.write_ppm(str(tmp_path / "wood.ppm"), ts.PPM_PIX)
    (tmp_path / "tex.mtl").write_text(ts.MTL.replace("map_Kd wood.ppm", "map_Kd -s 2 2 1 wood.ppm"))
    with pytest.raises(abi.HijikiError, match="-s"):
        host.Scene.from_obj(path, textures=True)
    # out-of-range texture index, bad texel arrays
    s = host.Scene()
    with pytest.raises(abi.HijikiError) as e:
        s.add_diffuse_textured(0)
    assert e.value.status == abi.HJ_ERR_INVALID
    t = s.add_texture(np.zeros((1, 1, 3), np.float32))
    with pytest.raises(abi.HijikiError):
        s.add_diffuse_textured(t + 1)
    with pytest.raises(abi.HijikiError):
        s.add_texture(np.zeros((1, 1, 4), np.float32), filter=2)
    with pytest.raises(ValueError):
        s.add_texture(np.zeros((2, 2), np.float32))
    L = host.lib()
    assert L.hjh_scene_add_texture(s._h, 0, 1, np.zeros(4, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 4, 0) == -abi.HJ_ERR_INVALID
    assert L.hjh_scene_add_texture(s._h, 1, 1, np.zeros(4, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 2, 0) == -abi.HJ_ERR_INVALID


def test_textured_upload_argument_checks_need_no_gpu():
    L = device.lib()
    assert L.hj_scene_upload_textured(None, None, None) == abi.HJ_ERR_INVALID
    ts_ = abi.TextureSet()
    assert L.hj_scene_upload_textured(None, None, C.byref(ts_)) == abi.HJ_ERR_INVALID
    uv = np.zeros((1, 2), np.float32)
    rgb = np.zeros((1, 3), np.float32)
    fp = C.POINTER(C.c_float)
    assert L.hj_debug_texture_lookup(None, 0, uv.ctypes.data_as(fp), 1, rgb.ctypes.data_as(fp)) == abi.HJ_ERR_INVALID
    assert L.hj_version() >= 0x000400
    assert C.sizeof(abi.Texture) == 16 and abi.MAT_DIFFUSE_TEXTURED == 5


def test_numpy_lookup_restatement_edges():
    """The restatement itself at the edges the definition names (the GPU test compares the kernel with it)."""
    tex = np.zeros((2, 4, 4), np.float32)
    tex[..., 0] = np.arange(4)[None, :]
    tex[..., 1] = np.arange(2)[:, None]
    uv = np.array([[0.0, 1.0], [-1e-9, 0.0], [np.nan, np.inf], [0.99, 0.01]], np.float32)
    near = ts.lookup(tex, abi.TEX_NEAREST, uv)
    assert near[:, :2].tolist() == [[0, 1], [3, 1], [0, 1], [3, 1]]      # t = 0 is the bottom row; -1e-9 wraps to s = 1.0: the last column
    bil = ts.lookup(tex, abi.TEX_BILINEAR, uv)
    assert bil[0, :2].tolist() == [1.5, 0.5]                              # (0, 1): the corner between columns 3, 0 and rows 1, 0
