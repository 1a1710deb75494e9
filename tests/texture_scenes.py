"""Textured scenes and their diffuse twins, the OBJ/MTL/image files of the textured loader, and the lookup of DESIGN.md
"Image textures" restated in numpy float32 (tests/test_textures_host.py, tests/test_textures_gpu.py)."""
import struct

import numpy as np

from hijiki_amd import abi, host

F = np.float32


def lookup(tex, filt, uv):
    """The texture lookup, float32 throughout, in the order the definition gives: tex = (H, W, 4) texels (row 0 on top),
    uv = (n, 2) -> (n, 3)."""
    H, W = tex.shape[:2]
    uv = np.asarray(uv, F).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        s = uv[:, 0] - np.floor(uv[:, 0])
        t = uv[:, 1] - np.floor(uv[:, 1])
        s = np.where(np.isfinite(s), s, F(0)).astype(F)
        t = np.where(np.isfinite(t), t, F(0)).astype(F)
        if filt == abi.TEX_NEAREST:
            x = np.minimum((s * F(W)).astype(np.int64), W - 1)
            y = np.minimum(((F(1) - t) * F(H)).astype(np.int64), H - 1)
            return tex[y, x, :3].astype(F)
        fx = s * F(W) - F(0.5)
        fy = (F(1) - t) * F(H) - F(0.5)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = (fx - x0f)[:, None], (fy - y0f)[:, None]
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        xa, xb, ya, yb = np.mod(x0, W), np.mod(x0 + 1, W), np.mod(y0, H), np.mod(y0 + 1, H)
        c00, c10, c01, c11 = (tex[yy, xx, :3].astype(F) for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
        bx, by = F(1) - ax, F(1) - ay
        return ((c00 * bx + c10 * ax) * by + (c01 * bx + c11 * ax) * ay).astype(F)


def srgb_to_linear(b):
    """The sRGB EOTF of 8-bit values, evaluated in double and rounded once to float32."""
    c = np.asarray(b, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(F)


def cbox_parts(mesh_triangles=320):
    """The synthetic Cornell box as arrays: triangles, vertices (positions and normals as compiled), material words, the emissive
    records and the camera."""
    cs = host.Scene.synthetic(host.SYNTH_CBOX, mesh_triangles=mesh_triangles).compile()
    d = cs.desc
    tri = cs.triangles
    vert = cs.vertices
    emissive = np.array([list(d.emissive[i].power) for i in range(d.num_emissive)], F).reshape(-1, 3)
    cam = d.camera
    return dict(tri=tri.copy(), vert=vert.copy(), mat=cs.materials.copy(), emissive=emissive,
                camera=(tuple(cam.position[:3]), tuple(cam.rotation[:4]), cam.fov))


def textured_cbox(seed=1, W=16, H=8, extra=True, filt=abi.TEX_NEAREST):
    """(textured scene, diffuse twin, the texture): the synthetic cbox's walls, light and object, every diffuse triangle with all
    three vertex uv at the centre of one texel of a random-colour W x H texture; the twin gives each triangle a diffuse material of
    that texel's colour.  extra: a sphere and a quad with 1 x 1 textures (their twins: that texel's colour)."""
    p = cbox_parts()
    rng = np.random.default_rng(seed)
    tex = np.ones((H, W, 4), F)
    tex[..., :3] = rng.uniform(0.05, 0.95, (H, W, 3)).astype(F)
    one = rng.uniform(0.1, 0.9, (2, 3)).astype(F)
    scenes = []
    for textured in (True, False):
        s = host.Scene()
        s.set_camera(*p["camera"])
        t = s.add_texture(tex, filt) if textured else None
        lights = [s.add_emissive(tuple(e)) for e in p["emissive"]]
        for i, (abc, word) in enumerate(zip(p["tri"], p["mat"])):
            k = i % (W * H)
            x, y = k % W, k // W
            u, v = F((x + 0.5) / W), F(1) - F((y + 0.5) / H)
            vs = p["vert"][abc]
            uv = np.tile([u, v], (3, 1))
            first = s.add_vertices(vs[:, 0:3], vs[:, 4:7], uv)
            if word >> 24 == abi.MAT_EMISSIVE:
                m = lights[word & 0xFFFFFF]
            elif textured:
                m = s.add_diffuse_textured(t)
            else:
                m = s.add_diffuse(tuple(tex[y, x, :3]))
            s.add_triangle(first, first + 1, first + 2, m)
        if extra:
            for j, shape in enumerate(("sphere", "quad")):
                m = s.add_diffuse_textured(s.add_texture(one[j].reshape(1, 1, 3))) if textured else s.add_diffuse(tuple(one[j]))
                if shape == "sphere":
                    s.add_sphere((-0.45, 0.35, -0.3), 0.3, m)
                else:
                    s.add_quad((0.2, 0.05, 0.1), (0.5, 0.0, 0.1), (0.0, 0.5, 0.0), m)
        scenes.append(s)
    return scenes[0], scenes[1], tex


# -------------------------------------------------------------------------------- files of the textured OBJ loader

OBJ = """mtllib tex.mtl
o floor
v -1 0 -1
v 1 0 -1
v 1 0 1
v -1 0 1
vn 0 1 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
usemtl wood
f 1/1/1 2/2/1 3/3/1 4/4/1
o back
v -1 0 -1
v 1 0 -1
v 1 2 -1
v -1 2 -1
vn 0 0 1
usemtl backwall
f 5/1/2 6/2/2 7/3/2 8/4/2
o side
v -1 0 1
v -1 0 -1
v -1 2 -1
vn 1 0 0
usemtl plain
f 9/1/3 10/2/3 11/3/3
o lamp
v -0.3 1.99 -0.3
v 0.3 1.99 -0.3
v 0.3 1.99 0.3
vn 0 -1 0
usemtl light_top
f 12//4 13//4 14//4
"""
MTL = """newmtl wood
Kd 0.5 0.25 0.125
map_Kd wood.ppm
newmtl backwall
Kd 0.2 0.6 0.3
map_Kd img/back.pfm
newmtl plain
Kd 0.7 0.7 0.7
newmtl light_top
Kd 0 0 0
Ke 6 5 4
"""
PPM_PIX = np.array([[[0, 10, 40], [128, 200, 255], [5, 11, 250]],
                    [[255, 0, 64], [33, 66, 99], [190, 180, 170]]], np.uint8)    # 3 x 2, row 0 on top


def write_ppm(path, pix):
    h, w = pix.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n# written by the tests\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(pix, np.uint8).tobytes())


def write_pfm_big_endian(path, rgb):
    """A PFM with a positive scale (big-endian samples), bottom row first."""
    h, w = rgb.shape[:2]
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n1.0\n" % (w, h))
        for y in range(h - 1, -1, -1):
            f.write(struct.pack(">%df" % (3 * w), *rgb[y].reshape(-1).tolist()))


def write_obj_files(d, pfm_rgb):
    """OBJ + MTL + wood.ppm + img/back.pfm under directory d (pathlib); returns the OBJ path."""
    (d / "img").mkdir(exist_ok=True)
    (d / "scene.obj").write_text(OBJ)
    (d / "tex.mtl").write_text(MTL)
    write_ppm(str(d / "wood.ppm"), PPM_PIX)
    host.write_image(str(d / "img" / "back.pfm"), pfm_rgb)
    return str(d / "scene.obj")
