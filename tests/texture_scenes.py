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


# -------------------------------------------------------------------------------- scenes whose colour varies across surfaces

TEXTURE_SHAPES = ((1, 1), (1, 9), (9, 1), (7, 5), (13, 9), (3, 2048))     # (H, W): 1 x 1, 1 x N, N x 1, odd sizes, 2048 x 3


def random_texels(rng, H, W):
    """Random colours, a few of them outside [0, 1] (negative ones included)."""
    t = np.ones((H, W, 4), F)
    t[..., :3] = rng.uniform(0.05, 0.95, (H, W, 3))
    out = rng.random((H, W)) < 0.1
    t[out, :3] = rng.uniform(-0.5, 1.6, (int(out.sum()), 3))
    return t


def _uv(rng, n, widths):
    """n vertex uv in [-3, 3]: some at integers, some on texel edges k / W of the scene's textures."""
    uv = rng.uniform(-3, 3, (n, 2))
    kind = rng.integers(0, 4, (n, 2))
    uv[kind == 1] = rng.integers(-3, 4, int((kind == 1).sum()))
    edge = kind == 2
    w = rng.choice(widths, int(edge.sum()))
    uv[edge] = rng.integers(-3 * w, 3 * w + 1) / w
    return uv.astype(F)


def random_textured_scene(seed, big=True):
    """tests/scenes.py random_scene with image textures: a 1024 x 1024 texture first (big=False: 64 x 48), so the small ones start
    a million texels into the buffer, then 1 x 1, 1 x 9, 9 x 1, odd and 2048 x 3 ones, nearest and bilinear, some texels outside
    [0, 1]; textured quads (walls among them), spheres (the lat-long seam) and triangles whose vertex uv lie in [-3, 3], on
    integers and on texel edges; every other material kind alongside."""
    rng = np.random.default_rng(3000 + seed)
    s = host.Scene()
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    q = q * 0.15 + np.array([0, 0, 0, 1.0])
    q /= np.linalg.norm(q)
    s.set_camera((float(rng.uniform(-0.2, 0.2)), float(rng.uniform(0.7, 1.0)), float(rng.uniform(3.0, 3.6))),
                 tuple(float(x) for x in q), float(rng.uniform(25, 45)))
    shapes = [(1024, 1024) if big else (48, 64)] + list(TEXTURE_SHAPES)
    filters = [abi.TEX_NEAREST, abi.TEX_BILINEAR] + [int(f) for f in rng.integers(0, 2, len(shapes) - 2)]
    widths = []
    textured = []
    for (h, w), f in zip(shapes, filters):
        textured.append(s.add_diffuse_textured(s.add_texture(random_texels(rng, h, w), f)))
        widths.append(w)
    plain = [s.add_diffuse(tuple(rng.uniform(0.1, 0.9, 3))) for _ in range(2)]
    other = [s.add_diffuse_cboard(tuple(rng.uniform(0.2, 0.9, 3)), float(rng.uniform(0.05, 0.3)),
                                  tuple(rng.uniform(0.1, 0.8, 3)), float(rng.uniform(0.05, 0.3))),
             s.add_mirror(), s.add_dielectric(float(rng.uniform(1.2, 1.8))),
             s.add_dielectric(1.5, extinction=tuple(rng.uniform(0.0, 2.0, 3)))]
    lights = [s.add_emissive(tuple(rng.uniform(5, 25, 3))) for _ in range(2)]
    mats = textured + textured + plain + other
    walls = [int(rng.choice(textured)), int(rng.choice(textured)), other[0], plain[0]]
    s.add_quad((-1.2, 0, 1.2), (2.4, 0, 0), (0, 0, -2.4), walls[0])
    s.add_quad((-1.2, 0, -1.2), (2.4, 0, 0), (0, 2.0, 0), walls[1])
    s.add_quad((-1.2, 0, 1.2), (0, 0, -2.4), (0, 2.0, 0), walls[2])
    s.add_quad((1.2, 0, -1.2), (0, 0, 2.4), (0, 2.0, 0), walls[3])
    s.add_quad((-0.4, 1.99, -0.4), (0.8, 0, 0), (0, 0, 0.8), lights[0])
    for k in range(int(rng.integers(3, 7))):
        m = textured[int(rng.integers(0, len(textured)))] if k < 2 else int(rng.choice(mats + lights[1:]))
        s.add_sphere(tuple(rng.uniform([-0.8, 0.2, -0.8], [0.8, 1.2, 0.8])), float(rng.uniform(0.1, 0.35)), m)
    s.add_quad(tuple(rng.uniform([-0.9, 0.1, -0.9], [0.3, 0.6, 0.3])), (0.5, 0.0, 0.1), (0.0, 0.5, 0.05), int(rng.choice(textured)))
    nv = int(rng.integers(16, 40))
    pos = rng.uniform([-0.9, 0.05, -0.9], [0.9, 1.5, 0.9], (nv, 3)).astype(F)
    nrm = rng.normal(size=(nv, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    base = s.add_vertices(pos, nrm, _uv(rng, nv, widths))
    for _ in range(int(rng.integers(12, 36))):
        a, b, c = (int(x) for x in rng.choice(nv, 3, replace=False))
        s.add_triangle(base + a, base + b, base + c, int(rng.choice(mats + lights[1:])))
    return s.compile()


def mixed_bin_scene(seed=0, n=24, W=9, H=7, filt=abi.TEX_BILINEAR):
    """The hit bin that textured hits share with the checkerboard (DESIGN.md "Image textures"): a floor and a back wall of n x n
    cells, each two triangles, whose materials run checkerboard, textured, plain diffuse from one triangle to the next - the
    waves of that bin hold lookups and checkerboards side by side.  uv follow the position, so both vary across the mesh."""
    rng = np.random.default_rng(4000 + seed)
    s = host.Scene()
    s.set_camera_cbox()
    tex = s.add_diffuse_textured(s.add_texture(random_texels(rng, H, W), filt))
    cb = s.add_diffuse_cboard((0.9, 0.8, 0.2), 0.07, (0.1, 0.3, 0.8), 0.11)
    plain = s.add_diffuse((0.6, 0.6, 0.6))
    light = s.add_emissive((15.0, 14.0, 12.0))
    s.add_quad((-0.4, 1.99, -0.4), (0.8, 0, 0), (0, 0, 0.8), light)
    s.add_sphere((0.3, 0.35, 0.2), 0.3, tex)
    cycle = (cb, tex, plain)
    g = np.linspace(-1.2, 1.2, n + 1, dtype=F)
    k = 0
    for plane in ("floor", "back"):
        if plane == "floor":
            pos = np.array([[x, 0.0, z] for z in g for x in g], F)
            nrm = np.tile(np.array([[0, 1, 0]], F), (len(pos), 1))
            uv = np.stack([pos[:, 0] * 1.7, pos[:, 2] * 1.3], 1)
        else:
            pos = np.array([[x, (y + 1.2) / 1.2, -1.2] for y in g for x in g], F)
            nrm = np.tile(np.array([[0, 0, 1]], F), (len(pos), 1))
            uv = np.stack([pos[:, 0] * 2.1 + 0.3, pos[:, 1] * 1.9], 1)
        b = s.add_vertices(pos, nrm, uv.astype(F))
        for j in range(n):
            for i in range(n):
                v00 = b + j * (n + 1) + i
                v01, v10, v11 = v00 + 1, v00 + n + 1, v00 + n + 2
                tris = ((v00, v10, v01), (v01, v10, v11)) if plane == "floor" else ((v00, v01, v10), (v01, v11, v10))
                for t in tris:
                    s.add_triangle(*t, cycle[k % 3])
                    k += 1
    return s.compile()


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
