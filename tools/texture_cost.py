"""What image textures cost: Mpaths/s of the synthetic cbox whose walls and object take their colour from 2048 x 2048 textures
(nearest, then bilinear), next to its diffuse twin (the same shapes and tree, the synthetic scene's own diffuse colours).

    python tools/texture_cost.py [--spp 512] [--size 1024] [--reps 3] [--tex 2048]

uv: the vertex position projected on the wall's plane (x + z, y), so neighbouring hits read neighbouring texels, as on an unwrapped
asset.  Best frame of --reps per variant, variants interleaved twice."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hijiki_amd import abi, device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=512)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tex", type=int, default=2048)
a = ap.parse_args()

base = host.Scene.synthetic(host.SYNTH_CBOX).compile()
d = base.desc
vert = base.vertices.copy()
vert[:, 3] = (vert[:, 0] + vert[:, 2]) * 0.5 + 0.5            # u
vert[:, 7] = vert[:, 1] * 0.5                                # v
rng = np.random.default_rng(1)
textures = [rng.uniform(0.05, 0.95, (a.tex, a.tex, 4)).astype(np.float32) for _ in range(2)]


def scene(filt):
    """filt None: the diffuse twin; else walls (the first 10 diffuse triangles) and object textured with that filter."""
    s = host.Scene()
    cam = d.camera
    s.set_camera(tuple(cam.position[:3]), tuple(cam.rotation[:4]), cam.fov)
    s.add_vertices(vert[:, 0:3], vert[:, 4:7], np.stack([vert[:, 3], vert[:, 7]], 1))
    tex = [s.add_texture(t, filt) for t in textures] if filt is not None else None
    mats, seen = {}, 0
    for i, (abc, word) in enumerate(zip(base.triangles, base.materials)):
        tag, idx = int(word) >> 24, int(word) & 0xFFFFFF
        if tag == abi.MAT_EMISSIVE:
            key = ("e", idx)
            if key not in mats:
                mats[key] = s.add_emissive(tuple(d.emissive[idx].power))
        elif filt is None:
            key = ("d", idx)
            if key not in mats:
                mats[key] = s.add_diffuse(tuple(d.diffuse[idx].color))
        else:
            seen += 1
            key = ("t", 0 if seen <= 10 else 1)
            if key not in mats:
                mats[key] = s.add_diffuse_textured(tex[key[1]])
        s.add_triangle(int(abc[0]), int(abc[1]), int(abc[2]), mats[key])
    return s.compile()


twin = scene(None)
variants = {"diffuse twin": twin, "nearest": scene(abi.TEX_NEAREST), "bilinear": scene(abi.TEX_BILINEAR)}
for cs in variants.values():
    cs.set_bvh(twin.bvh)                                      # one tree for all three
r = device.Renderer(0)
best = {k: 0.0 for k in variants}
for _ in range(2):
    for name, cs in variants.items():
        r.upload_scene(cs)
        r.create_framebuffer(a.size, a.size)
        o = device.default_opts()
        r.reserve(a.spp * host.blocks_per_pass(a.size, a.size), o)
        r.render_frame(1, 1, opts=o)                          # warm-up
        for _ in range(a.reps):
            r.clear()
            t = time.perf_counter()
            r.render_frame(a.spp, 1, opts=o)
            dt = time.perf_counter() - t
            best[name] = max(best[name], a.size * a.size * a.spp / dt / 1e6)
for name, v in best.items():
    print(f"{name:13s} {a.size}x{a.size}x{a.spp}, {a.tex}^2 textures: {v:8.1f} Mpaths/s  ({100.0 * (v / best['diffuse twin'] - 1):+.1f} %)")
r.close()
