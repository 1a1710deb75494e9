"""What hj_render_motion costs, and what it buys the temporal denoiser.

    --mode cost:     the milliseconds of hj_render_motion at --size x --size (1024) into a device tensor, the previous state being the
                     uploaded one (every kind staged from the host: the upload of the previous arrays is part of a call), on the box
                     with the spheres (--scene cbox) or the 1 M-triangle mesh (--scene mesh).  One warm-up call, then the median
                     (min ... max) of --rounds calls; a call's time is a host clock around it (it returns after its stream synchronise).
    --mode quality:  the box with the spheres at --size x --size (256), sphere 0 moved --step pixels a frame by hj_scene_update_shapes
                     under a fixed camera; --frames (8) frames of --spp (4); per frame hj_render_aovs, hj_render_motion against the old
                     spheres, and the two temporal chains - hj_denoise_frame_temporal and hj_denoise_frame_temporal_motion.  The
                     error is the mean squared difference to a --truth-spp frame of the last pose over the pixels whose centre ray
                     hits the mover in the last frame or that it uncovered since the frame before: the spatial filter alone, the
                     static temporal call, the motion call - and the same three over the whole image.

One mode and one scene per process, each under its own time limit, chained:

    timeout -k 10 300 python tools/motion_cost.py --mode cost --scene cbox && timeout -k 10 420 python tools/motion_cost.py --mode cost --scene mesh \\
      && timeout -k 10 300 python tools/motion_cost.py --mode quality
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)
from hijiki_amd import abi, device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["cost", "quality"], default="cost")
ap.add_argument("--scene", choices=["cbox", "mesh"], default="cbox", help="cost mode - cbox: the Cornell box with the spheres; mesh: 1 M triangles")
ap.add_argument("--size", type=int, default=0, help="default: 1024 (cost), 256 (quality)")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--step", type=float, default=3.0, help="pixels a frame")
ap.add_argument("--truth-spp", type=int, default=1024)
a = ap.parse_args()


class Prev:
    """a previous state in the form render_motion takes: cs's desc with another sphere array (None: the uploaded ones) and camera"""

    def __init__(self, cs, spheres=None):
        self.desc = abi.SceneDesc()
        C.memmove(C.byref(self.desc), C.byref(cs.desc), C.sizeof(abi.SceneDesc))
        self.spheres = None if spheres is None else np.ascontiguousarray(spheres, np.float32)
        if self.spheres is not None:
            self.desc.spheres = C.cast(C.c_void_p(self.spheres.ctypes.data), C.POINTER(abi.Sphere))


r = device.Renderer(0)
if a.mode == "cost":
    size = a.size or 1024
    kind, tris = (host.SYNTH_CBOX_SPHERES, 0) if a.scene == "cbox" else (host.SYNTH_CBOX_MESH, 1000000)
    cs = host.Scene.synthetic(kind, mesh_triangles=tris).compile()
    r.upload_scene(cs)
    prev = Prev(cs)
    m = r.render_motion(prev, size, size, device=True)                  # (the warm-up)
    hits = int((device.motion_ids(m) != abi.MOTION_NONE).sum())
    ms = []
    for _ in range(a.rounds):
        t = time.perf_counter()
        r.render_motion(prev, size, size, device=True)
        ms.append((time.perf_counter() - t) * 1e3)
    print(f"{a.scene}: {cs.num_shapes} shapes, {size} x {size} = {size * size} centre rays, {hits} with a previous position; {a.rounds} rounds after one warm-up")
    print(f"{a.scene} render_motion: {statistics.median(ms):.2f} ({min(ms):.2f} ... {max(ms):.2f}) ms, {size * size / statistics.median(ms) / 1e6:.2f} G pixels/s")
else:
    W = H = a.size or 256
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile()
    cam = cs.desc.camera
    rest = cs.spheres.copy()
    dist = float(np.linalg.norm(rest[0, 0:3] - np.array(list(cam.position)[0:3], np.float32)))
    pixel = 2.0 * dist * math.tan(math.radians(cam.fov / 2)) / W         # the side of a pixel at the mover's distance
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    hs = hm = None
    ids = []
    for k in range(a.frames):
        before = cs.spheres.copy()
        cs.spheres[0, 0] = rest[0, 0] + np.float32((k - a.frames / 2) * a.step * pixel)
        r.update_shapes(cs)
        r.clear()
        r.render_frame(a.spp, 100 + k)
        aov = r.render_aovs(W, H, spp=a.spp, master_seed=100 + k)
        motion = r.render_motion(Prev(cs, before), W, H)
        ids.append(device.motion_ids(motion).copy())
        static, hs = r.denoise_frame_temporal(aov, cam, cam, hs)
        moved, hm = r.denoise_frame_temporal(aov, cam, cam, hm, motion=motion)
    spatial = r.denoise_frame(aov)
    r.clear()
    r.render_frame(a.truth_spp, 999)
    truth = r.resolve().astype(np.float64)
    mover = (ids[-1] == 0) | ((ids[-2] == 0) & (ids[-1] != 0))
    guided = hm.view(np.uint32)[..., 7] != 0
    mse = lambda img, m: float(np.mean((img[..., 0:3].astype(np.float64) - truth)[m] ** 2))            # noqa: E731
    print(f"quality: {W} x {H}, sphere 0 moved {a.step} pixels a frame ({a.step * pixel:.4f} units), {a.frames} frames of {a.spp} spp, truth {a.truth_spp} spp")
    print(f"mover pixels (hit in the last frame or uncovered since the one before): {int(mover.sum())}, of them guided {int((mover & guided).sum())}; "
          f"mean history length there: static {float(hs[..., 3][mover & guided].mean()) if (mover & guided).any() else 0:.2f}, "
          f"motion {float(hm[..., 3][mover & guided].mean()) if (mover & guided).any() else 0:.2f}")
    for what, msk in (("mover pixels", mover), ("whole image", np.ones((H, W), bool))):
        print(f"{what}: mse spatial {mse(spatial, msk):.6g}, static temporal {mse(static, msk):.6g}, motion temporal {mse(moved, msk):.6g}")
r.close()
