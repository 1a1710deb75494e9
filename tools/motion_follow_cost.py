"""What hj_render_motion_followed costs, and what it buys the temporal denoiser on mirrors and glass.

    --mode cost:     on the box with the spheres at --size x --size (1024), into a device tensor, the previous state being the uploaded
                     one: the milliseconds of hj_render_motion and of hj_render_motion_followed at max_follow 0, 2 and 8 - the four
                     calls interleaved, round by round, so that a drift of the machine falls on all of them.  One warm-up call each,
                     then the median (min ... max) of --rounds rounds; a call's time is a host clock around it (it returns after its
                     stream synchronise).  max_follow = 0 issues hj_render_motion's two launches and must cost what it costs.
                     Against the parent commit: tools/motion_cost.py --mode cost --scene cbox, which both trees have, run from a
                     checkout of each in alternation.
    --mode quality:  the box with the spheres at --size x --size (256); a sphere that is neither the mirror nor a light moves --step
                     pixels a frame by hj_scene_update_shapes under a fixed camera and is seen in the mirror; --frames (8) frames of
                     --spp (4).  Guides: hj_render_aovs_frame_followed at max_follow 2.  Three temporal chains over the same frames -
                     followed motion, first-hit motion, no motion (the static call) - and the spatial filter alone.  The error is
                     the mean squared difference to a --truth-spp frame of the last pose over the SPECULAR pixels (first hit a
                     mirror or a dielectric), with the mean history length there.

One mode per process, each under its own time limit, chained:

    timeout -k 10 300 python tools/motion_follow_cost.py --mode cost && timeout -k 10 300 python tools/motion_follow_cost.py --mode quality
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
ap.add_argument("--size", type=int, default=0, help="default: 1024 (cost), 256 (quality)")
ap.add_argument("--rounds", type=int, default=15)
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


L = device.lib()
r = device.Renderer(0)
cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile()
if a.mode == "cost":
    size = a.size or 1024
    r.upload_scene(cs)
    prev = Prev(cs)
    out = torch.empty((size, size, abi.MOTION_WORDS), dtype=torch.float32, device=torch.device("cuda", r.device))
    torch.cuda.synchronize()
    flags = abi.MOTION_DEVICE_OUT

    def first_hit():
        r._check(L.hj_render_motion(r._h, C.byref(prev.desc), size, size, flags, out.data_ptr()))

    def followed(n):
        return lambda: r._check(L.hj_render_motion_followed(r._h, C.byref(prev.desc), size, size, n, flags, out.data_ptr()))

    calls = [("hj_render_motion", first_hit)] + [(f"hj_render_motion_followed, max_follow {n}", followed(n)) for n in (0, 2, 8)]
    ms = {name: [] for name, _ in calls}
    for name, call in calls:                                            # (the warm-up)
        call()
    for _ in range(a.rounds):
        for name, call in calls:
            t = time.perf_counter()
            call()
            ms[name].append((time.perf_counter() - t) * 1e3)
    print(f"library {device.HIP_LIB_PATH}: cbox with the spheres, {cs.num_shapes} shapes, {size} x {size} centre rays; {a.rounds} interleaved rounds after one warm-up")
    for name, _ in calls:
        v = ms[name]
        print(f"{name}: {statistics.median(v):.3f} ({min(v):.3f} ... {max(v):.3f}) ms")
    followed(8)()
    ids = device.motion_ids(out.cpu().numpy())
    first_hit()
    base = device.motion_ids(out.cpu().numpy())
    print(f"pixels whose record the chain changed at max_follow 8: {int((ids != base).sum())}, of them left into nothing: {int((ids == abi.MOTION_LEFT).sum())}")
else:
    W = H = a.size or 256
    cam = cs.desc.camera
    tags = np.asarray(cs.materials, np.uint32) >> abi.MATERIAL_TAG_SHIFT
    ns = len(cs.spheres)
    movers = [i for i in range(ns) if tags[i] not in (abi.MAT_MIRROR, abi.MAT_EMISSIVE)]
    assert movers and (tags[:ns] == abi.MAT_MIRROR).any(), "the scene needs a mirror sphere and another sphere"
    mv = movers[0]
    rest = cs.spheres.copy()
    dist = float(np.linalg.norm(rest[mv, 0:3] - np.array(list(cam.position)[0:3], np.float32)))
    pixel = 2.0 * dist * math.tan(math.radians(cam.fov / 2)) / W         # the side of a pixel at the mover's distance
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    hf = h1 = hs = None
    for k in range(a.frames):
        before = cs.spheres.copy()
        cs.spheres[mv, 0] = rest[mv, 0] + np.float32((k - a.frames / 2) * a.step * pixel)
        r.update_shapes(cs)
        r.clear()
        r.render_frame(a.spp, 100 + k)
        aov = r.render_aovs(W, H, spp=a.spp, master_seed=100 + k, follow=2)
        prev = Prev(cs, before)
        mf, m1 = r.render_motion(prev, W, H, follow=2), r.render_motion(prev, W, H)
        out_f, hf = r.denoise_frame_temporal(aov, cam, cam, hf, motion=mf)
        out_1, h1 = r.denoise_frame_temporal(aov, cam, cam, h1, motion=m1)
        out_s, hs = r.denoise_frame_temporal(aov, cam, cam, hs)
    spatial = r.denoise_frame(aov)
    r.clear()
    r.render_frame(a.truth_spp, 999)
    truth = r.resolve().astype(np.float64)
    first = device.motion_ids(m1).astype(np.int64)
    first[first >= cs.num_shapes] = -1
    specular = (first >= 0) & np.isin(tags[np.maximum(first, 0)], (abi.MAT_MIRROR, abi.MAT_DIELECTRIC))
    guided = hf.view(np.uint32)[..., 7] != 0
    msk = specular & guided
    mse = lambda img: float(np.mean((img[..., 0:3].astype(np.float64) - truth)[msk] ** 2))            # noqa: E731
    print(f"quality: {W} x {H}, sphere {mv} moved {a.step} pixels a frame, {a.frames} frames of {a.spp} spp, followed guides (max_follow 2), truth {a.truth_spp} spp")
    print(f"specular pixels: {int(specular.sum())}, of them guided {int(msk.sum())}; mean history length there: followed motion {float(hf[..., 3][msk].mean()):.2f}, "
          f"first-hit motion {float(h1[..., 3][msk].mean()):.2f}, no motion {float(hs[..., 3][msk].mean()):.2f}")
    print(f"specular pixels: mse spatial {mse(spatial):.6g}, followed motion {mse(out_f):.6g}, first-hit motion {mse(out_1):.6g}, no motion {mse(out_s):.6g}")
r.close()
