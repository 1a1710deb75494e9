"""What an all-hit query costs beside the closest hit: hj_trace_rays_all at K = 0 (counting) and K = 8, and hj_points_inside, on arrays
that stay on the device (torch tensors), each timed beside hj_trace_rays (closest hit) on the same rays:

    2^20 camera rays (a 1024 x 1024 camera, pixel centres) on the scene, K = 0 and K = 8;
    2^20 uniformly random points in the box of the scene's vertices through points_inside.

Interleaved (closest, K = 0, K = 8, inside, closest, ...), 3 warm-up rounds, the median (min ... max) of --rounds calls each; a call's
time is a host clock around it (it returns after its stream synchronise) and includes the launch.  One scene per process, each under
its own time limit, chained:

    timeout -k 10 300 python tools/allhits_cost.py --scene cbox && timeout -k 10 420 python tools/allhits_cost.py --scene mesh
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)
from hijiki_amd import device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", choices=["cbox", "mesh"], default="cbox", help="cbox: the Cornell box; mesh: 1 M triangles")
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=15)
a = ap.parse_args()

kind, tris = (host.SYNTH_CBOX, 0) if a.scene == "cbox" else (host.SYNTH_CBOX_MESH, 1000000)
cs = host.Scene.synthetic(kind, mesh_triangles=tris).compile()
r = device.Renderer(0)
r.upload_scene(cs)
dev = torch.device("cuda", 0)

from oracle import hj_oracle  # noqa: E402  (the camera's rays, as the renderer makes them for pixel centres)
ys, xs = np.mgrid[0:a.size, 0:a.size]
pix = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
cam = np.zeros((len(pix), 8), np.float32)
cam[:, 0:6] = hj_oracle.camera_rays(cs.desc.camera, a.size, a.size, pix)
cam[:, 6], cam[:, 7] = 0.0, np.inf
rays = torch.from_numpy(cam).to(dev)
v = cs.vertices[:, 0:3]
lo, hi = v.min(0), v.max(0)
rng = np.random.default_rng(1)
pts = np.zeros((len(cam), 4), np.float32)
pts[:, 0:3] = rng.uniform(lo, hi, (len(cam), 3))
points = torch.from_numpy(pts).to(dev)

calls = {"closest hit": lambda: r.trace_rays(rays), "all hits K = 0": lambda: r.trace_rays_all(rays, 0),
         "all hits K = 8": lambda: r.trace_rays_all(rays, 8), "points_inside": lambda: r.points_inside(points)}
for _ in range(3):
    for f in calls.values():
        f()
ms = {k: [] for k in calls}
for _ in range(a.rounds):
    for k, f in calls.items():
        t = time.perf_counter()
        f()
        ms[k].append((time.perf_counter() - t) * 1e3)
counts = r.trace_rays_all(rays, 0)[0]
inside = r.points_inside(points)[0]
print(f"{a.scene}: {cs.num_shapes} shapes, {len(cam)} camera rays with {counts.sum().item() / len(cam):.2f} candidates a ray (most {counts.max().item()}), "
      f"{len(pts)} points of which {inside.sum().item()} inside; {a.rounds} interleaved rounds")
base = statistics.median(ms["closest hit"])
for k, t in ms.items():
    print(f"{a.scene} {k}: {statistics.median(t):.2f} ({min(t):.2f} ... {max(t):.2f}) ms, {statistics.median(t) / base:.2f} x closest hit")
r.close()
