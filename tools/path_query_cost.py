"""What a path query costs: hj_trace_paths on rays that stay on the device (HJ_PATHS_DEVICE_ARRAYS, torch tensors) beside the
renderer's own frame, on one box, interleaved:

    (a) the camera rays of a --size x --size, --spp cbox frame (pixel centres; one query of size^2 rays at spp samples each),
    (b) hj_render_frame of the same frame with the library as built (paths traced AND reconstructed: the query reconstructs nothing),
    (c) one generation of incoherent rays built in torch from trace_rays' surface records of (a)'s rays: from p + 2e-4 n into a
        seeded random direction in the hemisphere of n, one per camera ray that hit, at the same spp.

--pairs rounds of (a), (b), (c) after a warm-up of each; paths/s lowest ... highest of each.  A call's time is a host clock around it
(each returns when its results are complete) and includes the launches.  The table belongs in DESIGN.md ("Path queries"), the raw
output in profiles/.  Run under its own time limit:

    timeout -k 10 300 python tools/path_query_cost.py
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)
from hijiki_amd import device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--pairs", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()

cs = host.Scene.synthetic(host.SYNTH_CBOX).compile()
dev = torch.device("cuda", 0)
r = device.Renderer(0)
r.upload_scene(cs)
r.create_framebuffer(a.size, a.size)

from oracle import hj_oracle  # noqa: E402  (the camera's rays, as the renderer makes them for pixel centres)
ys, xs = np.mgrid[0:a.size, 0:a.size]
pix = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
cam = np.zeros((len(pix), 8), np.float32)
cam[:, 0:6] = hj_oracle.camera_rays(cs.desc.camera, a.size, a.size, pix)
cam.view(np.uint32)[:, 6] = np.random.default_rng(a.seed).integers(0, 1 << 32, len(cam), dtype=np.uint64).astype(np.uint32)
primary = torch.from_numpy(cam).to(dev)

probe = primary.clone()
probe[:, 6], probe[:, 7] = 1e-4, float("inf")
ids, _, _, _, surf = r.trace_rays(probe, surface=True)
hit = ids >= 0
p, n = surf[hit, 0:3], surf[hit, 3:6]
g = torch.Generator(device=dev)
g.manual_seed(a.seed)
d = torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32)
d = d / d.norm(dim=1, keepdim=True)
d = torch.where((d * n).sum(dim=1, keepdim=True) < 0, -d, d)
bounce = torch.zeros((p.shape[0], 8), device=dev, dtype=torch.float32)
bounce[:, 0:3], bounce[:, 3:6] = p + 2e-4 * n, d
bounce.view(torch.int32)[:, 6] = primary.view(torch.int32)[hit, 6]
bounce = bounce.contiguous()
print(f"cbox {a.size} x {a.size} x {a.spp}: (a) {len(primary)} camera rays, {int(hit.sum())} hit; (c) {len(bounce)} incoherent rays from their surface records")


def query(rays):
    t = time.perf_counter()
    _, st = r.trace_paths(rays, spp=a.spp, stats=True)
    return st["paths"] / (time.perf_counter() - t), st


def frame():
    r.clear()
    t = time.perf_counter()
    st = r.render_frame(a.spp, 1)
    return st["paths"] / (time.perf_counter() - t), st


runs = {"(a) query, camera rays": lambda: query(primary), "(b) hj_render_frame": frame, "(c) query, incoherent rays": lambda: query(bounce)}
rate = {k: [] for k in runs}
stats = {k: f()[1] for k, f in runs.items()}                            # warm-up of each (allocations, first launches)
for _ in range(a.pairs):
    for k, f in runs.items():
        rate[k].append(f()[0])
for k, v in rate.items():
    st = stats[k]
    print(f"{k}: {st['paths']} paths, {st['closest_rays'] + st['shadow_rays']} rays, {st['batches']} launches; {a.pairs} interleaved runs, "
          f"Mpaths/s lowest ... highest: {min(v) / 1e6:.1f} ... {max(v) / 1e6:.1f}")
print(f"(a) / (b), highest: {max(rate['(a) query, camera rays']) / max(rate['(b) hj_render_frame']):.2f}")
r.close()
