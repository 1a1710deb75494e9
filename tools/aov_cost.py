"""What a frame's AOVs cost, and whether the fused fetch pays: on arrays that stay on the device (torch tensors),

    render_aovs_frame:   hj_render_aovs_frame at --size x --size with --spp samples a pixel (1024 x 1024 x 16 = 2^24 camera rays):
                         k_aov_walk builds each ray from its sample index, k_aov_resolve adds the records pass by pass;
    trace_rays+surface:  hj_trace_rays with the surface on the SAME camera rays from a device ray array - the way to the same hits
                         without this entry point (32 bytes a ray read that the fused walk never loads, 80 bytes a ray written).

One warm-up call each, then the median (min ... max) of --rounds calls each, interleaved; a call's time is a host clock around it (it
returns after its stream synchronise) and includes its launches and torch's allocation of the outputs.  One scene per process, each
under its own time limit, chained:

    timeout -k 10 300 python tools/aov_cost.py --scene cbox && timeout -k 10 420 python tools/aov_cost.py --scene mesh
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
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

kind, tris = (host.SYNTH_CBOX, 0) if a.scene == "cbox" else (host.SYNTH_CBOX_MESH, 1000000)
cs = host.Scene.synthetic(kind, mesh_triangles=tris).compile()
r = device.Renderer(0)
r.upload_scene(cs)
dev = torch.device("cuda", 0)

# the frame's camera rays, block after block, row by row inside a block: the samples hj_render_aovs_frame walks
from oracle import hj_oracle  # noqa: E402  (the camera's rays, as the renderer makes them)
blocks = host.make_blocks(a.size, a.size, a.spp, a.seed)
pix = []
for b in blocks:
    ly, lx = np.mgrid[0:b.dimension[1], 0:b.dimension[0]]
    pix.append(np.stack([lx.ravel() + b.origin[0] + b.sample_offset[0], ly.ravel() + b.origin[1] + b.sample_offset[1]], 1).astype(np.float32))
pix = np.concatenate(pix)
cam = np.zeros((len(pix), 8), np.float32)
cam[:, 0:6] = hj_oracle.camera_rays(cs.desc.camera, a.size, a.size, pix)
cam[:, 6], cam[:, 7] = 1e-4, np.inf
rays = torch.from_numpy(cam).to(dev)
del cam, pix

calls = {"render_aovs_frame": lambda: r.render_aovs(a.size, a.size, spp=a.spp, master_seed=a.seed, device=True),
         "trace_rays+surface": lambda: r.trace_rays(rays, surface=True)}
out = {k: f() for k, f in calls.items()}                                # (the warm-up)
hits_fused = int(out["render_aovs_frame"][..., 11].sum().item())
hits_rays = int((out["trace_rays+surface"][0] >= 0).sum().item())
del out
ms = {k: [] for k in calls}
for _ in range(a.rounds):
    for k, f in calls.items():
        t = time.perf_counter()
        f()
        ms[k].append((time.perf_counter() - t) * 1e3)
print(f"{a.scene}: {cs.num_shapes} shapes, {a.size} x {a.size} x {a.spp} spp = {len(rays)} camera rays in {len(blocks)} blocks; "
      f"hits {hits_fused} (fused) / {hits_rays} (ray array); {a.rounds} interleaved rounds after one warm-up")
base = statistics.median(ms["trace_rays+surface"])
for k, t in ms.items():
    print(f"{a.scene} {k}: {statistics.median(t):.2f} ({min(t):.2f} ... {max(t):.2f}) ms, {statistics.median(t) / base:.2f} x trace_rays+surface")
r.close()
