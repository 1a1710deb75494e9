"""What a ray query costs: hj_trace_rays on caller-supplied rays that stay on the device (HJ_TRACE_DEVICE_ARRAYS, torch tensors), the
persistent kernel form against the plain one (HJ_TRACE_PERSISTENT = 1 / 0: one context each, created under its setting), closest
hit and any-hit, on two ray sets:

    (a) the primary rays of a --size x --size camera (pixel centres; coherent),
    (b) one generation of incoherent rays built in torch from (a)'s own surface records: from p + 2e-4 n into a seeded random
        direction in the hemisphere of n, one per primary ray that hit.

Interleaved pairs (persistent, plain, persistent, ...), --pairs of them after a warm-up of each, Mrays/s lowest ... highest of each
form - so that the scatter can be read beside the effect.  A call's time is a host clock around it (it returns after its stream
synchronise) and includes the launch.  Under each scene, for scale: the renderer's own rays per second on it (closest-hit + shadow rays
of a frame over its wall time).  The closest-hit results of both forms are compared bit for bit on the way.  One scene per process,
each under its own time limit, chained:

    timeout -k 10 300 python tools/ray_query_cost.py --scene cbox && timeout -k 10 420 python tools/ray_query_cost.py --scene mesh
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
ap.add_argument("--scene", choices=["cbox", "mesh"], default="cbox", help="cbox: c2's scene; mesh: c4's 1 M triangles")
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--pairs", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()

kind, tris, spp = (host.SYNTH_CBOX, 0, 64) if a.scene == "cbox" else (host.SYNTH_CBOX_MESH, 1000000, 16)
t0 = time.perf_counter()
cs = host.Scene.synthetic(kind, mesh_triangles=tris).compile()
print(f"{a.scene}: {cs.num_shapes} shapes, host compile {time.perf_counter() - t0:.2f} s")


def context(persistent):
    os.environ["HJ_TRACE_PERSISTENT"] = persistent
    try:
        r = device.Renderer(0)
        r.upload_scene(cs)                                              # (an upload reads the switches again)
    finally:
        del os.environ["HJ_TRACE_PERSISTENT"]
    return r


forms = {"persistent": context("1"), "plain": context("0")}
dev = torch.device("cuda", 0)

from oracle import hj_oracle  # noqa: E402  (the camera's rays, as the renderer makes them for pixel centres)
ys, xs = np.mgrid[0:a.size, 0:a.size]
pix = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
cam = np.zeros((len(pix), 8), np.float32)
cam[:, 0:6] = hj_oracle.camera_rays(cs.desc.camera, a.size, a.size, pix)
cam[:, 6], cam[:, 7] = 1e-4, np.inf
primary = torch.from_numpy(cam).to(dev)

ids, _, _, _, surf = forms["persistent"].trace_rays(primary, surface=True)
hit = ids >= 0
p, n = surf[hit, 0:3], surf[hit, 3:6]
g = torch.Generator(device=dev)
g.manual_seed(a.seed)
d = torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32)
d = d / d.norm(dim=1, keepdim=True)
d = torch.where((d * n).sum(dim=1, keepdim=True) < 0, -d, d)
bounce = torch.zeros((p.shape[0], 8), device=dev, dtype=torch.float32)
bounce[:, 0:3], bounce[:, 3:6], bounce[:, 6], bounce[:, 7] = p + 2e-4 * n, d, 0.0, float("inf")
bounce = bounce.contiguous()
print(f"{a.scene}: (a) {len(primary)} primary rays, {int(hit.sum())} hit; (b) {len(bounce)} incoherent rays from their surface records")

for label, rays in (("(a) primary", primary), ("(b) incoherent", bounce)):
    for any_hit in (False, True):
        out = {k: r.trace_rays(rays, any_hit=any_hit) for k, r in forms.items()}            # warm-up of both, and the comparison
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out["persistent"], out["plain"]))
        hits = int((out["persistent"][0] >= 0).sum())
        rate = {k: [] for k in forms}
        for _ in range(a.pairs):
            for k, r in forms.items():
                t = time.perf_counter()
                r.trace_rays(rays, any_hit=any_hit)
                rate[k].append(len(rays) / (time.perf_counter() - t) / 1e6)
        print(f"{a.scene} {label}, {'any-hit' if any_hit else 'closest hit'}: {len(rays)} rays, {hits} hit, both forms the same bits: {same}; "
              f"{a.pairs} interleaved pairs, Mrays/s lowest ... highest: "
              + ", ".join(f"{k} {min(v):.0f} ... {max(v):.0f}" for k, v in rate.items())
              + f"; persistent / plain (highest) {max(rate['persistent']) / max(rate['plain']):.2f}")

r = forms["persistent"]
r.create_framebuffer(1024, 1024)
r.render_frame(spp, 1)
best = 0.0
for _ in range(3):
    r.clear()
    t = time.perf_counter()
    st = r.render_frame(spp, 1)
    best = max(best, (st["closest_rays"] + st["shadow_rays"]) / (time.perf_counter() - t) / 1e6)
print(f"{a.scene}: for scale, the renderer's own frame (1024 x 1024 x {spp}): {best:.0f} Mrays/s (closest-hit + shadow rays over wall time, best of 3)")
for r in forms.values():
    r.close()
