"""What the probe look-up saves, and what the bake adds to its gather: hj_sample_probes beside the route a caller had before it, and
hj_bake_probes beside its gather alone, on one box, interleaved.

Scene: the cbox.  Volume: --grid^3 probes over the scene's root box, baked at --bake-spp.  Points: --points surface points (first
hits of camera rays, hj_trace_rays' surface records) with their normals.

    sample   Renderer.sample_probes on the device tensors (HJ_PROBES_DEVICE_ARRAYS): one fused kernel
    route    what a caller did before: the same trilinear look-up with validity weights and the SH evaluation written in torch on the
             same tensors - clamp, eight index gathers of 28 words, weighted sums, division, basis, dot products.  Its operation
             order is torch's; its result is compared with the kernel's only to a tolerance, and printed
    bake     Renderer.bake_probes(device=True) at --spp
    gather   its parts as separate calls: probe_points(device=True), then trace_irradiance(sphere, sh9) on them - the bake without
             its resolve (the difference of the two is the resolve, with the second synchronisation it brings)

--pairs interleaved runs of each pair after a warm-up; a look-up run is --reps calls back to back between two device
synchronisations (every call ends in one of its own), a bake run is one call; a run's time is a host clock; ms a call, lowest ...
highest.  No threshold is set: the table belongs in DESIGN.md ("Probe volumes"), the raw output in profiles/ (--out).  Run under its
own time limit:

    timeout -k 10 600 python tools/probe_cost.py --out profiles/probe_cost_mi355x.txt
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
ap.add_argument("--points", type=int, default=1 << 20)
ap.add_argument("--grid", type=int, default=32)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bake-spp", type=int, default=16)
ap.add_argument("--pairs", type=int, default=9)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default="", help="append the run to this file")
a = ap.parse_args()

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


cs = host.Scene.synthetic(host.SYNTH_CBOX).compile()
dev = torch.device("cuda", 0)
r = device.Renderer(0)
r.upload_scene(cs)

from oracle import hj_oracle  # noqa: E402  (the camera's rays, as the renderer makes them for pixel centres)
side = int(np.ceil(np.sqrt(2 * a.points)))
ys, xs = np.mgrid[0:side, 0:side]
pix = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
cam = np.zeros((len(pix), 8), np.float32)
cam[:, 0:6] = hj_oracle.camera_rays(cs.desc.camera, side, side, pix)
cam[:, 6], cam[:, 7] = 1e-4, np.inf
ids, _, _, _, surf = r.trace_rays(torch.from_numpy(cam).to(dev), surface=True)
hit = torch.nonzero(ids >= 0).flatten()[:a.points]
if len(hit) != a.points:
    raise SystemExit(f"only {len(hit)} of {a.points} surface points from a {side} x {side} camera grid")
pts = torch.zeros((a.points, 8), device=dev, dtype=torch.float32)
pts[:, 0:3], pts[:, 3:6] = surf[hit, 0:3], surf[hit, 3:6]

root = cs.bvh_f32[0]
lo, hi = root[0:3].astype(np.float64), root[4:7].astype(np.float64)
G = a.grid
origin = (lo + 0.02 * (hi - lo)).astype(np.float32)
spacing = (0.96 * (hi - lo) / max(G - 1, 1)).astype(np.float32)
grid = dict(origin=origin, spacing=spacing, count=(G, G, G))
vol = r.bake_probes(**grid, spp=a.bake_spp, min_distance=0.5 * float(spacing.min()), device=True)
valid = float((vol[..., 27] == 1).float().mean())
say(f"cbox: {a.points} surface points against {G}^3 probes ({vol.numel() * 4 / 2**20:.1f} MiB, {100 * valid:.1f} % valid, baked at {a.bake_spp} spp); "
    f"{a.reps} look-ups a run; the bake at {a.spp} spp = {G ** 3 * a.spp} paths")


def sample():
    return r.sample_probes(vol, origin, spacing, pts)


t_origin, t_spacing = torch.from_numpy(origin).to(dev), torch.from_numpy(spacing).to(dev)
t_m = torch.tensor([G - 1] * 3, device=dev, dtype=torch.float32)


def route():
    """The caller's route before hj_sample_probes: the same look-up in torch, its own operation order."""
    flat = vol.view(-1, 28)
    g = torch.minimum(torch.clamp(torch.nan_to_num((pts[:, 0:3] - t_origin) / t_spacing, nan=0.0), min=0.0), t_m)
    i0 = torch.clamp(g.to(torch.int64), max=max(G - 2, 0))
    f = g - i0.to(torch.float32)
    i1 = torch.clamp(i0 + 1, max=G - 1)
    idx, w = (i0, i1), (1.0 - f, f)
    acc = torch.zeros((pts.shape[0], 27), device=dev)
    wsum = torch.zeros(pts.shape[0], device=dev)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                q = (idx[dz][:, 2] * G + idx[dy][:, 1]) * G + idx[dx][:, 0]
                rec = flat[q]
                wt = w[dx][:, 0] * w[dy][:, 1] * w[dz][:, 2] * rec[:, 27]
                acc = acc + torch.where((wt != 0)[:, None], rec[:, 0:27] * wt[:, None], 0.0)
                wsum = wsum + wt
    n = torch.nn.functional.normalize(pts[:, 3:6], dim=1)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    Y = torch.stack([torch.full_like(x, 0.28209479), 0.48860252 * y, 0.48860252 * z, 0.48860252 * x, 1.0925485 * x * y, 1.0925485 * y * z,
                     0.31539157 * (3 * z * z - 1), 1.0925485 * x * z, 0.54627424 * (x * x - y * y)], 1)
    c = (acc / torch.where(wsum == 0, 1.0, wsum)[:, None]).view(-1, 9, 3)
    e = torch.einsum("pjc,pj->pc", c, Y)
    return torch.cat([torch.where((wsum == 0)[:, None], 0.0, e), wsum[:, None]], 1)


def bake():
    return r.bake_probes(**grid, spp=a.spp, device=True)


def gather():
    p = r.probe_points(**grid, device=True)
    return r.trace_irradiance(p, spp=a.spp, sphere=True, sh9=True)


def timed(f, reps):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) / reps


def spread(v, scale=1.0, fmt="{:.3f}"):
    return f"{fmt.format(min(v) * scale)} ... {fmt.format(max(v) * scale)}"


def compare(runs, reps, what, rate=None):
    for f in runs.values():                                             # warm-up of each (allocations, first launches)
        f()
    secs = {k: [] for k in runs}
    for _ in range(a.pairs):
        for k, f in runs.items():
            secs[k].append(timed(f, reps))
    say(f"{what}: {a.pairs} interleaved runs, lowest ... highest")
    for k, v in secs.items():
        say(f"  {k}: {spread(v, 1e3)} ms a call" + (f", {spread([rate / s for s in v], 1e-6, '{:.0f}')} M a second" if rate else ""))
    return secs


got, ref = sample(), route()
ok = torch.isfinite(ref).all(1)
err = float(((got - ref).abs()[ok] / (ref.abs()[ok] + 1e-3)).max())
say(f"route against kernel: largest difference {err:.2e} relative (1e-3 absolute floor) over {int(ok.sum())} points; mean weight {float(got[:, 3].mean()):.3f}")
s = compare({"sample": sample, "route": route}, a.reps, f"look-up, {a.points} points", rate=a.points)
say(f"  time, route / sample, best of each: {min(s['route']) / min(s['sample']):.2f}")
say(f"  bytes the kernel asks of the caches: {a.points * (8 * 112 + 32 + 16) / 2**20:.0f} MiB a call (eight 112-byte records, a point, a result)")
b = compare({"bake": bake, "gather": gather}, 1, f"bake, {G}^3 probes x {a.spp} spp", rate=G ** 3 * a.spp)
say(f"  the resolve and its synchronisation, bake - gather, best of each: {(min(b['bake']) - min(b['gather'])) * 1e3:.3f} ms = "
    f"{100 * (min(b['bake']) - min(b['gather'])) / min(b['bake']):.1f} % of the bake")
p = compare({"points": lambda: r.probe_points(**grid, device=True)}, a.reps, f"point generation alone, {G}^3 probes")
say(f"  point generation, best: {100 * min(p['points']) / min(b['bake']):.1f} % of the bake (a call of its own: launch and synchronisation included)")
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
r.close()
