"""What a gather query saves: hj_trace_irradiance beside the route a caller had before it, on one box, interleaved.

Scene: the cbox.  Points: --points surface points (first hits of camera rays, hj_trace_rays' surface records, lifted 2e-4 along the
normal) at --spp samples each, in two modes: hemisphere, and sphere + SH9.

    gather   Renderer.trace_irradiance on the point tensor (HJ_GATHER_DEVICE_ARRAYS): directions, paths and reduction on the device
    route    what a caller did before: points x spp directions drawn in torch (its RNG, cosine or uniform), one ray per sample,
             hj_trace_paths at spp = 1 on the device, then the reduction in torch (sums, hit count, nearest hit; the nine
             SH-weighted sums in SH9 mode) - through --parent-lib (a libhijiki_hip.so built from the parent commit, loaded beside
             this one, its entry points declared here by hand); without it: through this library

--pairs interleaved runs of (gather, route) per mode after a warm-up of each; a run's time is a host clock between two device
synchronisations; Mpaths/s and ms, lowest ... highest.  No threshold is set: the table belongs in DESIGN.md ("Gather queries"), the
raw output in profiles/ (--out).  Run under its own time limit:

    timeout -k 10 600 python tools/gather_cost.py --parent-lib PATH --out profiles/gather_cost_cbox.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)
from hijiki_amd import abi, device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1 << 16)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--pairs", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--parent-lib", default="", help="libhijiki_hip.so of the parent commit for the route's hj_trace_paths")
ap.add_argument("--out", default="", help="append the run to this file")
a = ap.parse_args()

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


class ParentRoute:
    """hj_trace_paths through ANOTHER libhijiki_hip.so (the parent commit's): the entry points it needs, declared here by hand."""

    def __init__(self, path, compiled):
        vp, L = C.c_void_p, C.CDLL(path)
        L.hj_context_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.hj_context_destroy.argtypes = [vp]
        L.hj_context_destroy.restype = None
        L.hj_last_error.argtypes = [vp]
        L.hj_last_error.restype = C.c_char_p
        L.hj_scene_upload.argtypes = [vp, C.POINTER(abi.SceneDesc)]
        L.hj_trace_paths.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.POINTER(abi.RenderOpts), C.c_uint32, vp, C.POINTER(abi.RenderStats)]
        if hasattr(L, "hj_trace_irradiance"):
            raise SystemExit(f"{path} exports hj_trace_irradiance: it is not the parent commit's library")
        self.L, self._h = L, vp()
        self._check(L.hj_context_create(0, C.byref(self._h)))
        self._check(L.hj_scene_upload(self._h, C.byref(compiled.desc)))

    def _check(self, rc):
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, (self.L.hj_last_error(self._h) or b"").decode())

    def trace_paths(self, rays, spp=1):
        out = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()
        self._check(self.L.hj_trace_paths(self._h, rays.data_ptr(), rays.shape[0], spp, None, abi.PATHS_DEVICE_ARRAYS, out.data_ptr(), None))
        return out

    def close(self):
        self.L.hj_context_destroy(self._h)


cs = host.Scene.synthetic(host.SYNTH_CBOX).compile()
dev = torch.device("cuda", 0)
r = device.Renderer(0)
r.upload_scene(cs)
parent = ParentRoute(a.parent_lib, cs) if a.parent_lib else r

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
nrm = surf[hit, 3:6].contiguous()
pts = torch.zeros((a.points, 8), device=dev, dtype=torch.float32)
pts[:, 0:3], pts[:, 3:6] = surf[hit, 0:3] + 2e-4 * nrm, nrm
seeds = np.random.default_rng(a.seed).integers(0, 1 << 31, a.points, dtype=np.int64).astype(np.int32)
pts.view(torch.int32)[:, 6] = torch.from_numpy(seeds).to(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(a.seed)
M = a.points * a.spp
say(f"cbox: {a.points} surface points x {a.spp} spp = {M} paths a run; the route's hj_trace_paths through "
    f"{'the parent library ' + a.parent_lib if a.parent_lib else 'THIS library'}")


def gather(sphere):
    return r.trace_irradiance(pts, spp=a.spp, sphere=sphere, sh9=sphere)


def route(sphere):
    """The caller's route before hj_trace_irradiance.  Deliberately NOT the contract: torch's RNG and trigonometry, decimal SH
    constants and torch's own operation order - what a caller would have written; only its cost is compared, never its bits."""
    u, v = torch.rand(M, generator=gen, device=dev), torch.rand(M, generator=gen, device=dev) * (2 * np.pi)
    nn = nrm.repeat_interleave(a.spp, dim=0)
    if sphere:
        z = 2 * u - 1
        rad = torch.sqrt(torch.clamp(1 - z * z, min=0))
        d = torch.stack([rad * torch.cos(v), rad * torch.sin(v), z], 1)
    else:
        bt = torch.where((nn[:, 0].abs() > nn[:, 1].abs())[:, None], torch.tensor([0.0, 1.0, 0.0], device=dev), torch.tensor([1.0, 0.0, 0.0], device=dev))
        t = torch.nn.functional.normalize(torch.linalg.cross(nn, bt), dim=1)
        b = torch.linalg.cross(nn, t)
        rad = torch.sqrt(u)
        d = t * (rad * torch.cos(v))[:, None] + b * (rad * torch.sin(v))[:, None] + nn * torch.sqrt(torch.clamp(1 - u, min=0))[:, None]
    rays = torch.zeros((M, 8), device=dev, dtype=torch.float32)
    rays[:, 0:3], rays[:, 3:6] = pts[:, 0:3].repeat_interleave(a.spp, dim=0), d
    rays.view(torch.int32)[:, 6] = torch.arange(M, device=dev, dtype=torch.int32)
    smp = parent.trace_paths(rays, spp=1).view(a.points, a.spp, 8)
    L, t_hit = smp[:, :, 0:3], smp[:, :, 7]
    out = [L.sum(1), (t_hit > 0).sum(1), torch.where(t_hit > 0, t_hit, torch.inf).amin(1)]
    if sphere:
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        Y = torch.stack([torch.full_like(x, 0.28209479), 0.48860252 * y, 0.48860252 * z, 0.48860252 * x, 1.0925485 * x * y, 1.0925485 * y * z,
                         0.31539157 * (3 * z * z - 1), 1.0925485 * x * z, 0.54627424 * (x * x - y * y)], 1).view(a.points, a.spp, 9)
        out.append(torch.einsum("psj,psc->pjc", Y, L))
    return out


def timed(f, sphere):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    f(sphere)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t


def spread(v, scale=1.0, fmt="{:.1f}"):
    return f"{fmt.format(min(v) * scale)} ... {fmt.format(max(v) * scale)}"


for mode, sphere in (("hemisphere", False), ("sphere + SH9", True)):
    runs = {"gather": gather, "route": route}
    for f in runs.values():                                             # warm-up of each (allocations, first launches)
        f(sphere)
    secs = {k: [] for k in runs}
    for _ in range(a.pairs):
        for k, f in runs.items():
            secs[k].append(timed(f, sphere))
    say(f"{mode}: {a.pairs} interleaved runs, lowest ... highest")
    for k, v in secs.items():
        say(f"  {k}: {spread(v, 1e3, '{:.2f}')} ms, {spread([M / s for s in v], 1e-6)} Mpaths/s")
    say(f"  time, route / gather, best of each: {min(secs['route']) / min(secs['gather']):.2f}")
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
if parent is not r:
    parent.close()
r.close()
