"""What adaptive sampling costs and buys: hj_trace_paths_adaptive beside hj_trace_paths on rays that stay on the device (torch
tensors), on one box, interleaved.  The rays are one generation of incoherent rays built in torch from trace_rays' surface records of
a --size x --size camera grid (from p + 2e-4 n into a seeded random direction in the hemisphere of n), repeated with other seeds up
to --rays rays.

    (a) the cost of the rounds themselves: adaptive at rel_error = 0, floor = 0 and 4 / +4 / 16 - only rays whose samples have no
        variance at all stop before 16 - beside hj_trace_paths(spp = 16) through --parent-lib (a libhijiki_hip.so built from the
        parent commit, loaded beside this one; without it: through this library).  Both are reported as paths/s, the adaptive run
        with the paths it really traced, so the difference is accumulate, compaction and the per-round synchronisation.
    (b) equal-budget error: adaptive at rel_error 0.1 / 0.25 / 0.5 (--spp-min / --spp-step / --spp-max): mean n_i, time, paths/s,
        and on the first --rmse-rays rays the RMSE of rgb / n_i against a uniform query of --ref-spp samples (seeds far from the
        runs'), beside a uniform query at the nearest equal number of samples per ray.

--pairs interleaved runs of each after a warm-up of each; lowest ... highest.  A call's time is a host clock around it (each returns
when its results are complete).  The table belongs in DESIGN.md ("Adaptive path queries"), the raw output in profiles/ (--out).  Run
under its own time limit:

    timeout -k 10 600 python tools/path_adaptive_cost.py --scene cbox --out profiles/path_adaptive_cost_cbox.txt
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
ap.add_argument("--scene", choices=["cbox", "mesh"], default="cbox", help="mesh: 1 M triangles")
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--rays", type=int, default=1 << 20)
ap.add_argument("--pairs", type=int, default=9)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--spp-min", type=int, default=4)
ap.add_argument("--spp-step", type=int, default=4)
ap.add_argument("--spp-max", type=int, default=64)
ap.add_argument("--rel-errors", default="0.1,0.25,0.5")
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--rmse-rays", type=int, default=1 << 16)
ap.add_argument("--parent-lib", default="", help="libhijiki_hip.so of the parent commit for (a)'s uniform query")
ap.add_argument("--out", default="", help="append the run to this file")
a = ap.parse_args()

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


class ParentQuery:
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
        if hasattr(L, "hj_trace_paths_adaptive"):
            raise SystemExit(f"{path} exports hj_trace_paths_adaptive: it is not the parent commit's library")
        self.L, self._h = L, vp()
        self._check(L.hj_context_create(0, C.byref(self._h)))
        self._check(L.hj_scene_upload(self._h, C.byref(compiled.desc)))

    def _check(self, rc):
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, (self.L.hj_last_error(self._h) or b"").decode())

    def trace_paths(self, rays, spp, stats=True):
        out = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
        st = abi.RenderStats()
        torch.cuda.current_stream(rays.device).synchronize()
        self._check(self.L.hj_trace_paths(self._h, rays.data_ptr(), rays.shape[0], spp, None, abi.PATHS_DEVICE_ARRAYS, out.data_ptr(), C.byref(st)))
        return out, device.stats_dict(st)

    def close(self):
        self.L.hj_context_destroy(self._h)


dev = torch.device("cuda", 0)
r = device.Renderer(0)
if a.scene == "mesh":
    cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=1000000).compile(with_tree=False)
    cs.set_bvh(r.build_bvh(cs))
else:
    cs = host.Scene.synthetic(host.SYNTH_CBOX).compile()
r.upload_scene(cs)
parent = ParentQuery(a.parent_lib, cs) if a.parent_lib else r

from oracle import hj_oracle  # noqa: E402  (the camera's rays, as the renderer makes them for pixel centres)
ys, xs = np.mgrid[0:a.size, 0:a.size]
pix = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
cam = np.zeros((len(pix), 8), np.float32)
cam[:, 0:6] = hj_oracle.camera_rays(cs.desc.camera, a.size, a.size, pix)
probe = torch.from_numpy(cam).to(dev)
probe[:, 6], probe[:, 7] = 1e-4, float("inf")
ids, _, _, _, surf = r.trace_rays(probe, surface=True)
hit = ids >= 0
p, n = surf[hit, 0:3], surf[hit, 3:6]
reps = -(-a.rays // p.shape[0])
p, n = p.repeat(reps, 1)[:a.rays], n.repeat(reps, 1)[:a.rays]
g = torch.Generator(device=dev)
g.manual_seed(a.seed)
d = torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32)
d = d / d.norm(dim=1, keepdim=True)
d = torch.where((d * n).sum(dim=1, keepdim=True) < 0, -d, d)
rays = torch.zeros((p.shape[0], 8), device=dev, dtype=torch.float32)
rays[:, 0:3], rays[:, 3:6] = p + 2e-4 * n, d
rays.view(torch.int32)[:, 6] = torch.randint(-(1 << 31), 1 << 31, (p.shape[0],), generator=g, device=dev, dtype=torch.int64).to(torch.int32)
rays = rays.contiguous()
N = rays.shape[0]
say(f"{a.scene}: {cs.num_shapes} shapes, {N} incoherent rays from the surface records of a {a.size} x {a.size} camera grid; "
    f"(a)'s uniform query through {'the parent library ' + a.parent_lib if a.parent_lib else 'THIS library'}")


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def spread(v, scale=1.0, fmt="{:.1f}"):
    return f"{fmt.format(min(v) * scale)} ... {fmt.format(max(v) * scale)}"


# ---------------------------------------------------------------------------------------------------- (a) the rounds' own cost
KW0 = dict(spp_min=4, spp_step=4, spp_max=16, rel_error=0.0, floor=0.0)
runs = {"adaptive 4 / +4 / 16, rel_error 0": lambda: r.trace_paths_adaptive(rays, stats=True, **KW0)[1],
        "hj_trace_paths(spp = 16)": lambda: parent.trace_paths(rays, spp=16, stats=True)[1]}
stats = {k: f() for k, f in runs.items()}                                # warm-up of each (allocations, first launches)
secs = {k: [] for k in runs}
for _ in range(a.pairs):
    for k, f in runs.items():
        secs[k].append(timed(f)[0])
say(f"(a) {a.pairs} interleaved runs, lowest ... highest")
for k, v in secs.items():
    st = stats[k]
    say(f"  {k}: {st['paths']} paths ({st['paths'] / N:.2f} a ray), {st['batches']} launches, {st['bounce_rounds']} rounds; "
        f"{spread(v, 1e3)} ms, {spread([st['paths'] / s for s in v], 1e-6)} Mpaths/s")
ka, kb = list(secs)
say(f"  paths/s, adaptive / uniform, best of each: {(stats[ka]['paths'] / min(secs[ka])) / (stats[kb]['paths'] / min(secs[kb])):.3f}")

# ---------------------------------------------------------------------------------------------------- (b) equal-budget error
M = min(a.rmse_rays, N)
sub = rays[:M].contiguous()
far = sub.clone()
far.view(torch.int32)[:, 6] += 0x40000000                               # the reference's samples are not the runs' (int32 wrap-around)
ref = torch.zeros((M, 3), device=dev, dtype=torch.float64)
left, at = a.ref_spp, 0
while left:                                                             # (in calls of at most 1024 samples a ray)
    c = min(left, 1024)
    part = far.clone()
    part.view(torch.int32)[:, 6] += at
    ref += r.trace_paths(part, spp=c)[:, 0:3].double()
    left, at = left - c, at + c
ref /= a.ref_spp


def rmse(rec):
    return float(((rec[:M, 0:3].double() / rec[:M, 3:4].double() - ref) ** 2).mean().sqrt())


say(f"(b) rounds {a.spp_min} / +{a.spp_step} / {a.spp_max}, floor 0.01; RMSE of rgb on the first {M} rays against {a.ref_spp} spp; {a.pairs} runs each")
for rel in [float(x) for x in a.rel_errors.split(",")]:
    kw = dict(spp_min=a.spp_min, spp_step=a.spp_step, spp_max=a.spp_max, rel_error=rel, floor=0.01)
    rec, st = r.trace_paths_adaptive(rays, stats=True, **kw)
    mean_n = st["paths"] / N
    spp_u = max(1, round(mean_n))
    rec_u, st_u = r.trace_paths(rays, spp=spp_u, stats=True)
    ta, tu = [], []
    for _ in range(a.pairs):
        ta.append(timed(lambda: r.trace_paths_adaptive(rays, **kw))[0])
        tu.append(timed(lambda: r.trace_paths(rays, spp=spp_u))[0])
    say(f"  rel_error {rel}: mean n_i {mean_n:.2f}, {st['bounce_rounds']} rounds, {st['batches']} launches; {spread(ta, 1e3)} ms, "
        f"{spread([st['paths'] / s for s in ta], 1e-6)} Mpaths/s, RMSE {rmse(rec):.5f}")
    say(f"    uniform spp {spp_u}: {spread(tu, 1e3)} ms, {spread([st_u['paths'] / s for s in tu], 1e-6)} Mpaths/s, RMSE {rmse(rec_u):.5f}")
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
if parent is not r:
    parent.close()
r.close()
