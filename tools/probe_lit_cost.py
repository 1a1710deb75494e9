"""What hj_render_probe_lit costs, and how far a probe-lit frame is from a converged path-traced one.

On the box with the spheres at --size x --size (1024), 1 spp, into a device tensor, the volume on the device: the milliseconds of
hj_render_aovs_frame_followed and of hj_render_probe_lit_frame at max_follow 0, 2 and 8 - per max_follow the plain, the visible and
the placed look-up -, all calls interleaved round by round so that a drift of the machine falls on all of them.  One warm-up call
each, then the median (min ... max) of --rounds rounds; a call's time is a host clock around it (it returns after its stream
synchronise).

The volume: --grid probes a side over the middle 80 % of the scene's box, hj_bake_probes at --bake-spp, the atlas at res 8, placed
by 4 hj_place_probes steps.  The error: the resolved frame at --spp samples (4) and max_follow 8 against hj_render_frame of the same
scene at --truth-spp (1024) - root mean square over all pixels and channels, beside the truth's mean, per look-up.  Neither figure has
a threshold: they go into profiles/NOTES.md as measured.

    timeout -k 10 600 python tools/probe_lit_cost.py
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
from hijiki_amd import abi, device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--grid", type=int, default=8)
ap.add_argument("--bake-spp", type=int, default=1024)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--truth-spp", type=int, default=1024)
a = ap.parse_args()

r = device.Renderer(0)
cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile()
r.upload_scene(cs)
N = a.size
box = cs.bvh_f32
lo, hi = np.array(box[0, 0:3], np.float64), np.array(box[0, 4:7], np.float64)
count = (a.grid,) * 3
origin = lo + 0.1 * (hi - lo)
spacing = 0.8 * (hi - lo) / (a.grid - 1)

t0 = time.perf_counter()
vol = r.bake_probes(origin, spacing, count, a.bake_spp, min_distance=0.02, seed=1, device=True)
atlas = r.bake_probe_visibility(origin, spacing, count, res=8, rays_per_texel=16, max_distance=float(np.linalg.norm(spacing)) * 1.5, seed=2, device=True)
desc = dict(origin=origin, spacing=spacing, count=count, seed=3)
vis = dict(res=8, rays_per_texel=16, max_distance=float(np.linalg.norm(spacing)) * 1.5)
place = r.new_placement(count, device=torch.device("cuda", r.device))
for frame in range(4):
    r.place_probes(desc, vis, place, frame=frame, min_front_distance=0.2 * float(spacing.min()))
asleep = int((place.cpu().numpy().view(np.uint32)[..., 3] != 0).sum())
print(f"volume: {a.grid}^3 probes, bake {a.bake_spp} spp, atlas res 8, {asleep} probes asleep; baked and placed in {time.perf_counter() - t0:.2f} s")

LOOKS = {"plain": dict(), "visible": dict(atlas=atlas, normal_bias=0.02), "placed": dict(atlas=atlas, placement=place, normal_bias=0.02)}


def lit(kind, follow, spp=1):
    return r.render_probe_lit(vol, origin, spacing, N, N, spp=spp, master_seed=7, follow=follow, **LOOKS[kind])


calls = {}
for follow in (0, 2, 8):
    calls[f"hj_render_aovs_frame_followed, max_follow {follow}"] = lambda f=follow: r.render_aovs(N, N, spp=1, master_seed=7, follow=f, device=True)
    for kind in LOOKS:
        calls[f"hj_render_probe_lit_frame, {kind}, max_follow {follow}"] = lambda f=follow, k=kind: lit(k, f)
times = {k: [] for k in calls}
for fn in calls.values():
    fn()
for _ in range(a.rounds):
    for k, fn in calls.items():
        t = time.perf_counter()
        fn()
        times[k].append((time.perf_counter() - t) * 1e3)
print(f"{N} x {N}, 1 spp, device arrays, median (min ... max) of {a.rounds} rounds, ms:")
for k, v in times.items():
    print(f"  {k:58s} {statistics.median(v):7.3f} ({min(v):.3f} ... {max(v):.3f})")

r.create_framebuffer(N, N)
r.clear()
o = abi.RenderOpts.default()
r.render_frame(a.truth_spp, 99, opts=o)
truth = r.resolve().astype(np.float64)
print(f"against hj_render_frame at {a.truth_spp} spp (mean {truth.mean():.4f}), the resolved frame at {a.spp} spp, max_follow 8:")
for kind in LOOKS:
    got = device.resolve_probe_lit(lit(kind, 8, a.spp)).cpu().numpy().astype(np.float64)
    diff = got - truth
    print(f"  {kind:8s} RMS error {np.sqrt((diff ** 2).mean()):.4f}, mean signed {diff.mean():+.4f}, RMS over pixels with truth < 1 {np.sqrt((diff[truth.max(2) < 1] ** 2).mean()):.4f}")
r.close()
