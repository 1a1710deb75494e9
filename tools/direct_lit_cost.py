"""What hj_render_direct_lit costs beside hj_render_probe_lit, and what traced direct light buys.

On the box with the spheres at --size x --size (1024), into a device tensor, the volume on the device: the milliseconds of
hj_render_probe_lit_frame and of hj_render_direct_lit_frame at the same --spp and max_follow 0, 2 and 8 (the plain look-up; direct-lit
also without a volume), all calls interleaved round by round so that a drift of the machine falls on all of them.  One warm-up call
each, then the median (min ... max) of --rounds rounds; a call's time is a host clock around it (it returns after its stream
synchronise; a direct-lit call synchronises once more a walk launch, for the count of its shadow rays).

The volumes: --grid probes a side over the middle 80 % of the scene's box, hj_bake_probes at --bake-spp, once plain and once with
HJ_PROBES_INDIRECT_ONLY.  The error of three frames at --err-spp samples and max_follow 8 against hj_render_frame of the same scene at
--truth-spp (1024) - root mean square over all pixels and channels, and the mean signed difference, beside the truth's mean:
    probe-lit from the plain volume
    direct-lit from the indirect-only volume
    direct-lit from the plain volume, which counts direct light twice
No figure has a threshold: they go into profiles/NOTES.md as measured.

    timeout -k 10 600 python tools/direct_lit_cost.py
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
ap.add_argument("--spp", type=int, default=1)
ap.add_argument("--err-spp", type=int, default=4)
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
plain = r.bake_probes(origin, spacing, count, a.bake_spp, min_distance=0.02, seed=1, device=True)
indirect = r.bake_probes(origin, spacing, count, a.bake_spp, min_distance=0.02, seed=1, device=True, indirect_only=True)
print(f"volumes: {a.grid}^3 probes, bake {a.bake_spp} spp, plain and indirect-only; baked in {time.perf_counter() - t0:.2f} s; "
      f"mean constant band {plain[..., 0:3].mean().item():.4f} / {indirect[..., 0:3].mean().item():.4f}")


def probe_lit(vol, follow, spp):
    return r.render_probe_lit(vol, origin, spacing, N, N, spp=spp, master_seed=7, follow=follow)


def direct_lit(vol, follow, spp):
    if vol is None:
        return r.render_direct_lit(N, N, spp=spp, master_seed=7, follow=follow, device=True)
    return r.render_direct_lit(N, N, volume=vol, origin=origin, spacing=spacing, spp=spp, master_seed=7, follow=follow)


calls = {}
for follow in (0, 2, 8):
    calls[f"hj_render_probe_lit_frame, plain volume, max_follow {follow}"] = lambda f=follow: probe_lit(plain, f, a.spp)
    calls[f"hj_render_direct_lit_frame, indirect-only volume, max_follow {follow}"] = lambda f=follow: direct_lit(indirect, f, a.spp)
    calls[f"hj_render_direct_lit_frame, no volume, max_follow {follow}"] = lambda f=follow: direct_lit(None, f, a.spp)
times = {k: [] for k in calls}
for fn in calls.values():
    fn()
for _ in range(a.rounds):
    for k, fn in calls.items():
        t = time.perf_counter()
        fn()
        times[k].append((time.perf_counter() - t) * 1e3)
print(f"{N} x {N}, {a.spp} spp, device arrays, median (min ... max) of {a.rounds} rounds, ms:")
for k, v in times.items():
    print(f"  {k:70s} {statistics.median(v):7.3f} ({min(v):.3f} ... {max(v):.3f})")

r.create_framebuffer(N, N)
r.clear()
o = abi.RenderOpts.default()
r.render_frame(a.truth_spp, 99, opts=o)
truth = r.resolve().astype(np.float64)
print(f"against hj_render_frame at {a.truth_spp} spp (mean {truth.mean():.4f}), the resolved frame at {a.err_spp} spp, max_follow 8:")
frames = {"probe-lit, plain volume": lambda: probe_lit(plain, 8, a.err_spp), "direct-lit, indirect-only volume": lambda: direct_lit(indirect, 8, a.err_spp),
          "direct-lit, plain volume (direct light twice)": lambda: direct_lit(plain, 8, a.err_spp)}
for name, fn in frames.items():
    got = device.resolve_probe_lit(fn()).cpu().numpy().astype(np.float64)
    diff = got - truth
    print(f"  {name:48s} RMS error {np.sqrt((diff ** 2).mean()):.4f}, mean signed {diff.mean():+.4f}, RMS over pixels with truth < 1 {np.sqrt((diff[truth.max(2) < 1] ** 2).mean()):.4f}")
r.close()
