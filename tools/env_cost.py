"""What environment lighting costs: Mpaths/s of the synthetic cbox (its front is open, so rays leave it) under a 2048 x 1024 lat-long
environment (bilinear, select_prob 0.5: half of the next-event samples go to the sky), next to the same scene without one.

    python tools/env_cost.py [--spp 512] [--size 1024] [--reps 3] [--env-w 2048]

The environment is a sky gradient with a sun and noise, so that its alias table is not uniform.  Best frame of --reps per variant,
variants interleaved twice; the same tree for both."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hijiki_amd import abi, device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=512)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--env-w", type=int, default=2048)
a = ap.parse_args()

W, H = a.env_w, a.env_w // 2
rng = np.random.default_rng(1)
y = (np.arange(H) + 0.5) / H
sky = np.zeros((H, W, 4), np.float32)
sky[..., 0] = np.where(y < 0.5, 0.3 + 0.6 * (0.5 - y), 0.05)[:, None]
sky[..., 1] = np.where(y < 0.5, 0.4 + 0.7 * (0.5 - y), 0.05)[:, None]
sky[..., 2] = np.where(y < 0.5, 0.7 + 1.0 * (0.5 - y), 0.05)[:, None]
sky[..., :3] *= rng.uniform(0.8, 1.2, (H, W, 1)).astype(np.float32)
sky[H // 6:H // 6 + 4, W // 3:W // 3 + 4, :3] = 500.0


def scene(with_env):
    s = host.Scene.synthetic(host.SYNTH_CBOX)
    if with_env:
        s.set_environment(s.add_texture(sky, abi.TEX_BILINEAR), 1.0, 0.5)
    return s.compile()


plain = scene(False)
variants = {"no environment": plain, "environment": scene(True)}
variants["environment"].set_bvh(plain.bvh)                # one tree for both
r = device.Renderer(0)
best = {k: 0.0 for k in variants}
for _ in range(2):
    for name, cs in variants.items():
        r.upload_scene(cs)
        r.create_framebuffer(a.size, a.size)
        o = device.default_opts()
        r.reserve(a.spp * host.blocks_per_pass(a.size, a.size), o)
        r.render_frame(1, 1, opts=o)                       # warm-up
        for _ in range(a.reps):
            r.clear()
            t = time.perf_counter()
            r.render_frame(a.spp, 1, opts=o)
            dt = time.perf_counter() - t
            best[name] = max(best[name], a.size * a.size * a.spp / dt / 1e6)
for name, v in best.items():
    print(f"{name:15s} {a.size}x{a.size}x{a.spp}, {W}x{H} environment: {v:8.1f} Mpaths/s  ({100.0 * (v / best['no environment'] - 1):+.1f} %)")
r.close()
