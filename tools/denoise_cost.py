"""What hj_denoise_frame costs, and which form of its iteration to take at which step: on arrays that stay on the device (torch
tensors), a fabricated, fully guided --size x --size frame (the denoiser needs no scene),

    temporal:          hj_denoise_frame_temporal at 0 and --iterations iterations in the default form, with a full valid history under
                       a camera shifted by a few pixels and with no history, beside hj_denoise_frame in the same rounds
    denoise_frame:     hj_denoise_frame at 0 ... --iterations iterations, once with every step in the LDS form
                       (HJ_DENOISE_LDS_STEP=128) and once with every step in the direct form (0); the cost of the iteration at step
                       1 << i is the difference between i + 1 and i iterations, the cost of prepare + variance + finish is the row
                       of 0 iterations; and once at --iterations iterations with the switch at its default;
    filter_lightmap:   as a yardstick from existing code, hj_filter_lightmap over a fully guided atlas of the same size at
                       --iterations iterations (40 bytes a staged cell against the denoiser's 48, and no variance passes).

One warm-up call each, then the median (min ... max) of --rounds calls each, interleaved; a call's time is a host clock around it (it
returns after its stream synchronise) and includes its launches and, for the denoiser, torch's allocation of the output.

    timeout -k 10 300 python tools/denoise_cost.py
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
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--iterations", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
N = a.size
dev = torch.device("cuda", 0)

# a frame like a rendered one: 4 samples a pixel, bands of albedo, two normals, a depth ramp with a step, noisy light
rng = np.random.default_rng(7)
y, x = np.mgrid[0:N, 0:N]
albedo = np.stack([0.2 + 0.6 * ((x // 97) % 2), 0.5 + 0.0 * x, 0.8 - 0.5 * ((y // 61) % 2)], -1).astype(np.float32)
normal = np.where((y < N // 3)[..., None], (0.0, 0.6, 0.8), (0.0, 0.0, 1.0)).astype(np.float32)
depth = (3.0 + 0.002 * x + 0.001 * y + np.where(x >= (6 * N) // 10, 2.5, 0.0)).astype(np.float32)
colour = (albedo * (0.5 + 0.3 * np.sin(0.01 * x + 0.02 * y))[..., None] * rng.uniform(0.25, 1.75, (N, N, 3))).astype(np.float32)
aov = np.zeros((N, N, 12), np.float32)
aov[..., 0:3], aov[..., 3] = albedo * 4, 4
aov[..., 4:7], aov[..., 7], aov[..., 11] = normal * 4, depth * 4, 4
beauty = np.concatenate([colour * 4, np.full((N, N, 1), 4, np.float32)], -1)
t_aov, t_beauty = torch.from_numpy(aov).to(dev), torch.from_numpy(beauty).to(dev)

# the yardstick's guide: every texel named by a point (position on a plane, the frame's normal), the frame's colour as the atlas
points = np.zeros((N * N, 8), np.float32)
points[:, 0], points[:, 1], points[:, 2] = x.ravel() / N, y.ravel() / N, depth.ravel()
points[:, 3:6] = normal.reshape(-1, 3)
points.view(np.uint32)[:, 7] = np.arange(N * N, dtype=np.uint32)
t_points = torch.from_numpy(points).to(dev)
t_atlas = torch.from_numpy(np.concatenate([colour, np.ones((N, N, 1), np.float32)], -1)).to(dev)
del aov, beauty, points, colour

made = {}
for form, step in (("lds", "128"), ("direct", "0")):
    os.environ["HJ_DENOISE_LDS_STEP"] = step                             # (read when the context is created)
    made[form] = device.Renderer(0)
os.environ.pop("HJ_DENOISE_LDS_STEP")
made["default"] = device.Renderer(0)
# hj_filter_lightmap's gate wants a scene (the filter reads none).  On a renderer of its own: an upload re-reads the switches from
# the environment, which would put a forced form back to the default.
yard = device.Renderer(0)
yard.upload_scene(host.Scene.synthetic(host.SYNTH_CBOX).compile())

calls = {}
for form, r in made.items():
    for it in ([a.iterations] if form == "default" else range(a.iterations + 1)):
        calls[f"denoise_frame {form} {it} iterations"] = (lambda r=r, it=it: r.denoise_frame(t_aov, t_beauty, it, device=True))
# hj_denoise_frame_temporal beside it: a full valid history (the frame's own, written by a first call) under a camera shifted by a few
# pixels, so that every pixel reads four history taps off its own position; feedback on (one more pass over the history's light)
from hijiki_amd import abi  # noqa: E402
cam, prev = abi.Camera(), abi.Camera()
cam.position[:], cam.rotation[:], cam.fov = (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 60.0
prev.position[:], prev.rotation[:], prev.fov = (0.01, 0.004, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 60.0
t_history = made["default"].denoise_frame_temporal(t_aov, cam, cam, None, t_beauty, 0, device=True)[1]
for it in (0, a.iterations):
    calls[f"temporal default {it} iterations"] = (lambda it=it: made["default"].denoise_frame_temporal(t_aov, cam, prev, t_history, t_beauty, it, device=True))
    calls[f"temporal default {it} iterations, no history"] = (lambda it=it: made["default"].denoise_frame_temporal(t_aov, cam, cam, None, t_beauty, it, device=True))
calls[f"denoise_frame default 0 iterations"] = lambda: made["default"].denoise_frame(t_aov, t_beauty, 0, device=True)
calls[f"filter_lightmap {a.iterations} iterations"] = lambda: yard.filter_lightmap(t_atlas.clone(), t_points, a.iterations, 0.01, 0.5, 0.5, device=True)
calls["(the atlas's clone alone)"] = lambda: (t_atlas.clone(), torch.cuda.synchronize())

first, same = None, True
for k, f in calls.items():                                               # (the warm-up; every form gives the same bits)
    out = f()
    if k.endswith(f"{a.iterations} iterations") and k.startswith("denoise_frame"):
        if first is None:
            first = out
        else:
            same = same and bool((first.view(torch.int32) == out.view(torch.int32)).all().item())
ms = {k: [] for k in calls}
for _ in range(a.rounds):
    for k, f in calls.items():
        t = time.perf_counter()
        f()
        ms[k].append((time.perf_counter() - t) * 1e3)
print(f"{N} x {N}, fully guided; {a.rounds} interleaved rounds after one warm-up; the forms' outputs are bit-identical: {same}")
med = {k: statistics.median(t) for k, t in ms.items()}
for k, t in ms.items():
    print(f"{k}: {med[k]:.3f} ({min(t):.3f} ... {max(t):.3f}) ms")
for it in range(a.iterations):
    lds = med[f"denoise_frame lds {it + 1} iterations"] - med[f"denoise_frame lds {it} iterations"]
    direct = med[f"denoise_frame direct {it + 1} iterations"] - med[f"denoise_frame direct {it} iterations"]
    print(f"the iteration at step {1 << it}: LDS form {lds:.3f} ms, direct form {direct:.3f} ms")
found = made["default"].denoise_frame_temporal(t_aov, cam, prev, t_history, t_beauty, 0, device=True)[1][..., 3]
print(f"temporal: {float((found > 1).float().mean()):.4f} of the pixels found their history under the shifted camera")
for it in (0, a.iterations):
    extra = med[f"temporal default {it} iterations"] - med[f"denoise_frame default {it} iterations"]
    print(f"temporal over denoise_frame at {it} iterations: + {extra:.3f} ms with a history, "
          f"+ {med[f'temporal default {it} iterations, no history'] - med[f'denoise_frame default {it} iterations']:.3f} ms without")
for r in list(made.values()) + [yard]:
    r.close()
