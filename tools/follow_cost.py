"""What the followed AOVs cost, and what they buy the frame denoiser.  A measuring tool, not a test.

    --mode cost:     the milliseconds of hj_render_aovs_frame_followed at --size x --size (1024), one pass, into a device tensor, on the
                     box with the spheres, at max_follow 0, 2 and 8, and of hj_render_aovs_frame beside them.  One warm-up call each,
                     then the median (min ... max) of --rounds calls; a call's time is a host clock around it (it returns after its
                     stream synchronise).  The live chains per round are counted apart from the timing, by alternating
                     hj_follow_specular with hj_trace_rays over the frame's camera rays on the device.
    --mode quality:  the same scene at --size x --size (256) and --spp (4): hj_denoise_frame with default options, guided by
                     hj_render_aovs and by the followed call at --follow (2); the mean squared error of each against a --truth-spp
                     frame, over the pixels whose first hit is the mirror or the glass sphere in every pass, and over the image.

One mode per process, each under its own time limit, chained:

    timeout -k 10 300 python tools/follow_cost.py --mode cost && timeout -k 10 420 python tools/follow_cost.py --mode quality
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime per process)
from hijiki_amd import abi, device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["cost", "quality"], default="cost")
ap.add_argument("--size", type=int, default=0, help="default: 1024 (cost), 256 (quality)")
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--follow", type=int, default=2)
ap.add_argument("--truth-spp", type=int, default=4096)
a = ap.parse_args()

cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile()
r = device.Renderer(0)
r.upload_scene(cs)
tags = cs.materials >> abi.MATERIAL_TAG_SHIFT


def timed(call):
    call()                                                              # (the warm-up)
    ms = []
    for _ in range(a.rounds):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


if a.mode == "cost":
    size = a.size or 1024
    print(f"box with spheres: {cs.num_shapes} shapes, {size} x {size}, 1 pass = {size * size} samples; {a.rounds} rounds after one warm-up")
    ms = timed(lambda: r.render_aovs(size, size, spp=1, master_seed=3, device=True))
    print(f"render_aovs_frame:               {statistics.median(ms):.3f} ({min(ms):.3f} ... {max(ms):.3f}) ms")
    L = device.lib()
    out = torch.empty((size, size, abi.AOV_WORDS), dtype=torch.float32, device=torch.device("cuda", r.device))
    torch.cuda.synchronize()
    for m in (0, 2, 8):
        ms = timed(lambda: r._check(L.hj_render_aovs_frame_followed(r._h, size, size, 1, 3, 0, 1, m, abi.AOV_DEVICE_ARRAY, out.data_ptr())))
        print(f"render_aovs_frame_followed, {m}:   {statistics.median(ms):.3f} ({min(ms):.3f} ... {max(ms):.3f}) ms")
    # the live chains per round: the first hits from the plain image cannot say, so the chain is walked by the public pair
    plain = r.render_aovs(size, size, spp=1, master_seed=3)
    from oracle import hj_oracle as oracle  # noqa: E402  (camera rays only)
    blocks = host.make_blocks(size, size, 1, 3)
    rays = []
    for b in blocks:
        W, H = int(b.dimension[0]), int(b.dimension[1])
        ly, lx = np.mgrid[0:H, 0:W]
        px = np.stack([lx.ravel() + b.origin[0] + b.sample_offset[0], ly.ravel() + b.origin[1] + b.sample_offset[1]], 1).astype(np.float32)
        cam = oracle.camera_rays(cs.desc.camera, size, size, px)
        ray = np.zeros((W * H, 8), np.float32)
        ray[:, 0:6], ray[:, 6], ray[:, 7] = cam[:, 0:6], 1e-4, np.inf
        rays.append(ray)
    cur = torch.from_numpy(np.concatenate(rays)).to(torch.device("cuda", r.device))
    live = []
    for _ in range(8):
        ids, t, u, v = r.trace_rays(cur)
        hits = torch.stack([ids.view(torch.float32), t, u, v], 1).contiguous()
        nxt = r.follow_specular(cur, hits)
        go = nxt[:, 7] > 0                                              # (a continued ray: tMax = +inf; the empty ray: -inf)
        live.append(int(go.sum()))
        if live[-1] == 0:
            break
        cur = nxt[go].contiguous()
    print(f"live chains per round (of {size * size} samples; a round's continuation that hits nothing still counts): {live}")
    assert float(plain[..., 3].sum()) == size * size
else:
    W = H = a.size or 256
    r.create_framebuffer(W, H)
    r.clear()
    r.render_frame(a.truth_spp, 999)
    truth = r.resolve().astype(np.float64)
    r.clear()
    r.render_frame(a.spp, 31)
    beauty = r.read()
    plain = r.render_aovs(W, H, spp=a.spp, master_seed=31)
    followed = r.render_aovs(W, H, spp=a.spp, master_seed=31, follow=a.follow)
    # the pixels whose every sample hits the mirror or the glass sphere first: albedo sum == sample count in all channels, hit count too
    spec = (plain[..., 0:3] == plain[..., 3:4]).all(-1) & (plain[..., 11] == plain[..., 3])
    raw = r.resolve()
    d_plain, d_followed = r.denoise_frame(plain, beauty), r.denoise_frame(followed, beauty)
    mse = lambda img, m: float(np.mean((img[..., 0:3].astype(np.float64) - truth)[m] ** 2))            # noqa: E731
    print(f"quality: box with spheres, {W} x {H}, {a.spp} spp, truth {a.truth_spp} spp, default denoiser options, max_follow {a.follow}")
    for what, msk in ((f"pixels whose first hit is the mirror or the glass sphere ({int(spec.sum())})", spec), (f"whole image ({W * H})", np.ones((H, W), bool))):
        e0, e1, e2 = mse(raw, msk), mse(d_plain, msk), mse(d_followed, msk)
        print(f"{what}: mse raw {e0:.6g}, denoised with first-hit guides {e1:.6g}, with followed guides {e2:.6g}; followed / first-hit = {e2 / e1:.3f}")
r.close()
