"""What hj_optimize_bvh_device costs and what its tree is worth on c4's 1 M-triangle mesh, interleaved on one GPU: time of
hj_build_bvh_device(out_nodes = NULL) alone and of build + optimise for 1, 2, 4, 8 passes (lowest ... highest of --reps), cost and
moves after each pass (calls of one pass each on the call's own output), and the highest frame rate of --frames frames on (a) the host
tree, (b) the device build alone, (c) the device build plus 8 passes and the vote.  HJ_LBVH_TIMING=1 in the environment adds the
stages' times on stderr; with --stages the run is one build and one call of 8 passes, for those times alone (every mark drains
the stream, so the other figures would not be the call's).

    timeout -k 10 900 python tools/reinsert_cost.py > profiles/NAME.txt 2>&1
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hijiki_amd import device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tris", type=int, default=1000000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frames", type=int, default=6)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--stages", action="store_true", help="one build + one call of 8 passes (for HJ_LBVH_TIMING=1), nothing else")
a = ap.parse_args()

t0 = time.perf_counter()
cs = host.Scene.synthetic(host.SYNTH_CBOX_MESH, mesh_triangles=a.tris).compile()
print(f"mesh: {cs.num_shapes} shapes, host compile {time.perf_counter() - t0:.2f} s", flush=True)
r = device.Renderer(0)
ms = lambda f: (lambda t: (f(), 1e3 * (time.perf_counter() - t))[1])(time.perf_counter())  # noqa: E731
r.build_bvh(cs, keep_on_device=True)                                      # (warm-up)
r.optimize_bvh_device(cs, passes=1)
if a.stages:
    print("---- stages of one build and one call of 8 passes with the vote", file=sys.stderr, flush=True)
    r.build_bvh(cs, keep_on_device=True)
    print(r.optimize_bvh_device(cs, passes=8), flush=True)
    r.close()
    sys.exit(0)

times = {}
for _ in range(a.reps):                                                   # interleaved: build alone, build + k passes
    times.setdefault("build", []).append(ms(lambda: r.build_bvh(cs, keep_on_device=True)))
    for k in (1, 2, 4, 8):
        times.setdefault(f"build + {k} passes", []).append(ms(lambda: (r.build_bvh(cs, keep_on_device=True), r.optimize_bvh_device(cs, passes=k))))
for name, v in times.items():
    print(f"{name:18s} {min(v):8.2f} ... {max(v):8.2f} ms", flush=True)

r.build_bvh(cs, keep_on_device=True)
for k in range(8):
    res = r.optimize_bvh_device(None, passes=1)
    print(f"pass {k}: cost {res['cost_before']:.4f} -> {res['cost_after']:.4f}, {res['moves']} moves", flush=True)
    if res["moves"] == 0:
        break


def frame_rate(upload):
    upload()
    r.create_framebuffer(a.size, a.size)
    r.render_frame(a.spp, 1)
    rates = []
    for _ in range(a.frames):
        r.clear()
        t = time.perf_counter()
        r.render_frame(a.spp, 1)
        rates.append(a.size * a.size * a.spp / (time.perf_counter() - t) / 1e6)
    return rates


routes = {"(a) host tree": lambda: r.upload_scene(cs),
          "(b) device build": lambda: (r.build_bvh(cs, keep_on_device=True), r.upload_scene(cs, device_tree=True)),
          "(c) device build + 8 passes + vote": lambda: (r.build_bvh(cs, keep_on_device=True), r.optimize_bvh_device(cs, passes=8),
                                                         r.upload_scene(cs, device_tree=True))}
best = {}
for _ in range(2):                                                        # interleaved
    for name, up in routes.items():
        v = frame_rate(up)
        best[name] = max(best.get(name, 0.0), max(v))
        print(f"{name:36s} {min(v):8.1f} ... {max(v):8.1f} Msamples/s", flush=True)
for name in routes:
    print(f"{name:36s} highest {best[name]:8.1f} Msamples/s, x{best[name] / best['(a) host tree']:.3f} of the host tree's")
r.close()
