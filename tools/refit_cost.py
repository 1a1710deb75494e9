"""What a refit costs and what its tree is worth, for a deformation of growing amplitude (tests/refit_scenes.py: smooth, seeded,
emitters stay): time of hj_build_bvh_device(out_nodes = NULL), of hj_refit_bvh_device (host links once, then kept links) and of
the upload behind each (HJ_UPLOAD_TIMING=1 shows the light-shaft grid's share on scenes small enough to have one), the
surface-area cost refitted / rebuilt, and the frame rate of four trees on the deformed geometry: rebuilt on the device, the
device-built topology refitted, the host-compiled (tuned SAH) topology of the REST shape refitted, and a fresh host compile of the
deformed shapes (a geometry-only twin scene - diffuse and emissive materials - compiled for its tree).  Both kernel forms of the
refit are timed (HJ_REFIT_TILED = 1 / 0).  --oracle adds the oracle's node visits per ray (CPU).  Interleaved, best of --reps; frame
rates with the lowest and highest of the repetitions, so that the scatter can be read beside the effect.  The build the refit is
timed against is this library's own hj_build_bvh_device.  One scene per process, each under its own time limit, chained:

    timeout -k 10 600 python tools/refit_cost.py --scene mesh && timeout -k 10 300 python tools/refit_cost.py --scene cbox --oracle
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hijiki_amd import abi, device, host  # noqa: E402
from refit_scenes import Deformation, shape_boxes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", choices=["mesh", "cbox"], default="mesh", help="mesh: 1 M triangles (c4's scene); cbox: c2's")
ap.add_argument("--tris", type=int, default=0, help="mesh triangles (default: 1 000 000 for mesh, the generator's own for cbox)")
ap.add_argument("--amps", default="0.002,0.01,0.03")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=0, help="default: 64 for mesh, 256 for cbox (frames of 0.1 ... 0.2 s)")
ap.add_argument("--oracle", action="store_true")
a = ap.parse_args()

a.spp = a.spp or (64 if a.scene == "mesh" else 256)
kind = host.SYNTH_CBOX_MESH if a.scene == "mesh" else host.SYNTH_CBOX
tris = a.tris or (1000000 if a.scene == "mesh" else 0)
t0 = time.perf_counter()
cs = host.Scene.synthetic(kind, mesh_triangles=tris).compile()
print(f"{a.scene}: {cs.num_shapes} shapes, host compile (rest shape) {time.perf_counter() - t0:.2f} s")
host_topo = cs.bvh.copy()
r = device.Renderer(0)
dev_topo = r.build_bvh(cs)
d = Deformation(cs, seed=1)
ms = lambda f: (lambda t: (f(), 1e3 * (time.perf_counter() - t))[1])(time.perf_counter())  # noqa: E731


def host_compile_as_it_is(cs):
    """Scene::compile's tree over the shapes of `cs` as they are NOW: a twin scene with the same shapes in the same order."""
    s = host.Scene()
    s.set_camera_cbox()
    dm, em = s.add_diffuse((0.6, 0.6, 0.6)), s.add_emissive((9, 9, 9))
    mat = np.where((cs.materials >> abi.MATERIAL_TAG_SHIFT) == abi.MAT_EMISSIVE, em, dm).tolist()
    ns, nq = len(cs.spheres), len(cs.quads)
    for i, sp in enumerate(cs.spheres):
        s.add_sphere(tuple(sp[:3]), float(sp[3]), mat[i])
    for i, q in enumerate(cs.quads):
        s.add_quad(tuple(q[0:3]), tuple(q[4:7]), tuple(q[8:11]), mat[ns + i])
    v = cs.vertices
    s.add_vertices(v[:, 0:3], v[:, 4:7], np.stack([v[:, 3], v[:, 7]], axis=1))
    tm = np.asarray(mat[ns + nq:])
    cuts = [0] + (np.flatnonzero(tm[1:] != tm[:-1]) + 1).tolist() + [len(tm)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):                              # runs of one material: the triangles keep their order
        if hi > lo:
            s.add_triangles(cs.triangles[lo:hi], int(tm[lo]))
    t = time.perf_counter()
    twin = s.compile()
    dt = time.perf_counter() - t
    assert all((x == y).all() for x, y in zip(shape_boxes(twin), shape_boxes(cs))), "the twin's shapes are not the scene's"
    return twin.bvh.copy(), dt


def frame_rate(upload):
    rates = []
    upload()
    r.create_framebuffer(a.size, a.size)
    r.render_frame(a.spp, 1)
    for _ in range(a.reps):
        r.clear()
        t = time.perf_counter()
        r.render_frame(a.spp, 1)
        rates.append(a.size * a.size * a.spp / (time.perf_counter() - t) / 1e6)
    return rates


def refit_form(tiled, **kw):
    os.environ["HJ_REFIT_TILED"] = tiled
    try:
        return r.refit_bvh(cs, **kw)
    finally:
        del os.environ["HJ_REFIT_TILED"]


for amp in [float(x) for x in a.amps.split(",")]:
    d.apply(amp, t=0.3)
    r.refit_bvh(cs, topology=dev_topo, keep_on_device=True)              # (warm-up; the kept links are the device topology's)
    best = {}
    for _ in range(a.reps):                                               # interleaved pairs: build, refit over kept links
        pair = {"build": ms(lambda: r.build_bvh(cs, keep_on_device=True)),
                "upload after build": ms(lambda: r.upload_scene(cs, device_tree=True)),
                "refit, kept links": ms(lambda: r.refit_bvh(cs, keep_on_device=True)),
                "upload after refit": ms(lambda: r.upload_scene(cs, device_tree=True)),
                "refit tiled": ms(lambda: refit_form("1", keep_on_device=True)),
                "refit plain climb": ms(lambda: refit_form("0", keep_on_device=True)),
                "refit, host links": ms(lambda: r.refit_bvh(cs, topology=dev_topo, keep_on_device=True))}
        print(f"  amplitude {amp}: pair " + ", ".join(f"{k} {v:.2f} ms" for k, v in pair.items())
              + ("" if pair["refit, kept links"] < pair["build"] else "   <-- REFIT NOT FASTER THAN THE BUILD"))
        for k, v in pair.items():
            best[k] = min(best.get(k, v), v)
    _, cost_refit = r.refit_bvh(cs, topology=dev_topo, keep_on_device=True, cost=True)
    refit_dev = r.read_device_bvh()
    rebuilt = r.build_bvh(cs)
    _, cost_rebuilt = r.refit_bvh(cs, topology=rebuilt, keep_on_device=True, cost=True)
    refit_host, cost_host = r.refit_bvh(cs, topology=host_topo, cost=True)
    print(f"amplitude {amp}: best of {a.reps}: " + ", ".join(f"{k} {v:.2f} ms" for k, v in best.items())
          + f"; build / refit = {best['build'] / best['refit, kept links']:.1f}")
    print(f"amplitude {amp}: cost rebuilt {cost_rebuilt:.3f}, device topology refitted {cost_refit:.3f} (x{cost_refit / cost_rebuilt:.3f}), "
          f"host topology refitted {cost_host:.3f} (x{cost_host / cost_rebuilt:.3f})")
    fresh_host, compile_s = host_compile_as_it_is(cs)
    _, cost_fresh = r.refit_bvh(cs, topology=fresh_host, keep_on_device=True, cost=True)
    print(f"amplitude {amp}: fresh host compile of the deformed shapes {compile_s:.2f} s, cost {cost_fresh:.3f} (x{cost_fresh / cost_rebuilt:.3f} of rebuilt)")
    trees = {"rebuilt": rebuilt, "device topology refitted": refit_dev, "host topology refitted": refit_host, "fresh host compile": fresh_host}
    rate = {k: [] for k in trees}
    for _ in range(2):
        for name, nodes in trees.items():
            cs.set_bvh(nodes)
            rate[name] += frame_rate(lambda: r.upload_scene(cs))
    top = max(rate["rebuilt"])
    print(f"amplitude {amp}: {a.size}x{a.size}x{a.spp}, {2 * a.reps} frames each, Mpaths/s lowest ... highest (highest / rebuilt's highest): "
          + ", ".join(f"{k} {min(v):.1f} ... {max(v):.1f} ({max(v) / top:.3f})" for k, v in rate.items()))
    if a.oracle:
        from oracle import hj_oracle
        blocks = host.make_blocks(160, 96, 2, 5)
        for name, nodes in trees.items():
            cs.set_bvh(nodes)
            _, ctr, _ = hj_oracle.render_blocks(cs, blocks, 160, 96)
            print(f"amplitude {amp}: oracle, {name}: {ctr['nodes'] / ctr['closest_calls']:.2f} nodes per closest-hit ray, "
                  f"{ctr['shadow_nodes'] / max(ctr['shadow_calls'], 1):.2f} per shadow ray")
    cs.set_bvh(host_topo)
d.restore()
r.close()
