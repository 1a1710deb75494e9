"""What hj_scene_update_shapes costs per frame step against the route it replaces, for a deformation of growing amplitude
(tests/refit_scenes.py), interleaved on one GPU, 3 amplitudes x --reps pairs:

  (a) refit_bvh(keep_on_device) + upload_scene(device_tree=True) - through --parent-lib when given (a libhijiki_hip.so built from
      the parent commit, loaded beside this one), else through this library
  (b) update_shapes from host arrays        (c) update_shapes from torch tensors on the device
  (d) (cbox: the scene has a light-shaft grid) both again with HJ_UPDATE_NO_LIGHT_GRID

then the highest frame rate of 6 frames after (a) and after (b): an update keeps the rest shape's collapse and hot sets, an upload
chooses them anew.  HJ_LBVH_TIMING=1 prints the update's stage times.  One scene per process, each under its own time limit, chained:

    timeout -k 10 600 python tools/update_cost.py --scene mesh && timeout -k 10 300 python tools/update_cost.py --scene cbox
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before the HIP library: one runtime per process)
from hijiki_amd import abi, device, host  # noqa: E402
from refit_scenes import Deformation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", choices=["mesh", "cbox"], default="mesh", help="mesh: 1 M triangles (c4's scene); cbox: c2's")
ap.add_argument("--amps", default="0.002,0.01,0.03")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=0, help="default: 64 for mesh, 256 for cbox")
ap.add_argument("--parent-lib", default="", help="libhijiki_hip.so of the parent commit for route (a)")
ap.add_argument("--out", default="", help="append the run to this file (profiles/r11_scene_update.txt)")
a = ap.parse_args()
a.spp = a.spp or (64 if a.scene == "mesh" else 256)


class ParentRoute:
    """Route (a) through ANOTHER libhijiki_hip.so (the parent commit's): the seven entry points the route needs, declared here by
    hand - a symbol that library lacks raises AttributeError when this class is made, and no call can reach this commit's library."""

    def __init__(self, path, device_index=0):
        vp, L = C.c_void_p, C.CDLL(path)
        L.hj_context_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.hj_context_destroy.argtypes = [vp]
        L.hj_context_destroy.restype = None
        L.hj_last_error.argtypes = [vp]
        L.hj_last_error.restype = C.c_char_p
        L.hj_version.restype = C.c_uint32
        L.hj_scene_upload.argtypes = [vp, C.POINTER(abi.SceneDesc)]
        L.hj_refit_bvh_device.argtypes = [vp, C.POINTER(abi.SceneDesc), C.POINTER(abi.BvhNode), C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_double)]
        L.hj_framebuffer_create.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.hj_framebuffer_clear.argtypes = [vp]
        L.hj_render_frame.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(abi.RenderOpts), C.POINTER(abi.RenderStats)]
        if hasattr(L, "hj_scene_update_shapes"):
            raise SystemExit(f"{path} exports hj_scene_update_shapes: it is not the parent commit's library")
        self.L, self.version, self._h = L, L.hj_version(), vp()
        self._check(L.hj_context_create(device_index, C.byref(self._h)))

    def _check(self, rc):
        if rc != abi.HJ_OK:
            raise abi.HijikiError(rc, (self.L.hj_last_error(self._h) or b"").decode())

    def _desc(self, compiled, nodes):
        d = abi.SceneDesc()
        C.memmove(C.byref(d), C.byref(compiled.desc), C.sizeof(abi.SceneDesc))
        d.bvh = None if nodes is None else nodes.ctypes.data_as(C.POINTER(abi.BvhNode))
        d.num_bvh_nodes = 0 if nodes is None else len(nodes)
        return d

    def refit_bvh(self, compiled, topology=None, keep_on_device=True):
        assert keep_on_device
        got = C.c_size_t(0)
        self._check(self.L.hj_refit_bvh_device(self._h, C.byref(self._desc(compiled, topology)), None, 0, C.byref(got), None))

    def upload_scene(self, compiled, device_tree=True):
        assert device_tree
        self._check(self.L.hj_scene_upload(self._h, C.byref(self._desc(compiled, None))))

    def create_framebuffer(self, w, h):
        self._check(self.L.hj_framebuffer_create(self._h, w, h, None))

    def clear(self):
        self._check(self.L.hj_framebuffer_clear(self._h))

    def render_frame(self, spp, seed):
        st = abi.RenderStats()
        self._check(self.L.hj_render_frame(self._h, spp, seed, 0, spp, 0, 1, None, C.byref(st)))

    def close(self):
        self.L.hj_context_destroy(self._h)


LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


kind = host.SYNTH_CBOX_MESH if a.scene == "mesh" else host.SYNTH_CBOX
cs = host.Scene.synthetic(kind, mesh_triangles=1000000 if a.scene == "mesh" else 0).compile(with_tree=a.scene != "mesh")
r = device.Renderer(0)
ra = ParentRoute(a.parent_lib) if a.parent_lib else device.Renderer(0)
topo = r.build_bvh(cs)
cs.set_bvh(topo)
say(f"{a.scene}: {cs.num_shapes} shapes; route (a) through {'the parent library ' + a.parent_lib if a.parent_lib else 'THIS library'}")
r.upload_scene(cs)
r.update_shapes(cs)                                                        # (the first update: link set and scratch)
ra.refit_bvh(cs, topology=topo, keep_on_device=True)
ra.upload_scene(cs, device_tree=True)
dev = torch.device("cuda", 0)
d = Deformation(cs, seed=1)
ms = lambda f: (lambda t: (f(), 1e3 * (time.perf_counter() - t))[1])(time.perf_counter())  # noqa: E731
grid = a.scene == "cbox"


def arrays():
    return {k: torch.from_numpy(getattr(cs, k).copy()).to(dev) for k in ("vertices", "spheres", "quads")}


def rates(ctx):
    ctx.create_framebuffer(a.size, a.size)
    ctx.render_frame(a.spp, 1)
    out = []
    for _ in range(6):
        ctx.clear()
        t = time.perf_counter()
        ctx.render_frame(a.spp, 1)
        out.append(a.size * a.size * a.spp / (time.perf_counter() - t) / 1e6)
    return out


every = {}
for amp in [float(x) for x in a.amps.split(",")]:
    for rep in range(a.reps):
        d.apply(amp, t=0.3 + 0.1 * rep)
        t_dev = arrays()
        torch.cuda.synchronize()
        pair = {"(a) refit + upload": ms(lambda: (ra.refit_bvh(cs, keep_on_device=True), ra.upload_scene(cs, device_tree=True))),
                "(b) update, host arrays": ms(lambda: r.update_shapes(cs)),
                "(c) update, device arrays": ms(lambda: r.update_shapes(cs, device_arrays=t_dev))}
        if grid:
            pair["(d) update, host arrays, no grid"] = ms(lambda: r.update_shapes(cs, light_grid=False))
            r.upload_scene(cs)                                             # (the grid is gone: a fresh one for the next pair)
            r.update_shapes(cs)
        say(f"  amplitude {amp}, pair {rep}: " + ", ".join(f"{k} {v:.2f} ms" for k, v in pair.items())
              + ("" if pair["(b) update, host arrays"] < pair["(a) refit + upload"] else "   <-- UPDATE NOT FASTER THAN REFIT + UPLOAD"))
        for k, v in pair.items():
            every.setdefault(k, []).append(v)
    ra.refit_bvh(cs, keep_on_device=True)
    ra.upload_scene(cs, device_tree=True)
    r.update_shapes(cs)
    fa, fb = rates(ra), rates(r)
    say(f"amplitude {amp}: {a.size}x{a.size}x{a.spp}, highest of 6 frames: after (a) {max(fa):.1f}, after (b) {max(fb):.1f} Mpaths/s "
          f"(b / a = {max(fb) / max(fa):.3f}; scatter (a) {(max(fa) - min(fa)) / max(fa):.3f}, (b) {(max(fb) - min(fb)) / max(fb):.3f})")
say("all pairs, lowest ... highest: " + ", ".join(f"{k} {min(v):.2f} ... {max(v):.2f} ms" for k, v in every.items()))
d.restore()
r.close()
ra.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n\n")
