"""What the texel stage and the bake cost, on one box, interleaved.

Scenes: the cbox test scene with a UV-mapped floor and box (tests/lightmap_scenes.bake_scene), the synthetic 1 M-triangle mesh, and
that mesh with one chart over the whole atlas behind it (a large footprint among a million small ones).
When the mesh brings no usable UVs (hardly a texel owned), the tool gives it a grid atlas: its triangles get vertices of their own,
triangle i the cell i of a ceil(sqrt(n)) x ceil(sqrt(n)) grid over [0, 1]^2, its three uv inside three corners of the cell; the
tree of that scene is built on the device.

    texels   Renderer.lightmap_texels(device=True) at 1024 x 1024 and 4096 x 4096 on both scenes
    bake     Renderer.bake_lightmap(device=True) at --bake-size, --spp, beside the same run's trace_irradiance over the identical
             points: the difference is rasterise + scatter + dilate
    check    on the mesh: the texel stage at --bake-size against trace_irradiance at spp = 16 over its own output (DESIGN.md 4,
             "Light-map baking": a texel stage that takes longer than that gather has the wrong work split)

    filter   (--filter: this section alone, on the cbox scene and the mesh) Renderer.filter_lightmap(device=True) at 1024 x 1024 and
             4096 x 4096 over the texel stage's points, 1 ... 5 iterations, in three contexts: every step in the LDS form
             (HJ_LIGHTMAP_FILTER_LDS_STEP=128), every step in the direct form (0), the default; beside trace_irradiance at spp = 16
             over the same points.  A call of N iterations is the guide (32 B a texel zeroed, then the scatter), the steps
             1 ... 2^(N-1) and, for odd N, one copy of the image; a step's time is the difference of two calls' best times.  Beside it
             the bytes an iteration must move - 48 B read and 16 B written per guided texel - and the multiple of their time at
             6.3 TB/s that the step takes.

    adaptive (--adaptive: this section alone, on the cbox scene and the mesh) Renderer.bake_lightmap(device=True) at --bake-size:
             the fixed bake at 16 and 64 spp beside the adaptive bake at 4 / +4 / 64 (--rel-error, floor 0.01), and beside the fixed
             bake at the adaptive bake's own mean sample count (rounded): the same total samples without the between-round work
             (accumulate + compaction + one synchronisation a round).  Beside the times the samples taken, the rounds run and the
             RMSE over the owned texels against a bake at --truth-spp.

--pairs interleaved runs after a warm-up of each; a run's time is a host clock between two device synchronisations; ms, lowest ...
highest.  No threshold is set: the table belongs in DESIGN.md ("Light-map baking"), the raw output in profiles/ (--out).  Run under
its own time limit:

    timeout -k 10 600 python tools/lightmap_cost.py --out profiles/lightmap_cost_mi355x.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)
from hijiki_amd import device, host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mesh-triangles", type=int, default=1000000)
ap.add_argument("--bake-size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--gutter", type=int, default=2)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--filter", action="store_true", help="the filter section alone")
ap.add_argument("--adaptive", action="store_true", help="the adaptive section alone")
ap.add_argument("--rel-error", type=float, default=0.05)
ap.add_argument("--truth-spp", type=int, default=4096)
ap.add_argument("--out", default="", help="append the run to this file")
a = ap.parse_args()

LINES = []
dev = torch.device("cuda", 0)


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(f):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = f()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t, out


def spread(v):
    return f"{min(v) * 1e3:.2f} ... {max(v) * 1e3:.2f} ms"


def interleaved(runs):
    for f in runs.values():                                             # warm-up of each (allocations, first launches)
        f()
    secs = {k: [] for k in runs}
    for _ in range(a.pairs):
        for k, f in runs.items():
            secs[k].append(timed(f)[0])
    return secs


def with_grid_atlas(cs, chart=False):
    """The triangles of cs with vertices of their own and the uv of a grid atlas, under an area light over a floor quad, compiled
    without a tree (it is built on the device) -> (compiled scene, cells per side).  chart: behind them (the highest indices: they
    own only what the grid leaves) the floor as two triangles whose uv cover all of [0, 1]^2 - one large chart among a million
    sub-texel triangles."""
    tri = cs.triangles
    n = len(tri)
    side = int(np.ceil(np.sqrt(n)))
    rec = cs.vertices[tri].reshape(-1, 8)
    i = np.repeat(np.arange(n), 3)
    corner = np.tile(np.array([[0.05, 0.05], [0.95, 0.05], [0.05, 0.95]]), (n, 1))
    uv = np.stack([(i % side + corner[:, 0]) / side, (i // side + corner[:, 1]) / side], 1).astype(np.float32)
    s = host.Scene()
    s.set_camera_cbox()
    lo, hi = rec[:, 0:3].min(0), rec[:, 0:3].max(0)
    ext = float((hi - lo).max())
    s.add_quad((lo[0] - ext, lo[1] - 0.01 * ext, hi[2] + ext), (3 * ext, 0, 0), (0, 0, -3 * ext), s.add_diffuse((0.7, 0.7, 0.7)))
    s.add_quad((lo[0], hi[1] + ext, lo[2]), (ext, 0, 0), (0, 0, ext), s.add_emissive((15.0, 15.0, 15.0)))
    base = s.add_vertices(rec[:, 0:3], rec[:, 4:7], uv)
    s.add_triangles(base + np.arange(3 * n).reshape(-1, 3), s.add_diffuse((0.6, 0.6, 0.6)))
    if chart:
        y = lo[1] - 0.005 * ext
        quad = np.array([[lo[0], y, lo[2]], [hi[0], y, lo[2]], [hi[0], y, hi[2]], [lo[0], y, hi[2]]], np.float32)
        quv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
        b2 = s.add_vertices(quad, np.tile(np.array([0, 1, 0], np.float32), (4, 1)), quv)
        s.add_triangles(b2 + np.array([[0, 1, 2], [0, 2, 3]]), s.add_diffuse((0.7, 0.7, 0.7)))
    return s.compile(with_tree=False), side


def upload(cs):
    if cs.desc.num_bvh_nodes == 0:                                      # no tree on the host: built on the device, taken over there
        r.build_bvh(cs, keep_on_device=True)
        r.upload_scene(cs, device_tree=True)
    else:
        r.upload_scene(cs)


def filter_section(name, cs, forms):
    """forms: {"lds": renderer, "direct": renderer, "default": renderer} (contexts created under their switch; the filter reads no scene)"""
    pos = cs.vertices[:, 0:3]
    d = pos.max(0) - pos.min(0)
    sig = (float(np.float32(0.01) * np.sqrt((d * d).sum(dtype=np.float32))), 0.5, 0.0)
    say(f"{name}: filter, sigmas {sig[0]:.4g} / {sig[1]} / {sig[2]} (1 % of the mesh's diagonal, the command line's defaults)")
    for S in (1024, 4096):
        pts = r.lightmap_texels(S, S, offset=1e-3, device=True)
        img = torch.rand((S, S, 4), device=dev)
        runs = {"gather 16 spp": lambda: r.trace_irradiance(pts, spp=16)}
        for form, rr in forms.items():
            for n in range(1, 6):
                runs[f"{form} {n}"] = (lambda rr=rr, n=n: rr.filter_lightmap(img, pts, n, *sig, device=True))
        all_secs = interleaved(runs)
        secs = {k: min(v) for k, v in all_secs.items()}
        need = 64.0 * len(pts)
        floor = need / 6.3e12
        say(f"  {S} x {S}, {len(pts)} guided texels of {S * S}: {a.pairs} interleaved runs, lowest ... highest; an iteration must move "
            f"{need / 1e6:.1f} MB = {floor * 1e3:.4f} ms at 6.3 TB/s")
        for k, v in all_secs.items():
            say(f"    {k}: {spread(v)}")
        for form in forms:
            steps = ", ".join(f"s = {1 << (n - 1)}: {(secs[f'{form} {n}'] - secs[f'{form} {n - 1}']) * 1e3:.3f} ms "
                              f"({(secs[f'{form} {n}'] - secs[f'{form} {n - 1}']) / floor:.1f} x)" for n in range(2, 6))
            say(f"    {form}, a step as the difference of two calls' best (odd N carry one image copy more): {steps}")
        say(f"    5 iterations (default) / gather at 16 spp, best of each: {secs['default 5'] / secs['gather 16 spp']:.3f}")


def adaptive_section(name):
    S, kw = a.bake_size, dict(gutter=0, offset=1e-3, device=True)
    ad = dict(spp_min=4, spp_step=4, spp_max=64, rel_error=a.rel_error, floor=0.01)
    _, smap, st = r.bake_lightmap(S, S, None, adaptive=ad, sample_map=True, stats=True, seed=1 << 30, seed_stride=64, **kw)
    count, total, rounds = st["texels"], st["paths"], st["bounce_rounds"]
    mean = max(1, int(round(total / max(count, 1))))
    runs = {"fixed 16 spp": lambda: r.bake_lightmap(S, S, 16, seed=1 << 30, seed_stride=64, **kw),
            "fixed 64 spp": lambda: r.bake_lightmap(S, S, 64, seed=1 << 30, seed_stride=64, **kw),
            "adaptive 4 / +4 / 64": lambda: r.bake_lightmap(S, S, None, adaptive=ad, seed=1 << 30, seed_stride=64, **kw),
            f"fixed {mean} spp (the adaptive bake's mean)": lambda: r.bake_lightmap(S, S, mean, seed=1 << 30, seed_stride=64, **kw)}
    secs = interleaved(runs)
    truth = r.bake_lightmap(S, S, a.truth_spp, seed=1, seed_stride=a.truth_spp, **kw)
    owned = truth[:, :, 3] == 1
    say(f"{name}: {S} x {S}, {count} texels, rel_error {a.rel_error}: {a.pairs} interleaved runs, lowest ... highest; RMSE over the owned texels against {a.truth_spp} spp")
    for k, f in runs.items():
        img = f()
        rmse = float(torch.sqrt(torch.mean((img[owned][:, 0:3].double() - truth[owned][:, 0:3].double()) ** 2)))
        spp = {"fixed 16 spp": 16 * count, "fixed 64 spp": 64 * count, "adaptive 4 / +4 / 64": total}.get(k, mean * count)
        say(f"    {k}: {spread(secs[k])}; {spp} samples; rounds {rounds if k.startswith('adaptive') else 1}; RMSE {rmse:.5f}")
    hist = torch.bincount(smap.reshape(-1).long(), minlength=65)[4::4].tolist()
    say(f"    adaptive: samples a texel 4, 8, ... 64: {hist}")
    ka, km = "adaptive 4 / +4 / 64", f"fixed {mean} spp (the adaptive bake's mean)"
    say(f"    between-round work: adaptive - fixed at the mean, best of each: {(min(secs[ka]) - min(secs[km])) * 1e3:.2f} ms = "
        f"{(min(secs[ka]) - min(secs[km])) / min(secs[ka]):.3f} of the adaptive call ({total} against {mean * count} samples)")


import lightmap_scenes  # noqa: E402

scenes = {"cbox": lightmap_scenes.bake_scene()}
synth = host.Scene.synthetic(host.SYNTH_CBOX_MESH, a.mesh_triangles).compile(with_tree=False)
r = device.Renderer(0)
upload(synth)
mesh, note = synth, "its own UVs"
if len(r.lightmap_texels(1024, 1024, device=True)) < len(synth.triangles) // 100:
    mesh, side = with_grid_atlas(synth)
    note = f"a grid atlas of {side} x {side} cells"
scenes[f"mesh ({len(mesh.triangles)} triangles, {note})"] = mesh
forms = {}
if a.filter:
    for form, step in (("lds", "128"), ("direct", "0"), ("default", None)):
        if step is None:
            os.environ.pop("HJ_LIGHTMAP_FILTER_LDS_STEP", None)
        else:
            os.environ["HJ_LIGHTMAP_FILTER_LDS_STEP"] = step
        forms[form] = device.Renderer(0)
        forms[form].upload_scene(scenes["cbox"])                        # (a query needs a scene; the filter reads none of it)
    for name, cs in scenes.items():
        upload(cs)
        filter_section(name, cs, forms)
    scenes = {}
elif a.adaptive:
    for name, cs in scenes.items():
        upload(cs)
        adaptive_section(name)
    scenes = {}
else:
    mixed, _ = with_grid_atlas(synth, chart=True)
    scenes[f"mesh + one chart ({len(mixed.triangles)} triangles: the grid atlas, then a pair over the whole atlas)"] = mixed

for name, cs in scenes.items():
    upload(cs)
    say(f"{name}:")
    for size in (1024, 4096):
        f = lambda: r.lightmap_texels(size, size, device=True)           # noqa: E731
        n = len(f())
        say(f"  lightmap_texels {size} x {size}: {n} owned texels, {a.pairs} runs: {spread(interleaved({'texels': f})['texels'])}")
    S = a.bake_size
    pts = r.lightmap_texels(S, S, offset=1e-3, device=True)
    runs = {"bake": lambda: r.bake_lightmap(S, S, a.spp, gutter=a.gutter, offset=1e-3, device=True),
            "gather": lambda: r.trace_irradiance(pts, spp=a.spp),
            "texels": lambda: r.lightmap_texels(S, S, offset=1e-3, device=True)}
    secs = interleaved(runs)
    say(f"  {S} x {S}, {len(pts)} texels x {a.spp} spp, gutter {a.gutter}: {a.pairs} interleaved runs, lowest ... highest")
    for k, v in secs.items():
        say(f"    {k}: {spread(v)}")
    say(f"    bake - gather, best of each: {(min(secs['bake']) - min(secs['gather'])) * 1e3:.2f} ms (rasterise + scatter + dilate)")
    say(f"    texels / gather at spp {a.spp}, best of each: {min(secs['texels']) / min(secs['gather']):.3f}")
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
for rr in forms.values():
    rr.close()
r.close()
