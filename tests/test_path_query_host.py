"""hj_trace_paths, the part that needs no GPU: the symbol is declared, listed and exported; every argument refusal comes before the
device is touched, with its status and a message, and writes nothing; a valid call gets HJ_ERR_DEVICE where there is no device; the
Python wrapper's own checks raise before any call; the reference of the GPU tests (path_query_ref.compose) IS the oracle's
integrator on a block's camera rays, and the GPU tests' ray sets hold what they claim; the compiler's resource report of the unit."""
import os
import re
import subprocess

import numpy as np
import pytest

import path_query_ref as R
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions

U = np.uint32


def _call(rays, n, spp, opts, flags, samples, stats=None, ctx=None):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)  # noqa: E731
    return device.lib().hj_trace_paths(ctx, p(rays), n, spp, opts, flags, p(samples), stats)


def test_entry_point_is_declared_listed_and_exported():
    assert "hj_trace_paths" in declared_functions("hijiki_hip.h")
    assert "hj_trace_paths" in device.EXPORTS and hasattr(device.lib(), "hj_trace_paths")
    assert device.lib().hj_version() >= 0x000C00
    assert abi.PATHS_DEVICE_ARRAYS == 1
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    assert "#define HJ_PATHS_DEVICE_ARRAYS 1u" in header
    assert callable(device.Renderer.trace_paths)


def _opts(**kw):
    o = abi.RenderOpts.default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_argument_refusals_come_before_the_device():
    L = device.lib()
    rays, out = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32)
    st = abi.RenderStats()
    INV, UNS = abi.HJ_ERR_INVALID, abi.HJ_ERR_UNSUPPORTED
    cases = {
        "null rays": (INV, (None, 4, 1, None, 0, out)),
        "null samples": (INV, (rays, 4, 1, None, 0, None)),
        "unknown flag bits": (INV, (rays, 4, 1, None, 2, out)),
        "unknown flag bits beside the known one": (INV, (rays, 4, 1, None, 0x80000001, out)),
        "spp 0": (INV, (rays, 4, 0, None, 0, out)),
        "spp above 65536": (INV, (rays, 4, 65537, None, 0, out)),
        "too many rays": (INV, (rays, 0x80000000, 1, None, 0, out)),
        "misaligned device rays": (INV, (rays.ctypes.data + 4, 3, 1, None, abi.PATHS_DEVICE_ARRAYS, out)),
        "misaligned device samples": (INV, (rays, 3, 1, None, abi.PATHS_DEVICE_ARRAYS, out.ctypes.data + 8)),
        "max_bounces 0": (INV, (rays, 4, 1, _opts(max_bounces=0), 0, out)),
        "use_bvh 0": (UNS, (rays, 4, 1, _opts(use_bvh=0), 0, out)),
        "split kernels": (INV, (rays, 4, 1, _opts(flags=abi.RENDER_SPLIT_KERNELS), 0, out)),
        "no drain beside the light grid bit": (INV, (rays, 4, 1, _opts(flags=abi.RENDER_NO_DRAIN | abi.RENDER_NO_LIGHT_GRID), 0, out)),
    }
    for name, (status, args) in cases.items():
        L.hj_context_create(-1, None)                                  # (leaves ITS text in hj_last_error(NULL))
        before = L.hj_last_error(None)
        assert _call(*args, stats=st) == status, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_trace_paths" in text, (name, text)
    assert (out == 0).all() and (rays == 0).all()
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


def test_a_valid_call_without_a_gpu_is_a_device_error():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none."""
    L = device.lib()
    rays, out = np.zeros((4, 8), np.float32), np.full((4, 8), 7.0, np.float32)
    for flags, n, spp, o in ((0, 4, 1, None), (0, 4, 65536, _opts(flags=abi.RENDER_NO_LIGHT_GRID)), (0, 0, 1, None)):
        rc = _call(rays, n, spp, o, flags, out)
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert (out == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = np.zeros((3, 8), np.float32)
    for bad in (good.astype(np.float64), np.zeros((3, 7), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            r.trace_paths(bad)
    for seeds in (np.zeros(3, np.int32), np.zeros(4, np.uint32), np.zeros((3, 1), np.uint32), np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            r.trace_paths(good, seeds=seeds)
    for spp in (0, 65537, -1):
        with pytest.raises(ValueError):
            r.trace_paths(good, spp=spp)
    import torch
    for bad in (torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.float64)):      # on the host: not the renderer's GPU
        with pytest.raises(ValueError):
            r.trace_paths(bad)
    assert (good == 0).all()


@pytest.mark.parametrize("name", ["cbox", "env"])
def test_compose_on_camera_rays_is_the_integrator(name):
    """Premise (a): compose() on the oracle's camera rays and block seeds of a 32 x 32 block equals hjo_integrate_block word for
    word, and its counts are the oracle's counters (max_bounces = 40)."""
    from oracle import hj_oracle as oracle
    cs, block, o = R.scene(name), R.camera_block(), R.options(40)
    want, ctr = oracle.integrate_block(cs, block, o)
    got, counts = R.compose(cs, R.camera_rays(cs, block), 1, o)
    assert np.array_equal(got.view(U), want.reshape(-1, 8).view(U)), int((got.view(U) != want.reshape(-1, 8).view(U)).sum())
    assert (counts["paths"], counts["closest_rays"], counts["shadow_rays"], counts["hits"]) == \
           (ctr["paths"], ctr["closest_calls"], ctr["shadow_calls"], ctr["hits"])
    assert counts["unoccluded_shadow_rays"] == ctr["shadow_calls"] - ctr["shadow_hits"]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_ray_sets_hold_what_they_claim(name):
    """Premise (b), from the oracle alone: the GPU test's ray set of each scene holds at least 100 paths that end by a miss, by an
    emissive hit, by roulette and (max_bounces = 5) by the bounce cap, and at least 100 first hits of every material tag the scene
    has; the origins lie in the domain, 300 directions are no unit vectors, at least 200 rays leave the scene at once, the seeds
    include 0, 0xFFFFFFFE and 0xFFFFFFFF."""
    cs, rays = R.scene(name), R.ray_set(name)
    assert rays.shape == (R.N_RAYS, 8)
    lo, hi = R.domain(cs)
    assert ((rays[:, 0:3] >= lo) & (rays[:, 0:3] <= hi)).all()
    length = np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1)
    assert (np.abs(length - 1) > 1e-3).sum() >= 280 and (np.abs(length - 1) < 1e-6).sum() >= R.N_RAYS - 300
    assert length.min() >= 0.49 and length.max() <= 2.01
    assert rays.view(U)[0:3, 6].tolist() == [0, 0xFFFFFFFE, 0xFFFFFFFF]
    _, counts, detail = R.expected(name, 40)
    end, first_id = detail["end"][0], detail["first_id"][0]
    assert (first_id[-200:] < 0).all()                                  # the rays that leave the scene
    for kind in (R.END_MISS, R.END_EMISSIVE, R.END_ROULETTE):
        assert (end == kind).sum() >= 100, (name, kind, int((end == kind).sum()))
    assert (R.expected(name, 5)[2]["end"][0] == R.END_CAP).sum() >= 100, name
    tags = cs.materials >> abi.MATERIAL_TAG_SHIFT
    first_tag = tags[first_id[first_id >= 0]]
    for tag in sorted(set(tags.tolist())):
        assert (first_tag == tag).sum() >= 100, (name, tag, int((first_tag == tag).sum()))
    assert counts["shadow_rays"] > counts["unoccluded_shadow_rays"] > 100


def _report(text):
    report, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            report[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    return report


def test_path_query_kernels_add_no_scratch(tmp_path):
    """The compiler's resource report for api/path_query.hip (the flags are the Makefile's; read as test_walk_kernels_use_no_scratch
    reads its unit's): all four k_pq_paths instantiations and k_pq_resolve are there, the LDS is WgShared / WgSharedEnv (the hot nodes
    and the counters: 16 KB + at most 1 KB), and ScratchSize is no larger than what the report `make` wrote
    (hijiki_amd/lib/resource_usage.txt) gives for the fused kernel's explicit-record instantiation: the same called stages carry the
    same spills, the new kernel adds none.  For the environment instantiations that instantiation is the fused kernel's environment
    twin, k_path_wavefront_env<true, false, false>, whose called stages are the environment's (measured: 88 B per lane without, 96 B
    with an environment, on both sides)."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "path_query.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "path_query.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    fused = _report(open(os.path.join(ROOT, "hijiki_amd", "lib", "resource_usage.txt")).read())
    paths = {k: v for k, v in report.items() if "k_pq_paths<" in k}
    assert len(paths) == 4, sorted(report)                              # pair nodes x environment
    resolve = [v for k, v in report.items() if "k_pq_resolve" in k]
    assert len(resolve) == 1 and resolve[0]["ScratchSize"] == 0 and resolve[0]["LDS Size"] == 0
    twin = {False: [v for k, v in fused.items() if "k_path_wavefront<true, false, false>" in k],
            True: [v for k, v in fused.items() if "k_path_wavefront_env<true, false, false>" in k]}
    assert len(twin[False]) == 1 and len(twin[True]) == 1, sorted(fused)
    for k, v in paths.items():
        env = re.search(r"k_pq_paths<(?:true|false), true>", k) is not None
        print(k, v, "fused twin:", twin[env][0]["ScratchSize"])
        assert v["ScratchSize"] <= twin[env][0]["ScratchSize"], (k, v, twin[env][0])
        assert 16384 <= v["LDS Size"] <= 17408, (k, v)
        assert v["LDS Size"] == twin[env][0]["LDS Size"], (k, v)
        assert v["Occupancy"] >= twin[env][0]["Occupancy"], (k, v)
