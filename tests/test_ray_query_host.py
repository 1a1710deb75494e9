"""hj_trace_rays, the part that needs no GPU: the symbol is declared, listed and exported, every argument refusal comes before the
device is touched (with its status and a message), a call that is valid gets HJ_ERR_DEVICE where there is no device, the Python
wrapper's own checks raise before any call, and the compiler's resource report of the walk kernels shows no scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions


def _call(rays, n, flags, hits, surface, ctx=None):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)  # noqa: E731
    return device.lib().hj_trace_rays(ctx, p(rays), n, flags, p(hits), p(surface))


def test_entry_point_is_declared_listed_and_exported():
    assert "hj_trace_rays" in declared_functions("hijiki_hip.h")
    assert "hj_trace_rays" in device.EXPORTS and hasattr(device.lib(), "hj_trace_rays")
    assert device.lib().hj_version() >= 0x000A00
    assert (abi.TRACE_ANY_HIT, abi.TRACE_DEVICE_ARRAYS) == (1, 2)
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    assert "#define HJ_TRACE_ANY_HIT 1u" in header and "#define HJ_TRACE_DEVICE_ARRAYS 2u" in header
    assert callable(device.Renderer.trace_rays)


def test_argument_refusals_come_before_the_device():
    L = device.lib()
    rays, hits, surf = np.zeros((4, 8), np.float32), np.zeros((4, 4), np.float32), np.zeros((4, 16), np.float32)
    cases = {
        "null rays": (None, 4, 0, hits, None),
        "null hits": (rays, 4, 0, None, None),
        "unknown flag bits": (rays, 4, 4, hits, None),
        "unknown flag bits beside known ones": (rays, 4, 0x80000001, hits, None),
        "too many rays": (rays, 0x80000000, 0, hits, None),
        "surface with any-hit": (rays, 4, abi.TRACE_ANY_HIT, hits, surf),
        "misaligned device rays": (rays.ctypes.data + 4, 3, abi.TRACE_DEVICE_ARRAYS, hits, None),
        "misaligned device surface": (rays, 3, abi.TRACE_DEVICE_ARRAYS, hits, surf.ctypes.data + 8),
    }
    for name, args in cases.items():
        L.hj_context_create(-1, None)                                  # (leaves ITS text in hj_last_error(NULL))
        before = L.hj_last_error(None)
        assert _call(*args) == abi.HJ_ERR_INVALID, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_trace_rays" in text, (name, text)
    assert (hits == 0).all() and (surf == 0).all() and (rays == 0).all()


def test_a_valid_call_without_a_gpu_is_a_device_error():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none."""
    L = device.lib()
    rays, hits = np.zeros((4, 8), np.float32), np.full((4, 4), 7.0, np.float32)
    for flags, n in ((0, 4), (abi.TRACE_ANY_HIT, 4), (0, 0)):
        rc = _call(rays, n, flags, hits, None)
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert (hits == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError):
        r.trace_rays(good, any_hit=True, surface=True)
    for bad in (good.astype(np.float64), np.zeros((3, 7), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            r.trace_rays(bad)
    import torch
    for bad in (torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.float64)):      # on the host: not the renderer's GPU
        with pytest.raises(ValueError):
            r.trace_rays(bad)


def test_walk_kernels_use_no_scratch(tmp_path):
    """The persistent walk's speed rests on its state staying in registers: the compiler's own resource report for
    api/ray_query.hip - the flags are the Makefile's - gives 0 bytes of scratch per lane for every k_rq_walk instantiation (and
    for the plain form and the surface pass).  Only the report's numbers are read."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "ray_query.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "ray_query.hip")]
    env = dict(os.environ, TMPDIR=str(tmp_path))
    out = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    report = {}
    name = None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    walks = {k: v for k, v in report.items() if "k_rq_walk" in k}
    assert len(walks) == 4, sorted(report)                            # any-hit x pair nodes
    for k, v in report.items():
        if "k_rq_" in k:
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    for k, v in walks.items():
        assert 16384 <= v["LDS Size"] <= 17408, (k, v)               # the head word and the hot nodes
        assert v["Occupancy"] >= 7, (k, v)                            # no worse than the path kernel's own walk
    # the walk's shell and the hit record are hj_walk_segment.h's; the unit does not restate them
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "ray_query.hip")).read()
    segment = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_walk_segment.h")).read()
    assert "__shared__ WgShared sh;" in segment and "load_hot_nodes(sc, sh);" in segment and "trace_persistent<MODE, PAIRS>(" in segment
    assert "HJ_DEV float4 walk_hit_record(const RawHit& h)" in segment and "hit ? h.id : -1" in segment
    assert "walk_segment<ANY ? 1 : 0, PAIRS>(" in src and src.count("walk_hit_record(h)") == 2
    assert "__shared__ WgShared" not in src and "load_hot_nodes(" not in src and "trace_persistent<" not in src and "hit ? h.t" not in src
