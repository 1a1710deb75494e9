"""hj_trace_irradiance_adaptive and hj_bake_lightmap_adaptive, the part that needs no GPU: the symbols are declared, listed and
exported; every argument refusal comes before the device is touched, in the documented order, with its status and a message, and
writes nothing; a valid call gets HJ_ERR_DEVICE where there is no device; the Python wrapper's and the command line's own checks;
from the oracle alone, the premises of the GPU tests - the setting spreads every scene's points over every sample count, and the
reference (gather_adaptive_ref.expected) agrees with the headline invariant: a point's record is gather_ref.gather of that point at
spp = n_i -; and the compiler's report of the new unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gather_adaptive_ref as A
import gather_ref as G
import lightmap_ref as LR
import path_adaptive_ref as PA
import path_query_ref as R
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions

U, F = np.uint32, np.float32
NAMES = ("hj_trace_irradiance_adaptive", "hj_bake_lightmap_adaptive")


def _aopts(spp_min=4, spp_step=4, spp_max=16, rel_error=0.5, floor=0.01):
    return abi.AdaptiveOpts(spp_min, spp_step, spp_max, rel_error, floor)


def _opts(**kw):
    o = abi.RenderOpts.default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _p(x):
    return None if x is None else (x if isinstance(x, int) else x.ctypes.data)


def _gather(points, n, a, opts, flags, out, moments=None, stats=None, ctx=None):
    return device.lib().hj_trace_irradiance_adaptive(ctx, _p(points), n, a, opts, flags, _p(out), _p(moments), stats)


def _bake(d, a, gutter, f, opts, image, smap=None, count=None, stats=None, ctx=None):
    return device.lib().hj_bake_lightmap_adaptive(ctx, d, a, gutter, f, opts, _p(image), _p(smap), count, stats)


def _points(n=4):
    pts = np.zeros((n, 8), F)
    pts[:, 4] = 1.0
    return pts


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name), name
    assert device.lib().hj_version() >= 0x001200
    assert C.sizeof(abi.AdaptiveOpts) == 20 and abi.AdaptiveOpts.rel_error.offset == 12
    assert callable(device.Renderer.trace_irradiance_adaptive)
    import inspect
    sig = inspect.signature(device.Renderer.bake_lightmap).parameters
    assert sig["adaptive"].default is None and sig["sample_map"].default is False
    assert len(device.lib().hj_trace_irradiance_adaptive.argtypes) == 9 and len(device.lib().hj_bake_lightmap_adaptive.argtypes) == 10


def test_gather_refusals_come_before_the_device_in_order():
    L = device.lib()
    pts, out, mom = _points(), np.zeros((4, 8), F), np.zeros((4, 4), F)
    keep = pts.copy()
    bad_normal, nan_normal = _points(), _points()
    bad_normal[2, 3:6] = 0
    nan_normal[1, 5] = np.nan
    st = abi.RenderStats()
    INV, UNS = abi.HJ_ERR_INVALID, abi.HJ_ERR_UNSUPPORTED
    DEV, SPH, SH9 = abi.GATHER_DEVICE_ARRAYS, abi.GATHER_SPHERE, abi.GATHER_SH9
    ok = _aopts()
    nan, inf = float("nan"), float("inf")
    cases = {
        "null points": (INV, b"null points", (None, 4, ok, None, 0, out, mom)),
        "null out": (INV, b"null out", (pts, 4, ok, None, 0, None, mom)),
        "unknown flag bits": (INV, b"unknown flag", (pts, 4, ok, None, 8, out, mom)),
        "SH9": (INV, b"SH9", (pts, 4, ok, None, SPH | SH9, out, mom)),
        "SH9 without sphere": (INV, b"SH9", (pts, 4, ok, None, SH9, out, mom)),
        "null adaptive opts": (INV, b"null adaptive", (pts, 4, None, None, 0, out, mom)),
        "spp_min 1": (INV, b"spp_min", (pts, 4, _aopts(spp_min=1), None, 0, out, mom)),
        "spp_step 0": (INV, b"spp_step", (pts, 4, _aopts(spp_step=0), None, 0, out, mom)),
        "spp_max below spp_min": (INV, b"below spp_min", (pts, 4, _aopts(spp_min=8, spp_max=7), None, 0, out, mom)),
        "spp_max above 65536": (INV, b"above 65536", (pts, 4, _aopts(spp_step=4096, spp_max=65537), None, 0, out, mom)),
        "rel_error NaN": (INV, b"rel_error", (pts, 4, _aopts(rel_error=nan), None, 0, out, mom)),
        "rel_error infinite": (INV, b"rel_error", (pts, 4, _aopts(rel_error=inf), None, 0, out, mom)),
        "floor negative": (INV, b"floor", (pts, 4, _aopts(floor=-1e-3), None, 0, out, mom)),
        "65 rounds": (INV, b"rounds", (pts, 4, _aopts(spp_min=2, spp_step=1, spp_max=66), None, 0, out, mom)),
        "too many points": (INV, b"2^31", (pts, 0x80000000, ok, None, 0, out, mom)),
        "misaligned device points": (INV, b"aligned", (pts.ctypes.data + 4, 3, ok, None, DEV, out, mom)),
        "misaligned device out": (INV, b"aligned", (pts, 3, ok, None, DEV, out.ctypes.data + 8, mom)),
        "misaligned device moments": (INV, b"aligned", (pts, 3, ok, None, DEV, out, mom.ctypes.data + 4)),
        "max_bounces 0": (INV, b"max_bounces", (pts, 4, ok, _opts(max_bounces=0), 0, out, mom)),
        "use_bvh 0": (UNS, b"use_bvh", (pts, 4, ok, _opts(use_bvh=0), 0, out, mom)),
        "split kernels": (INV, b"HJ_RENDER", (pts, 4, ok, _opts(flags=abi.RENDER_SPLIT_KERNELS), 0, out, mom)),
        "a zero normal": (INV, b"point 2", (bad_normal, 4, ok, None, 0, out, mom)),
        "a NaN normal": (INV, b"point 1", (nan_normal, 4, ok, None, 0, out, mom)),
        # the order: each call has two faults, the message names the earlier one
        "flags before adaptive": (INV, b"unknown flag", (pts, 4, None, None, 8, out, mom)),
        "adaptive before n": (INV, b"spp_min", (pts, 0x80000000, _aopts(spp_min=1), None, 0, out, mom)),
        "n before alignment": (INV, b"2^31", (pts.ctypes.data + 4, 0x80000000, ok, None, DEV, out, mom)),
        "alignment before opts": (INV, b"aligned", (pts.ctypes.data + 4, 3, ok, _opts(max_bounces=0), DEV, out, mom)),
        "opts before normals": (INV, b"max_bounces", (bad_normal, 4, ok, _opts(max_bounces=0), 0, out, mom)),
    }
    for name, (status, word, args) in cases.items():
        L.hj_context_create(-1, None)                                  # (leaves ITS text in hj_last_error(NULL))
        before = L.hj_last_error(None)
        assert _gather(*args, stats=st) == status, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_trace_irradiance_adaptive" in text and word in text, (name, text)
    assert (out == 0).all() and (bits(pts) == bits(keep)).all() and (mom == 0).all()
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


def bits(a):
    return np.ascontiguousarray(a).view(U)


def test_bake_refusals_come_before_the_device_in_order():
    L = device.lib()
    INV = abi.HJ_ERR_INVALID
    DEV = abi.LIGHTMAP_DEVICE_ARRAYS
    img, smap = np.full((8, 8, 4), 7.0, F), np.full((8, 8), 7, U)
    count, st = C.c_size_t(77), abi.RenderStats()
    d, ok = abi.LightmapDesc(8, 8, 0, 0, 0, 1, 0.0, 0), _aopts()
    ddev = abi.LightmapDesc(8, 8, 0, 0, 0, 1, 0.0, DEV)
    nine = abi.LightmapFilter(9, 0.1, 0.5, 0.0, 0)
    cases = {
        "null desc": (b"null desc", (None, ok, 2, None, None, img, smap)),
        "null image": (b"null image", (d, ok, 2, None, None, None, smap)),
        "desc flags": (b"unknown flag", (abi.LightmapDesc(8, 8, 0, 0, 0, 1, 0.0, 2), ok, 2, None, None, img, smap)),
        "atlas": (b"atlas", (abi.LightmapDesc(0, 8, 0, 0, 0, 1, 0.0, 0), ok, 2, None, None, img, smap)),
        "null adaptive opts": (b"null adaptive", (d, None, 2, None, None, img, smap)),
        "spp_min 1": (b"spp_min", (d, _aopts(spp_min=1), 2, None, None, img, smap)),
        "65 rounds": (b"rounds", (d, _aopts(2, 1, 66), 2, None, None, img, smap)),
        "gutter": (b"gutter", (d, ok, 65, None, None, img, smap)),
        "misaligned device image": (b"device image", (ddev, ok, 2, None, None, img.ctypes.data + 8, smap)),
        "misaligned device sample map": (b"sample map", (ddev, ok, 2, None, None, img, smap.ctypes.data + 4)),
        "filter": (b"iterations", (d, ok, 2, C.byref(nine), None, img, smap)),
        "opts": (b"max_bounces", (d, ok, 2, None, _opts(max_bounces=0), img, smap)),
        "adaptive before gutter": (b"spp_step", (d, _aopts(spp_step=0), 65, None, None, img, smap)),
        "gutter before the filter": (b"gutter", (d, ok, 65, C.byref(nine), None, img, smap)),
        "filter before opts": (b"iterations", (d, ok, 2, C.byref(nine), _opts(max_bounces=0), img, smap)),
    }
    for name, (word, args) in cases.items():
        L.hj_context_create(-1, None)
        before = L.hj_last_error(None)
        assert _bake(*args, count=C.byref(count), stats=st) == INV, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_bake_lightmap_adaptive" in text and word in text, (name, text)
    assert (img == 7.0).all() and (smap == 7).all() and count.value == 77
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


def test_a_valid_call_without_a_gpu_is_a_device_error():
    L = device.lib()
    pts, out, mom = _points(), np.full((4, 8), 7.0, F), np.full((4, 4), 7.0, F)
    img, smap = np.full((8, 8, 4), 7.0, F), np.full((8, 8), 7, U)
    d = abi.LightmapDesc(8, 8, 0, 0, 0, 1, 0.0, 0)
    flt = abi.LightmapFilter(2, 0.1, 0.5, 0.0, 0)
    rcs = [_gather(pts, n, a, o, fl, out, m) for a, n, o, fl, m in
           ((_aopts(), 4, None, 0, mom), (_aopts(2, 1, 65), 4, _opts(flags=abi.RENDER_NO_LIGHT_GRID), abi.GATHER_SPHERE, None),
            (_aopts(4, 5, 11, 0.0, 0.0), 4, None, 0, mom), (_aopts(65536, 1, 65536), 4, None, 0, None), (_aopts(), 0, None, 0, None))]
    rcs += [_bake(d, _aopts(), 2, None, None, img, smap), _bake(d, _aopts(5, 1, 5), 0, C.byref(flt), None, img, None)]
    for rc in rcs:
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert (out == 7.0).all() and (mom == 7.0).all() and (img == 7.0).all() and (smap == 7).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = _points(3)
    for bad in (good.astype(np.float64), np.zeros((3, 7), F), np.zeros(8, F)):
        with pytest.raises(ValueError):
            r.trace_irradiance_adaptive(bad)
    with pytest.raises(ValueError):
        r.trace_irradiance_adaptive(good, seeds=np.zeros(4, U))
    with pytest.raises(ValueError, match="normal"):
        r.trace_irradiance_adaptive(np.zeros((3, 8), F))
    bad_kw = (dict(spp_min=1), dict(spp_step=0), dict(spp_min=8, spp_max=7), dict(spp_max=65537, spp_step=4096), dict(spp_min=2, spp_step=1, spp_max=66),
              dict(rel_error=-1.0), dict(rel_error=float("nan")), dict(floor=float("inf")))
    for kw in bad_kw:
        with pytest.raises(ValueError):
            r.trace_irradiance_adaptive(good, **kw)
        with pytest.raises(ValueError):
            r.bake_lightmap(8, 8, None, adaptive=kw)
    with pytest.raises(TypeError):
        r.trace_irradiance_adaptive(good, sh9=True)
    for kw in (dict(adaptive=dict(spp=4)), dict(adaptive={}, gutter=65), dict(adaptive={}, filter=(9, 0.1, 0.5)), dict(adaptive={}, filter=(2, 0.1)),
               dict(sample_map=True), dict(adaptive={}, offset=float("inf"))):
        with pytest.raises(ValueError):
            r.bake_lightmap(8, 8, 4, **kw)
    with pytest.raises(ValueError):
        r.bake_lightmap(0, 8, None, adaptive={})


def test_cli_refuses_bad_adaptive_arguments():
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    for args, text in ((["--adaptive", "4,4,16,0.5"], "--adaptive without --bake-lightmap"),
                       (["--bake-lightmap", "8x8", "--sample-map", "m.pfm"], "--sample-map without --adaptive"),
                       (["--bake-lightmap", "8x8", "--adaptive", "4,4,16"], "bad --adaptive"), (["--bake-lightmap", "8x8", "--adaptive", "1,4,16,0.5"], "bad --adaptive"),
                       (["--bake-lightmap", "8x8", "--adaptive", "4,0,16,0.5"], "bad --adaptive"), (["--bake-lightmap", "8x8", "--adaptive", "8,4,7,0.5"], "bad --adaptive"),
                       (["--bake-lightmap", "8x8", "--adaptive", "2,1,66,0.5"], "bad --adaptive"), (["--bake-lightmap", "8x8", "--adaptive", "4,4,16,-1"], "bad --adaptive"),
                       (["--bake-lightmap", "8x8", "--adaptive", "4,4,16,0.5,0.01,3"], "bad --adaptive"), (["--bake-lightmap", "8x8", "--adaptive", "4,4,16,x"], "bad --adaptive"),
                       (["--bake-lightmap", "8x8", "--adaptive"], "missing value")):
        r = subprocess.run([exe] + args + ["synthetic:cbox"] if text != "missing value" else [exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr[:200])


def test_the_stop_rule_is_one_text():
    """gather_adaptive_ref imports path_adaptive_ref.stops, and the C sources hold pa_stops once, in the header both units include"""
    assert A.stops is PA.stops
    api = os.path.join(ROOT, "hijiki_amd", "csrc", "api")
    defs = [f for f in sorted(os.listdir(api)) if re.search(r"\bbool pa_stops\(", open(os.path.join(api, f)).read())]
    assert defs == ["adaptive_stop.h"], defs
    for unit in ("path_adaptive.hip", "gather_adaptive.hip"):
        assert '#include "adaptive_stop.h"' in open(os.path.join(api, unit)).read(), unit


@pytest.mark.parametrize("name", list(G.SCENES))
def test_the_setting_spreads_the_points_over_every_sample_count(name):
    """Premise, from the oracle alone: at max_bounces = 40, rounds 4 / +4 / up to 16, rel_error = 0.5, floor = 0.01 - the starting
    setting, kept - each of the four possible n_i is taken by at least 20 of every scene's 566 points (cbox 352 / 101 / 50 / 63, rich
    240 / 31 / 35 / 260, env 386 / 89 / 21 / 70)."""
    e = A.expected_for(name)
    took = {m: int((e["n"] == m).sum()) for m in (4, 8, 12, 16)}
    print(f"{name}, 4 / +4 / 16, rel_error 0.5:", took, "rounds", e["rounds"], e["lists"], e["counts"])
    assert sum(took.values()) == G.N_POINTS and min(took.values()) >= 20, took
    assert e["rounds"] == 4 and e["lists"][0] == G.N_POINTS and e["counts"]["paths"] == int(e["n"].sum()) == sum(4 * l for l in e["lists"])
    assert (e["out"][:, 3] == e["n"]).all() and (e["moments"][:, 3] == e["n"]).all() and (e["out"][:, 6:8] == 0).all()


@pytest.mark.parametrize("name,sphere", [("cbox", False), ("rich", False), ("env", False), ("cbox", True)])
def test_the_reference_agrees_with_the_headline_invariant(name, sphere):
    """expected()'s record of point i is gather_ref.gather of the points of its n_i at spp = n_i, all 8 words, for every point"""
    cs, pts, o = R.scene(name), G.point_set(name), R.options(40)
    e = A.expected_for(name, sphere=sphere)
    counts = dict.fromkeys(G.COUNTS, 0)
    for m in sorted(set(e["n"].tolist())):
        idx = np.flatnonzero(e["n"] == m)
        want, c = G.gather(cs, pts[idx], m, sphere=sphere, opts=o)
        assert np.array_equal(bits(e["out"][idx]), bits(want)), (name, m)
        for k in counts:
            counts[k] += c[k]
    assert counts == e["counts"]


def test_the_reference_scatter_is_lightmap_refs_at_a_fixed_count():
    rng = np.random.default_rng(3)
    pts, rec = np.zeros((40, 8), F), rng.uniform(0, 9, (40, 8)).astype(F)
    pts.view(U)[:, 7] = rng.choice(12 * 10, 40, replace=False)
    for spp in (2, 5, 7):
        rec[:, 3] = spp
        img, smap = A.scatter(pts, rec, 12, 10)
        assert np.array_equal(bits(img), bits(LR.scatter(pts, rec, 12, 10, spp))) and smap.sum() == 40 * spp and (smap != 0).sum() == 40
    rec[:, 3] = rng.integers(2, 17, 40)
    img, smap = A.scatter(pts, rec, 12, 10)
    t = pts.view(U)[:, 7]
    assert np.array_equal(smap.reshape(-1)[t], rec[:, 3].astype(U))
    assert np.array_equal(bits(img.reshape(-1, 4)[t, 0]), bits(rec[:, 0] * (F(3.14159274) / rec[:, 3])))


def _report(text):
    """kernel name -> {field: int} of a -Rpass-analysis=kernel-resource-usage report"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def test_the_new_units_kernels_use_no_scratch():
    """The compiler's resource report of api/gather_adaptive.hip, as `make` put it into the library's report between the lines
    '# gather_adaptive.hip' and '# lightmap_filter.hip': exactly the two new kernels, neither with scratch or LDS, both at 8 waves."""
    text = open(os.path.join(ROOT, "hijiki_amd", "lib", "resource_usage.txt")).read()
    assert "\n# gather_query.hip\n" in text and "\n# gather_adaptive.hip\n" in text
    section = text.split("\n# gather_adaptive.hip\n", 1)[1]
    assert "\n# lightmap_filter.hip\n" in section and "# gather_query.hip" not in section
    report = _report(section.split("\n# lightmap_filter.hip\n", 1)[0])
    names = sorted(re.search(r"k_ga_[a-z]+", k).group(0) for k in report)
    assert names == ["k_ga_accumulate", "k_ga_scatter"], sorted(report)
    for k, v in report.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0 and v["Occupancy"] == 8, (k, v)
