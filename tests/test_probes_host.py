"""hj_probe_points / hj_bake_probes / hj_sample_probes, the part that needs no GPU: the symbols are declared, listed and exported and
the ABI mirror has the header's layout; every argument refusal comes before the device is touched, in the stated order, with a
message, and writes nothing; the wrapper's own checks raise before any call; the constants are the closed forms; the reference of the
GPU tests (probe_ref) reproduces constant radiance and a linear coefficient field; the compiler's resource report of the unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gather_ref as G
import probe_ref as P
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_probe_points", "hj_bake_probes", "hj_sample_probes")


_desc = P.abi_desc


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _opts(**kw):
    o = abi.RenderOpts.default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001300
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    assert "#define HJ_PROBES_DEVICE_ARRAYS 1u" in header and "#define HJ_PROBE_WORDS 28u" in header
    assert (abi.PROBES_DEVICE_ARRAYS, abi.PROBE_WORDS, P.WORDS) == (1, 28, 28)
    for text in ("12.5663706f", "3.14159274f", "2.09439516f", "0.785398185f"):
        assert text in header, text
    for fn in ("probe_points", "bake_probes", "sample_probes"):
        assert callable(getattr(device.Renderer, fn))


def test_abi_mirror_matches_the_header(tmp_path):
    """size and field offsets of hj_probe_desc as a C compiler lays the header's struct out"""
    names = [n for n, _ in abi.ProbeDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hijiki_hip.h"\nint main(void) {\n  printf("%zu", sizeof(hj_probe_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(hj_probe_desc, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.ProbeDesc)] + [getattr(abi.ProbeDesc, n).offset for n in names], got
    assert got[0] == 52 and names == ["origin", "spacing", "count", "seed", "seed_stride", "min_distance", "flags"]


def test_constants_are_the_closed_forms():
    """4 pi and the clamped-cosine factors pi, 2 pi / 3, pi / 4 (Ramamoorthi and Hanrahan 2001) are the float32 nearest their float64
    closed forms, and the header's decimal texts read back as them."""
    assert P.SPHERE_WEIGHT == F(4 * np.pi) and P.A_BAND == (F(np.pi), F(2 * np.pi / 3), F(np.pi / 4))
    assert [F(float(t)) for t in ("12.5663706", "3.14159274", "2.09439516", "0.785398185")] == [P.SPHERE_WEIGHT, *P.A_BAND]
    assert P.BAND == (0, 1, 1, 1, 2, 2, 2, 2, 2)


# every refusal in the header's order: (what, the word its message holds, the desc's keywords, further keywords of the call)
INF, NAN = float("inf"), float("nan")
DESC_REFUSALS = [
    ("unknown flag bits", b"flag bits", dict(flags=2), {}),
    ("unknown flag bits beside the known one", b"flag bits", dict(flags=0x80000001), {}),
    ("a count of 0", b"count", dict(count=(2, 0, 2)), {}),
    ("a count of 1025", b"count", dict(count=(1025, 1, 1)), {}),
    ("more than 2^22 probes", b"count", dict(count=(1024, 1024, 5)), {}),
    ("a NaN origin", b"origin", dict(origin=(0, NAN, 0)), {}),
    ("an infinite origin", b"origin", dict(origin=(0, 0, -INF)), {}),
    ("a spacing of 0", b"spacing", dict(spacing=(1, 0, 1)), {}),
    ("a negative spacing", b"spacing", dict(spacing=(-1, 1, 1)), {}),
    ("a NaN spacing", b"spacing", dict(spacing=(1, 1, NAN)), {}),
    ("an infinite spacing", b"spacing", dict(spacing=(INF, 1, 1)), {}),
    ("a negative min_distance", b"min_distance", dict(min_distance=-1.0), {}),
    ("a NaN min_distance", b"min_distance", dict(min_distance=NAN), {}),
    ("an infinite min_distance", b"min_distance", dict(min_distance=INF), {}),
]


def _calls():
    """-> the three entry points as functions of (desc or None, keywords), each over arrays this returns too"""
    L = device.lib()
    buf = dict(points=np.full((8, 8), 7.0, F), volume=np.full((8, 28), 7.0, F), spts=np.zeros((4, 8), F), out=np.full((4, 4), 7.0, F),
               stats=abi.RenderStats())
    buf["spts"][:, 4] = 1.0

    def points(d, points=buf["points"], **_):
        return L.hj_probe_points(None, C.byref(d) if d is not None else None, _p(points))

    def bake(d, spp=1, opts=None, probes=buf["volume"], **_):
        return L.hj_bake_probes(None, C.byref(d) if d is not None else None, spp, opts, _p(probes), buf["stats"])

    def sample(d, probes=buf["volume"], spts=buf["spts"], n=4, out=buf["out"], **_):
        return L.hj_sample_probes(None, C.byref(d) if d is not None else None, _p(probes), _p(spts), n, _p(out))
    return {"hj_probe_points": points, "hj_bake_probes": bake, "hj_sample_probes": sample}, buf


def _refused(call, name, status, word, *args, **kw):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call(*args, **kw) == status, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and name.encode() in text and word in text, (name, word, text)


def test_argument_refusals_come_before_the_device():
    calls, buf = _calls()
    INV, UNS, DEV = abi.HJ_ERR_INVALID, abi.HJ_ERR_UNSUPPORTED, abi.PROBES_DEVICE_ARRAYS
    for name, call in calls.items():
        _refused(call, name, INV, b"null desc", None)
        for what, word, dkw, kw in DESC_REFUSALS:
            _refused(call, name, INV, word, _desc(**dkw), **kw)
    _refused(calls["hj_probe_points"], "hj_probe_points", INV, b"null points", _desc(), points=None)
    _refused(calls["hj_probe_points"], "hj_probe_points", INV, b"aligned", _desc(flags=DEV), points=buf["points"].ctypes.data + 4)
    bake = calls["hj_bake_probes"]
    _refused(bake, "hj_bake_probes", INV, b"null probes", _desc(), probes=None)
    _refused(bake, "hj_bake_probes", INV, b"spp", _desc(), spp=0)
    _refused(bake, "hj_bake_probes", INV, b"spp", _desc(), spp=65537)
    _refused(bake, "hj_bake_probes", INV, b"aligned", _desc(flags=DEV), probes=buf["volume"].ctypes.data + 8)
    _refused(bake, "hj_bake_probes", INV, b"max_bounces", _desc(), opts=_opts(max_bounces=0))
    _refused(bake, "hj_bake_probes", UNS, b"use_bvh", _desc(), opts=_opts(use_bvh=0))
    _refused(bake, "hj_bake_probes", INV, b"HJ_RENDER", _desc(), opts=_opts(flags=abi.RENDER_SPLIT_KERNELS))
    sample = calls["hj_sample_probes"]
    for missing in ("probes", "spts", "out"):
        _refused(sample, "hj_sample_probes", INV, b"null", _desc(), **{missing: None})
    for where in ("probes", "spts", "out"):
        a = buf["volume" if where == "probes" else where]
        _refused(sample, "hj_sample_probes", INV, b"aligned", _desc(flags=DEV), **{where: a.ctypes.data + 4})
    _refused(sample, "hj_sample_probes", INV, b"points, at most", _desc(), n=0x80000000)

    def bad(word, *v):
        p = buf["spts"].copy()
        p[2, word:word + len(v)] = v
        return p
    for what, p in (("a NaN position", bad(1, NAN)), ("an infinite position", bad(0, -INF)), ("a NaN normal", bad(3, NAN, 0, 1)),
                    ("an infinite normal", bad(5, INF)), ("an all-zero normal", bad(3, 0, 0, 0)), ("a negative-zero normal", bad(3, -0.0, -0.0, 0))):
        _refused(sample, "hj_sample_probes", INV, b"point 2", _desc(), spts=p)
    assert (buf["points"] == 7.0).all() and (buf["volume"] == 7.0).all() and (buf["out"] == 7.0).all()
    assert not any(getattr(buf["stats"], f) for f, _ in abi.RenderStats._fields_)


def test_refusals_come_in_the_stated_order():
    """Two faults in one call: the earlier check's message.  Each refusal of the desc is paired with the one behind it, and the last of
    them with what each entry point checks next."""
    calls, buf = _calls()
    L = device.lib()
    order = [("flag bits", dict(flags=2)), ("count", dict(count=(0, 1, 1))), ("origin", dict(origin=(NAN, 0, 0))),
             ("spacing", dict(spacing=(0, 1, 1))), ("min_distance", dict(min_distance=-1.0))]
    for name, call in calls.items():
        for i in range(len(order)):
            kw = {}
            for _, k in order[i:]:
                kw.update(k)
            assert call(_desc(**kw), spp=0, n=0x80000000, opts=_opts(max_bounces=0)) == abi.HJ_ERR_INVALID
            assert order[i][0].encode() in L.hj_last_error(None), (name, order[i][0], L.hj_last_error(None))
        assert call(None, points=None, probes=None) == abi.HJ_ERR_INVALID and b"null desc" in L.hj_last_error(None)
        assert call(_desc(flags=2), points=None, probes=None) == abi.HJ_ERR_INVALID and b"null" in L.hj_last_error(None)
    DEV = abi.PROBES_DEVICE_ARRAYS
    odd = buf["volume"].ctypes.data + 4
    bake, sample = calls["hj_bake_probes"], calls["hj_sample_probes"]
    for kw, word in ((dict(spp=0, probes=odd, opts=_opts(max_bounces=0)), b"spp"), (dict(spp=1, probes=odd, opts=_opts(max_bounces=0)), b"aligned"),
                     (dict(spp=1, opts=_opts(max_bounces=0, use_bvh=0)), b"max_bounces")):
        assert bake(_desc(flags=DEV), **kw) == abi.HJ_ERR_INVALID and word in L.hj_last_error(None), (word, L.hj_last_error(None))
    zero = buf["spts"].copy()
    zero[0, 3:6] = 0
    for kw, word in ((dict(probes=odd, n=0x80000000), b"aligned"), (dict(n=0x80000000), b"at most")):
        assert sample(_desc(flags=DEV), **kw) == abi.HJ_ERR_INVALID and word in L.hj_last_error(None), (word, L.hj_last_error(None))
    assert sample(_desc(), spts=zero, n=0x80000000) == abi.HJ_ERR_INVALID and b"at most" in L.hj_last_error(None)
    assert sample(_desc(), spts=zero) == abi.HJ_ERR_INVALID and b"normal" in L.hj_last_error(None)


def test_a_valid_call_without_a_gpu_is_a_device_error():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none - also the sample call
    with n == 0 and no arrays at all, which a context would answer with HJ_OK."""
    calls, buf = _calls()
    L = device.lib()
    for name, call, kw in (("hj_probe_points", calls["hj_probe_points"], {}), ("hj_bake_probes", calls["hj_bake_probes"], dict(spp=65536)),
                           ("hj_sample_probes", calls["hj_sample_probes"], {}),
                           ("hj_sample_probes", calls["hj_sample_probes"], dict(n=0, probes=None, spts=None, out=None))):
        rc = call(_desc(count=(2, 2, 2), min_distance=0.5), **kw)
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None) and name.encode() in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert (buf["points"] == 7.0).all() and (buf["volume"] == 7.0).all() and (buf["out"] == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2))
    for kw in (dict(count=(0, 1, 1)), dict(count=(1, 1025, 1)), dict(count=(1024, 1024, 8)), dict(count=(2, 2)), dict(origin=(0, NAN, 0)),
               dict(origin=(0, 0)), dict(spacing=(1, 0, 1)), dict(spacing=(1, -2, 1)), dict(spacing=(INF, 1, 1)), dict(seed=-1), dict(seed_stride=1 << 32)):
        with pytest.raises(ValueError):
            r.probe_points(**dict(good, **kw))
        with pytest.raises(ValueError):
            r.bake_probes(spp=1, **dict(good, **kw))
    for kw in (dict(spp=0), dict(spp=65537), dict(spp=1, min_distance=-0.5), dict(spp=1, min_distance=NAN)):
        with pytest.raises(ValueError):
            r.bake_probes(**dict(good, **kw))
    vol, pts = np.zeros((2, 2, 2, 28), F), np.zeros((3, 8), F)
    pts[:, 5] = 1.0
    for v, p, nm in ((np.zeros((2, 2, 28), F), pts, None), (np.zeros((2, 2, 2, 27), F), pts, None), (vol, np.zeros((3, 7), F), None),
                     (vol, pts, pts[:, 3:6]), (vol, pts[:, 0:3], None), (vol, pts[:, 0:3], np.zeros((2, 3), F)), (vol, pts[:, 0:3], np.zeros((3, 3), F))):
        with pytest.raises(ValueError):
            r.sample_probes(v, (0, 0, 0), (1, 1, 1), p, nm)
    for word, v in ((0, NAN), (2, INF), (4, NAN), (5, 0.0)):
        bad = pts.copy()
        bad[1, word] = v
        with pytest.raises(ValueError):
            r.sample_probes(vol, (0, 0, 0), (1, 1, 1), bad)
    with pytest.raises(ValueError):
        r.sample_probes(vol, (0, 0, 0), (1, 0, 1), pts)
    import torch
    with pytest.raises(ValueError):                                    # tensors on the host: not the renderer's GPU
        r.sample_probes(torch.zeros((2, 2, 2, 28)), (0, 0, 0), (1, 1, 1), torch.zeros((3, 8)))


def test_reference_points_and_resolve_by_hand():
    """points(): index order, the product-then-sum position, the wrapping seed; resolve(): one record worked by hand."""
    d = P.desc((1.0, -2.0, 0.5), (0.25, 0.5, 2.0), (3, 2, 2), seed=0xFFFFFFF0, seed_stride=7)
    pts = P.points(d)
    assert pts.shape == (12, 8) and (pts[:, 3:6] == 0).all() and not np.signbit(pts[:, 3:6]).any()
    assert pts.view(U)[:, 7].tolist() == list(range(12))
    assert pts.view(U)[:, 6].tolist() == [(0xFFFFFFF0 + 7 * p) & 0xFFFFFFFF for p in range(12)] and pts.view(U)[3, 6] == 5
    assert pts[7, 0:3].tolist() == [1.25, -2.0, 2.5]                    # p = 7: x = 1, y = 0, z = 1
    assert pts[5, 0:3].tolist() == [1.5, -1.5, 0.5]                     # p = 5: x = 2, y = 1, z = 0
    rec = np.zeros((2, 36), F)
    rec[:, 8:35] = np.arange(1, 28)
    rec[0, 5], rec[1, 5] = 0.25, np.inf
    out = P.resolve(rec, 8, 0.5)
    s = F(12.5663706) / F(8)
    assert out[0, 0] == (F(1) * s) * F(3.14159274) and out[0, 3] == (F(4) * s) * F(2.09439516) and out[0, 26] == (F(27) * s) * F(0.785398185)
    assert out[0, 11] == (F(12) * s) * F(2.09439516) and out[0, 12] == (F(13) * s) * F(0.785398185)
    assert out[:, 27].tolist() == [0.0, 1.0] and P.resolve(rec, 8, 0.25)[:, 27].tolist() == [1.0, 1.0]


def test_reference_reproduces_constant_radiance():
    """A volume whose every probe holds the resolve of constant radiance 1 - fabricated sums sum[8 + c] = spp * c0, all others 0, the
    exact integrals of Y_j over the sphere - samples to pi, the irradiance under a uniform sky of 1, at random points and normals.
    Relative 1e-6: under ten float32 roundings of 6e-8 each (c0 twice, 4 pi, pi, the two products, the weights, their sum, the
    division, the evaluation)."""
    spp = 16
    rec = np.zeros((1, 36), F)
    rec[0, 8:11] = F(spp) * G.C0
    rec[0, 5] = np.inf
    d = P.desc((-1.0, 0.0, 2.0), (0.5, 0.75, 1.25), (4, 3, 5))
    vol = np.repeat(P.resolve(rec, spp, 0.0), 60, axis=0)
    assert (vol[:, 27] == 1).all() and (vol[:, 3:27] == 0).all()
    pts = P.sample_points(d, 600, seed=1)
    out = P.sample(d, vol, pts)
    print("constant radiance 1: irradiance in", out[:, 0:3].min(), out[:, 0:3].max(), "weights in", out[:, 3].min(), out[:, 3].max())
    assert np.abs(out[:, 0:3].astype(np.float64) / np.pi - 1).max() <= 1e-6
    assert np.abs(out[:, 3].astype(np.float64) - 1).max() <= 1e-6


def test_reference_reproduces_a_linear_field():
    """Two volumes that bracket a coefficient field linear in x - the field rounded down and rounded up to float32 at every probe -
    reproduce the linear function at interior points: trilinear interpolation is exact for it, so the exact value lies between the
    two results up to the same ten roundings (relative 1e-6 of the field's magnitude).  The normal is +z and only Y_0 carries a
    coefficient, so the result is c0 times the interpolated coefficient."""
    d = P.desc((0.3, -1.0, 0.0), (0.7, 0.4, 1.1), (5, 4, 3))
    pp = P.points(d)[:, 0:3].astype(np.float64)
    field = lambda x: 2.0 + 0.37 * x                                    # noqa: E731
    exact = field(pp[:, 0])
    near = exact.astype(F)
    lo = np.where(near.astype(np.float64) <= exact, near, np.nextafter(near, F(-np.inf)))
    hi = np.where(near.astype(np.float64) >= exact, near, np.nextafter(near, F(np.inf)))
    rng = np.random.default_rng(4)
    pts = np.zeros((500, 8), F)
    pts[:, 0:3] = rng.uniform(pp.min(0), pp.max(0), (500, 3))
    pts[:, 5] = 1.0
    res = []
    for v in (lo, hi):
        vol = np.zeros((60, 28), F)
        vol[:, 0:3] = v[:, None]
        vol[:, 27] = 1.0
        res.append(P.sample(d, vol, pts)[:, 0].astype(np.float64) / float(G.C0))
    want = field(pts[:, 0].astype(np.float64))
    print("linear field: below by at most", (res[0] - want).max() / want.max(), "above by at least", (res[1] - want).min() / want.max())
    tol = 1e-6 * np.abs(want).max()
    ulp = float(np.spacing(F(np.abs(exact).max())))                     # the two volumes differ by at most this at any probe
    assert (res[0] <= want + tol).all() and (res[1] >= want - tol).all()
    # ... and two-sided: interpolation is a convex combination, so a volume within one ulp of the field gives a result within one
    # ulp of the exact value, beside the roundings
    assert (np.abs(res[0] - want) <= tol + ulp).all() and (np.abs(res[1] - want) <= tol + ulp).all()


def test_fabricated_volumes_and_points_hold_what_they_claim():
    for count in ((1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2), (5, 4, 3)):
        vol = P.fabricated_volume(count, 9)
        valid = vol[..., 27]
        assert vol.shape == (count[2], count[1], count[0], 28) and set(np.unique(valid)) <= {0.0, 0.25, 1.0}
        assert np.isnan(vol[valid == 0, 0:27]).all() and np.isfinite(vol[valid != 0]).all()
        assert (valid == 1).any() and (valid.size < 2 or (valid == 0.25).any()) and (valid.size < 3 or (valid == 0).any()), (count, valid)
        assert (valid[0:2, 0:2, 0:2] == 0).all() == (count == (5, 4, 3))  # a whole invalid cell only where other cells remain
        d = P.desc((0.5, -1.0, 2.0), (0.5, 0.25, 1.5), count)
        pts = P.sample_points(d, 130, 3, nonfinite=True)
        assert np.isnan(pts[:, 0:3]).any() and np.isposinf(pts[:, 0:3]).any() and np.isneginf(pts[:, 0:3]).any()
        assert np.isfinite(pts[:, 3:6]).all() and (pts[:, 3:6] != 0).any(1).all()
        out = P.sample(d, vol, pts)
        finite = np.isfinite(pts[:, 0:3]).all(1)
        assert np.isfinite(out).all(), "a NaN coefficient behind a zero weight leaked, or a clamp let a NaN through"
        assert (out[out[:, 3] == 0] == 0).all() and finite.sum() > 100
        live = out[out[:, 3] != 0]
        distinct = len(np.unique(live.view(U), axis=0))
        print(count, "rows with weight:", len(live), "of", len(out), "distinct:", distinct)
        # at every count most rows carry weight and coefficients, and they differ (one probe: the normals alone tell rows apart)
        assert len(live) >= 100 and distinct >= 90 and (live[:, 0:3] != 0).any(1).all(), (count, len(live), distinct)
    pts = P.sample_points(d, 260, 3)
    length = np.linalg.norm(pts[:, 3:6].astype(np.float64), axis=1)
    assert np.isfinite(pts[:, 0:6]).all() and (np.abs(length - 1) > 1e-3).sum() > 40 and length.min() >= 0.49 and length.max() <= 2.01
    hi = d["origin"] + (np.array(count) - 1) * d["spacing"]
    assert (pts[:, 0:3] < d["origin"]).any(0).all() and (pts[:, 0:3] > hi).any(0).all()       # outside on each side of each axis
    assert (pts[:, 0:3] == hi).all(1).any() and (pts[:, 0:3] == d["origin"]).all(1).any()       # corners; the last planes


def test_probe_kernels_use_no_scratch():
    """The compiler's resource report of api/probe_volume.hip, as `make` put it into the library's report between the lines
    '# probe_volume.hip' and '# gather_adaptive.hip': the three kernels are there, none has scratch or LDS."""
    text = open(os.path.join(ROOT, "hijiki_amd", "lib", "resource_usage.txt")).read()
    assert "\n# probe_volume.hip\n" in text
    section = text.split("\n# probe_volume.hip\n", 1)[1]
    assert "\n# gather_adaptive.hip\n" in section and "# gather_query.hip" not in section
    report = _report(section.split("\n# gather_adaptive.hip\n", 1)[0])
    names = {re.search(r"k_pv_[a-z]+", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_pv_points", "k_pv_resolve", "k_pv_sample"], sorted(report)
    for k, v in names.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0, (k, v)


def test_the_sh_basis_is_one_text():
    """The gather's reduction and the probe look-up evaluate the same function: the C sources hold the basis' constants once, in the
    header both include."""
    src = os.path.join(ROOT, "hijiki_amd", "csrc")
    holds = []
    for sub in ("api", "kernels"):
        for f in sorted(os.listdir(os.path.join(src, sub))):
            if "0x1.20dd76p-2f" in open(os.path.join(src, sub, f)).read():
                holds.append(f)
    assert holds == ["hj_sh9.h"], holds
    assert '#include "../kernels/hj_sh9.h"' in open(os.path.join(src, "api", "gather_query.hip")).read()
    assert '#include "hj_sh9.h"' in open(os.path.join(src, "kernels", "hj_probes.h")).read()
