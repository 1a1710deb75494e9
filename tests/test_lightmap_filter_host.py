"""hj_filter_lightmap / hj_bake_lightmap_filtered, the part that needs no GPU: the reference of the GPU tests (lightmap_filter_ref)
against exact rational arithmetic rounded once per operation; the two zeros in -a; the colour stop's quadrupling; unguided texels
and alpha; every argument refusal before the device is touched, writing nothing; the ABI mirror against the header; the compiler's
resource report."""
import ctypes as C
import os
import subprocess
from fractions import Fraction as Q

import numpy as np
import pytest

import lightmap_filter_ref as FR
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32


def rnd(q):
    """the float32 nearest to the rational q, ties to even (normal range), as a Fraction; rnd.inexact counts the q that were not representable"""
    if q == 0:
        return q
    e, a = 0, abs(q)
    while a >= 2:
        a, e = a / 2, e + 1
    while a < 1:
        a, e = a * 2, e - 1
    m = a * (1 << 23)                                                   # in [2^23, 2^24)
    lo = m.numerator // m.denominator
    rest = m - lo
    if rest > Q(1, 2) or (rest == Q(1, 2) and lo % 2 == 1):
        lo += 1
    r = Q(lo) * Q(2) ** (e - 23)
    rnd.inexact += r != abs(q)
    return r if q > 0 else -r


rnd.inexact = 0


def exact_iteration(img, guided, s):
    """one iteration with all three sigmas 0 (a = +0, hj_exp(-0) = 1, w = h) in rational arithmetic, every operation rounded once:
    img (H, W, 4) of Fractions as nested lists"""
    H, W = len(img), len(img[0])
    k = (Q(3, 8), Q(1, 4), Q(1, 16))
    out = [[list(px) for px in row] for row in img]
    division = 0
    for y in range(H):
        for x in range(W):
            if not guided[y][x]:
                continue
            total, wsum = [Q(0)] * 3, Q(0)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    xx, yy = x + dx * s, y + dy * s
                    if not (0 <= xx < W and 0 <= yy < H) or not guided[yy][xx]:
                        continue
                    w = rnd(k[abs(dx)] * k[abs(dy)])
                    total = [rnd(total[c] + rnd(img[yy][xx][c] * w)) for c in range(3)]
                    wsum = rnd(wsum + w)
            before = rnd.inexact
            out[y][x][0:3] = [rnd(total[c] / wsum) for c in range(3)]
            division += rnd.inexact - before
    return out, division


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (7, 5)])
@pytest.mark.parametrize("iterations", [1, 3])
def test_reference_is_rational_arithmetic_rounded_once_per_operation(W, H, iterations):
    """Small-integer images, all three sigmas 0: every weight is dyadic and hj_exp(-0) == 1, so in the first iteration every
    product and every sum is exact and only the division rounds; later iterations (steps 2 and 4 reach beyond these atlases) round
    wherever float32 must.  The reference must give the rational model's bits."""
    rng = np.random.default_rng([W, H, iterations])
    img = rng.integers(0, 16, (H, W, 4)).astype(F)
    guided = rng.random((H, W)) < 0.8
    guided[0, 0] = True
    t = np.flatnonzero(guided.ravel())
    pts = np.zeros((len(t), 8), F)
    pts[:, 0:3], pts[:, 4] = rng.normal(size=(len(t), 3)), 1.0              # (positions of any value: the stop is off)
    pts.view(U)[:, 7] = t
    want = [[[Q(float(v)) for v in px] for px in row] for row in img]
    rnd.inexact = 0
    for i in range(iterations):
        before = rnd.inexact
        want, division = exact_iteration(want, guided.tolist(), 1 << i)
        if i == 0:
            assert rnd.inexact - before == division                         # the dyadic claim: nothing but the division rounded
    got = FR.run(img, pts, iterations, 0.0, 0.0, 0.0)
    assert got.shape == (H, W, 4)
    for y in range(H):
        for x in range(W):
            assert [Q(float(v)) for v in got[y, x]] == want[y][x], (x, y, got[y, x], [float(v) for v in want[y][x]])
    if (W, H) == (1, 1):
        assert np.array_equal(got.view(U), img.view(U))                     # c * 0.140625 / 0.140625


def _plane(W, H, seed=0, holes=True):
    """an image, and points over a tilted plane with slowly turning normals: every texel guided but a few"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    guided = (rng.random((H, W)) < 0.9) if holes else np.ones((H, W), bool)
    t = np.flatnonzero(guided.ravel())
    y, x = (t // W).astype(F), (t % W).astype(F)
    pts = np.zeros((len(t), 8), F)
    pts[:, 0], pts[:, 1], pts[:, 2] = x * F(0.1), (x + y) * F(0.01), y * F(0.1)
    n = np.stack([F(0.05) * x, np.ones_like(x), F(0.03) * y], 1)
    pts[:, 3:6] = n / np.linalg.norm(n, axis=1, keepdims=True)
    pts.view(U)[:, 7] = t
    return img, pts, guided


def test_the_two_zeros_in_minus_a():
    """hj_exp(-0) and hj_exp(+0) are both exactly 1: a texel whose taps all share its position, normal and colour has a = +0, -a = -0
    and w = h, so with stops ON a constant image over one point in space filters exactly as with the stops off."""
    assert np.array_equal(FR.hj_exp(F([-0.0, 0.0])).view(U), F([1.0, 1.0]).view(U))
    img, pts, _ = _plane(9, 6, 1)
    img[:, :, 0:3] = F(0.7)
    pts[:, 0:3], pts[:, 3:6] = F([0.3, -1.0, 2.0]), F([0.0, 0.6, 0.8])
    on, off = FR.run(img, pts, 2, 0.01, 0.02, 0.03), FR.run(img, pts, 2, 0.0, 0.0, 0.0)
    assert np.array_equal(on.view(U), off.view(U))


def test_the_colour_stop_quadruples_every_iteration():
    img, pts, _ = _plane(11, 7, 2)
    G, P, N = FR.guides(pts, 11, 7)
    ic = FR.inv_sq(0.6)
    one = FR.iteration(img, G, P, N, 1, F(0), F(0), ic)
    two = FR.iteration(one, G, P, N, 2, F(0), F(0), ic * F(4))
    three = FR.iteration(two, G, P, N, 4, F(0), F(0), (ic * F(4)) * F(4))
    got = FR.run(img, pts, 3, 0.0, 0.0, 0.6, keep=True)
    assert all(np.array_equal(a.view(U), b.view(U)) for a, b in zip(got, (one, two, three)))
    assert FR.inv_sq(0.5) * F(4) == FR.inv_sq(0.25) and FR.inv_sq(0.0) == 0 and FR.inv_sq(2.0) == F(0.25)   # sigma halves: 1 / sigma^2 quadruples
    assert not np.array_equal(two.view(U), FR.iteration(one, G, P, N, 2, F(0), F(0), ic).view(U))              # (the stop does bite here)


def test_unguided_texels_are_copied_and_alpha_is_kept():
    img, pts, guided = _plane(13, 9, 3)
    img[~guided] = np.nan                                               # never read as a tap: nothing of it may spread
    img[2, 3, 3] = np.inf
    out = FR.run(img, pts, 3, 0.5, 0.5, 0.5)
    assert np.array_equal(out[~guided].view(U), img[~guided].view(U))
    assert np.array_equal(out[:, :, 3].view(U), img[:, :, 3].view(U))
    assert np.isfinite(out[guided][:, 0:3]).all() and not np.array_equal(out[guided][:, 0:3], img[guided][:, 0:3])
    none = FR.run(img, np.zeros((0, 8), F), 2, 0.5, 0.5)
    assert np.array_equal(none.view(U), img.view(U))
    skipped = np.concatenate([pts, pts[-1:]])
    skipped.view(U)[-1, 7] = 13 * 9                                     # names no texel: as if it were not there
    assert np.array_equal(FR.run(img, skipped, 2, 0.5, 0.5).view(U), FR.run(img, pts, 2, 0.5, 0.5).view(U))
    assert np.array_equal(FR.run(img, pts, 0, 0.5, 0.5).view(U), img.view(U))


def test_entry_points_are_declared_listed_and_exported():
    for name in ("hj_filter_lightmap", "hj_bake_lightmap_filtered"):
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001100
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    assert "#define HJ_LIGHTMAP_FILTER_MAX_ITERATIONS 8u" in header and abi.LIGHTMAP_FILTER_MAX_ITERATIONS == 8
    assert "{0.375f, 0.25f, 0.0625f}" in header and FR.K == (F(0.375), F(0.25), F(0.0625)) and "0.140625" in header
    assert F(0.375) * F(0.375) == F(0.140625)
    assert callable(device.Renderer.filter_lightmap) and callable(device.default_filter_sigmas)


def test_abi_mirror_matches_the_header(tmp_path):
    """size and field offsets of hj_lightmap_filter as a C compiler lays the header's struct out"""
    names = [n for n, _ in abi.LightmapFilter._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hijiki_hip.h"\nint main(void) {\n  printf("%zu", sizeof(hj_lightmap_filter));\n'
                   + "".join(f'  printf(" %zu", offsetof(hj_lightmap_filter, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.LightmapFilter)] + [getattr(abi.LightmapFilter, n).offset for n in names], got
    assert got[0] == 20 and names == ["iterations", "sigma_position", "sigma_normal", "sigma_color", "flags"]


def _filter(**kw):
    f = abi.LightmapFilter(2, 0.1, 0.5, 0.0, 0)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _points(t, edits=None):
    pts = np.zeros((len(t), 8), F)
    pts[:, 4] = 1.0
    pts.view(U)[:, 7] = t
    for (i, k), v in (edits or {}).items():
        pts[i, k] = v
    return pts


def test_argument_refusals_come_before_the_device():
    """Each refusal: its status, a message that names the entry point, and nothing written."""
    L = device.lib()
    INV, DEV = abi.HJ_ERR_INVALID, abi.LIGHTMAP_DEVICE_ARRAYS
    W, H = 16, 8
    img = np.full((H, W, 4), 7.0, F)
    good = _points([0, 5, 127])
    nan, inf = float("nan"), float("inf")
    bad_filter = {"unknown flag bits": _filter(flags=2), "9 iterations": _filter(iterations=9), "a negative sigma_position": _filter(sigma_position=-1.0),
                  "a NaN sigma_position": _filter(sigma_position=nan), "an infinite sigma_normal": _filter(sigma_normal=inf),
                  "a negative sigma_normal": _filter(sigma_normal=-0.5), "a NaN sigma_color": _filter(sigma_color=nan),
                  "a negative sigma_color": _filter(sigma_color=-1e-30)}
    call = lambda w, h, p, f, im: (w, h, p.ctypes.data if p is not None else None, len(p) if p is not None else 3,  # noqa: E731
                                   C.byref(f) if f is not None else None, im)
    cases = {k: call(W, H, good, f, img.ctypes.data) for k, f in bad_filter.items()}
    cases["null filter"] = call(W, H, good, None, img.ctypes.data)
    cases["null image"] = call(W, H, good, _filter(), None)
    cases["null points with a count"] = call(W, H, None, _filter(), img.ctypes.data)
    cases["width 0"] = call(0, H, good, _filter(), img.ctypes.data)
    cases["height 0"] = call(W, 0, good, _filter(), img.ctypes.data)
    cases["width above 16384"] = call(16385, 1, good, _filter(), img.ctypes.data)
    cases["more than 2^26 texels"] = call(16384, 8192, good, _filter(), img.ctypes.data)
    cases["more points than texels"] = (2, 1, good.ctypes.data, 3, C.byref(_filter()), img.ctypes.data)
    cases["misaligned device points"] = (W, H, good.ctypes.data + 4, 2, C.byref(_filter(flags=DEV)), img.ctypes.data)
    cases["misaligned device image"] = (W, H, good.ctypes.data, 3, C.byref(_filter(flags=DEV)), img.ctypes.data + 8)
    host_points = {"unsorted indices": _points([0, 9, 5]), "a duplicate index": _points([0, 5, 5]), "an index out of range": _points([0, 5, 128]),
                   "the first index out of range": _points([4000000000]), "a NaN normal": _points([0, 5, 127], {(1, 4): nan}),
                   "an infinite normal": _points([0, 5, 127], {(2, 3): inf}), "a NaN position": _points([0, 5, 127], {(0, 2): nan}),
                   "an infinite position": _points([0, 5, 127], {(2, 0): -inf})}
    for k, p in host_points.items():
        cases[k] = call(W, H, p, _filter(), img.ctypes.data)
    for name, args in cases.items():
        L.hj_context_create(-1, None)                                   # (leaves ITS text in hj_last_error(NULL))
        before = L.hj_last_error(None)
        assert L.hj_filter_lightmap(None, *args) == INV, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_filter_lightmap" in text, (name, text)
    assert (img == 7.0).all()
    # the bake: the filter's refusals, between the misaligned device image and the refusals of opts
    d = abi.LightmapDesc(W, H, 0, 0, 0, 1, 0.0, 0)
    o0 = abi.RenderOpts.default()
    o0.max_bounces = 0
    count, st = C.c_size_t(77), abi.RenderStats()
    for name, f in bad_filter.items():
        assert L.hj_bake_lightmap_filtered(None, C.byref(d), 4, 2, C.byref(f), None, img.ctypes.data, C.byref(count), C.byref(st)) == INV, name
        assert b"hj_bake_lightmap_filtered" in L.hj_last_error(None), name
    nine = _filter(iterations=9)
    assert L.hj_bake_lightmap_filtered(None, C.byref(d), 4, 65, C.byref(nine), None, img.ctypes.data, None, None) == INV and b"gutter" in L.hj_last_error(None)
    assert L.hj_bake_lightmap_filtered(None, C.byref(d), 4, 2, C.byref(nine), C.byref(o0), img.ctypes.data, None, None) == INV
    assert b"iterations" in L.hj_last_error(None)
    assert L.hj_bake_lightmap_filtered(None, C.byref(d), 4, 2, None, C.byref(o0), img.ctypes.data, None, None) == INV and b"max_bounces" in L.hj_last_error(None)
    assert L.hj_bake_lightmap_filtered(None, C.byref(d), 0, 2, C.byref(_filter()), None, img.ctypes.data, None, None) == INV and b"spp" in L.hj_last_error(None)
    assert (img == 7.0).all() and count.value == 77 and not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)
    # two faults in one call: the earlier check's message
    assert L.hj_filter_lightmap(None, 0, H, good.ctypes.data, 3, C.byref(nine), img.ctypes.data) == INV and b"iterations" in L.hj_last_error(None)
    assert L.hj_filter_lightmap(None, 0, H, host_points["unsorted indices"].ctypes.data, 3, C.byref(_filter()), img.ctypes.data) == INV
    assert b"atlas" in L.hj_last_error(None)


@pytest.mark.parametrize("iterations", [0, 2])
def test_a_valid_call_without_a_context(iterations):
    """A process without a HIP device cannot hold a context: the valid call it can make - zero iterations included - gets
    HJ_ERR_DEVICE; with a device, a null context is HJ_ERR_INVALID.  Nothing is written either way."""
    L = device.lib()
    img, good = np.full((8, 16, 4), 7.0, F), _points([0, 5, 127])
    d = abi.LightmapDesc(16, 8, 0, 0, 0, 1, 1e-3, 0)
    count = C.c_size_t(77)
    for rc in (L.hj_filter_lightmap(None, 16, 8, good.ctypes.data, 3, C.byref(_filter(iterations=iterations)), img.ctypes.data),
               L.hj_filter_lightmap(None, 16, 8, None, 0, C.byref(_filter(iterations=iterations)), img.ctypes.data),
               L.hj_bake_lightmap_filtered(None, C.byref(d), 4, 0, C.byref(_filter(iterations=iterations)), None, img.ctypes.data, C.byref(count), None)):
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert count.value == 77 and (img == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    img, pts = np.zeros((4, 4, 4), F), _points([0, 3])
    for kw in (dict(iterations=9), dict(iterations=-1), dict(sigma_position=-1.0), dict(sigma_normal=float("nan")), dict(sigma_color=float("inf"))):
        args = dict(iterations=1, sigma_position=0.1, sigma_normal=0.5, sigma_color=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            r.filter_lightmap(img, pts, **args)
        with pytest.raises(ValueError):
            r.bake_lightmap(4, 4, 1, filter=(args["iterations"], args["sigma_position"], args["sigma_normal"], args["sigma_color"]))
    for bad in ((1,), (1, 0.1), (1, 0.1, 0.5, 0.0, 0.0)):
        with pytest.raises(ValueError):
            r.bake_lightmap(4, 4, 1, filter=bad)
    with pytest.raises(ValueError):
        r.filter_lightmap(np.zeros((4, 4, 3), F), pts, 1, 0.1, 0.5)
    with pytest.raises(ValueError):
        r.filter_lightmap(img, np.zeros((2, 7), F), 1, 0.1, 0.5)


def test_cli_refuses_a_bad_filter_before_anything_else():
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    for args, text in ((["--bake-lightmap", "8x8", "--filter", "9"], "bad --filter 9"), (["--bake-lightmap", "8x8", "--filter", "2,-1"], "bad --filter"),
                       (["--bake-lightmap", "8x8", "--filter", "2,0.1,0.5,0.1,7"], "bad --filter"), (["--bake-lightmap", "8x8", "--filter", "2,"], "bad --filter"),
                       (["--bake-lightmap", "8x8", "--filter", "x"], "bad --filter"), (["--filter", "3"], "--filter without --bake-lightmap"),
                       (["--bake-lightmap", "8x8", "--device-bvh", "--filter", "3"], "needs its sigma_position")):
        r = subprocess.run([exe] + args + ["synthetic:cbox"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr[:200])


def test_filter_kernels_use_no_scratch():
    """The compiler's resource report of api/lightmap_filter.hip, as `make` put it into the library's report between the lines
    '# lightmap_filter.hip' and '# lightmap.hip': the three kernels are there, none has scratch, all reach 8 waves a SIMD, and only
    the LDS form has LDS - 40 bytes for each of the (32 + 4) x (8 + 4) cells of a tile and its apron."""
    text = open(os.path.join(ROOT, "hijiki_amd", "lib", "resource_usage.txt")).read()
    assert "\n# lightmap_filter.hip\n" in text and "\n# lightmap.hip\n" in text
    section = text.split("\n# lightmap_filter.hip\n", 1)[1]
    assert "\n# lightmap.hip\n" in section
    report = _report(section.split("\n# lightmap.hip\n", 1)[0])
    names = {k.split("(")[0].split("::")[-1]: v for k, v in report.items()}
    assert sorted(names) == ["k_lm_filter_direct", "k_lm_filter_lds", "k_lm_guide"], sorted(report)
    for k, v in names.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["Occupancy"] == 8, (k, v)
        assert v["LDS Size"] == (36 * 12 * 40 if k == "k_lm_filter_lds" else 0), (k, v)
