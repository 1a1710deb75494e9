"""hj_lightmap_texels / hj_bake_lightmap, the part that needs no GPU: the reference of the GPU tests (lightmap_ref) against exact
rational arithmetic; the partition of a quad by its two triangles; both windings; the dilation on a hand-made image; every argument
refusal before the device is touched, writing nothing; the ABI mirror against the header; the compiler's resource report."""
import ctypes as C
import os
import subprocess
from fractions import Fraction as Q

import numpy as np
import pytest

import lightmap_ref as LR
import lightmap_scenes as LS
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
NONE = LR.NONE


def exact_owner(tri_uv, W, H):
    """coverage and owner in exact rational arithmetic: tri_uv (n, 3, 2) of exactly representable values"""
    owner = np.full((H, W), NONE, U)
    for i in reversed(range(len(tri_uv))):
        a, b, c = [(Q(float(p[0])), Q(float(p[1]))) for p in tri_uv[i]]
        edge = lambda s, t, p: (t[0] - s[0]) * (p[1] - s[1]) - (t[1] - s[1]) * (p[0] - s[0])  # noqa: E731
        for y in range(H):
            for x in range(W):
                p = (Q(2 * x + 1, 2 * W), Q(2 * y + 1, 2 * H))
                if not (min(a[0], b[0], c[0]) <= p[0] <= max(a[0], b[0], c[0]) and min(a[1], b[1], c[1]) <= p[1] <= max(a[1], b[1], c[1])):
                    continue
                e = (edge(b, c, p), edge(c, a, p), edge(a, b, p))
                if (all(v >= 0 for v in e) or all(v <= 0 for v in e)) and sum(e) != 0:
                    owner[y, x] = i
    return owner


def mesh(tri_uv):
    """(triangles, vertices) with the given uv, positions from the uv, normals +y"""
    uv = np.asarray(tri_uv, F).reshape(-1, 2)
    v = np.zeros((len(uv), 8), F)
    v[:, 0], v[:, 2], v[:, 3], v[:, 7], v[:, 5] = uv[:, 0], uv[:, 1], uv[:, 0], uv[:, 1], 1.0
    return np.arange(len(uv)).reshape(-1, 3), v


def test_entry_points_are_declared_listed_and_exported():
    for name in ("hj_lightmap_texels", "hj_bake_lightmap"):
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001000
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    assert "#define HJ_LIGHTMAP_DEVICE_ARRAYS 1u" in header and "#define HJ_LIGHTMAP_MAX_GUTTER 64u" in header
    assert (abi.LIGHTMAP_DEVICE_ARRAYS, abi.LIGHTMAP_MAX_GUTTER, abi.LIGHTMAP_NONE) == (1, 64, 0xFFFFFFFF)
    assert "3.14159274f" in header and LR.PI == F(np.pi)
    assert callable(device.Renderer.lightmap_texels) and callable(device.Renderer.bake_lightmap)


def test_abi_mirror_matches_the_header(tmp_path):
    """size and field offsets of hj_lightmap_desc as a C compiler lays the header's struct out"""
    names = [n for n, _ in abi.LightmapDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hijiki_hip.h"\nint main(void) {\n  printf("%zu", sizeof(hj_lightmap_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(hj_lightmap_desc, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.LightmapDesc)] + [getattr(abi.LightmapDesc, n).offset for n in names], got
    assert got[0] == 32 and names == ["width", "height", "first_triangle", "num_triangles", "seed", "seed_stride", "offset", "flags"]


@pytest.mark.parametrize("W,H", [(8, 8), (16, 4), (32, 64)])
def test_reference_is_exact_rational_arithmetic_on_dyadic_uv(W, H):
    """uv that are multiples of 1/64 on atlases whose sizes are powers of two: centres, differences and products are exact in
    float32, so the float32 reference must reproduce the rational predicate texel for texel - edges and vertices on centres,
    overlaps, zero-area and collinear footprints, triangles that stick out of [0, 1]^2 included."""
    rng = np.random.default_rng([W, H])
    tri_uv = rng.integers(-16, 81, (30, 3, 2)).astype(np.float64) / 64.0
    tri_uv[0] = [[0.25, 0.25], [0.75, 0.25], [0.75, 0.75]]
    tri_uv[1] = [[0.25, 0.25], [0.75, 0.75], [0.25, 0.75]]
    tri_uv[2] = [[0.5, 0.5], [0.5, 0.5], [0.5, 0.5]]
    tri_uv[3] = [[0.0, 0.0], [0.5, 0.5], [1.0, 1.0]]
    tri_uv[4] = [[1 / 64, 3 / 64], [33 / 64, 3 / 64], [17 / 64, 35 / 64]]
    want = exact_owner(tri_uv, W, H)
    got = LR.coverage_owner(*mesh(tri_uv), W, H)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (want != NONE).sum() > W * H // 4 and len(np.unique(want)) > 5
    for i in (0, 7, 19):                                                # coverage triangle by triangle, not only through the owner
        ys, xs, mask = LR.covers(tri_uv[i].astype(F), W, H)
        alone = np.zeros((H, W), bool)
        alone[np.ix_(ys, xs)] = mask
        assert np.array_equal(alone, exact_owner(tri_uv[i:i + 1], W, H) == 0)


def test_a_quads_two_triangles_own_every_texel_once():
    """The two triangles of a quad that share a diagonal through texel centres: every texel of the quad has exactly one owner, the
    diagonal's texels belong to the lower index, and nothing outside the quad is owned."""
    W = H = 64
    c = lambda x, y: (x / 64.0, y / 64.0)  # noqa: E731
    quad = [[c(8, 8), c(24, 8), c(24, 24)], [c(8, 8), c(24, 24), c(8, 24)]]
    tri, vt = mesh(quad)
    cover = []
    for t in quad:
        ys, xs, mask = LR.covers(np.array(t, F), W, H)
        full = np.zeros((H, W), bool)
        full[np.ix_(ys, xs)] = mask
        cover.append(full)
    inside = np.zeros((H, W), bool)
    inside[8:24, 8:24] = True
    assert np.array_equal(cover[0] | cover[1], inside)
    both = cover[0] & cover[1]
    assert np.array_equal(np.argwhere(both), np.stack([np.arange(8, 24)] * 2, 1))      # shared: exactly the diagonal's centres
    pts, owner = LR.texels(tri, vt, W, H)
    assert np.array_equal(owner != NONE, inside) and (owner[both] == 0).all() and len(pts) == 256
    assert (owner[8:24, 8:24][np.triu_indices(16, 1)] == 0).all() and (owner[8:24, 8:24][np.tril_indices(16, -1)] == 1).all()   # [y, x]
    swapped = LR.coverage_owner(tri[::-1], vt, W, H)                                   # the other triangle first: it takes the diagonal
    assert (swapped[both] == 0).all() and np.array_equal(swapped != NONE, inside)
    assert np.array_equal(pts.view(U)[:, 7], np.flatnonzero(inside.ravel()))


def test_both_windings_cover_the_same_texels():
    """On uv and centres that float32 holds exactly (multiples of 1/64, power-of-two atlases) every order of the three vertices
    gives the same coverage.  (For uv of any value this is not claimed bit for bit: the edge values of the two windings are
    anchored at different vertices and round differently within an ulp of an edge.)"""
    rng = np.random.default_rng(3)
    for k in range(60):
        uv = (rng.integers(-8, 73, (3, 2)) / 64.0).astype(F)
        for W, H in ((64, 64), (32, 16)):
            a = LR.covers(uv, W, H)
            for order in ([2, 1, 0], [1, 2, 0], [0, 2, 1]):
                assert all(np.array_equal(p, q) for p, q in zip(a, LR.covers(uv[order], W, H))), (k, uv, order)


def test_edge_scene_holds_what_it_claims():
    cs, case = LS.edge_scene()
    tri, vt = cs.triangles, cs.vertices
    assert 38 <= len(tri) <= 45
    pts, owner = LR.texels(tri, vt, 64, 64)
    by_cover = LR.coverage_owner(tri, vt, 64, 64)
    owned = lambda name: int((owner == case[name]).sum())  # noqa: E731
    for name in ("wholly outside", "zero area", "collinear", "collinear through centres", "nan uv", "inf uv", "zero normals"):
        assert owned(name) == 0, name
    assert (by_cover == case["zero normals"]).sum() > 20                                # covered, then dropped for the normal
    dropped = (by_cover == case["cancelling normals"]) & (owner == NONE)
    assert owned("cancelling normals") > 30 and np.array_equal(np.argwhere(dropped)[:, 1], np.full(dropped.sum(), 44)) and dropped.sum() >= 3
    assert owned("partly outside") > 0 and owned("quad lower") + owned("quad upper") == 256
    assert owner[8, 40] == case["vertex on a centre"] and owner[8, 50] == case["vertex on a centre"]
    low, high = LR.covers(vt[tri[case["overlap low"]]][:, [3, 7]], 64, 64), LR.covers(vt[tri[case["overlap high"]]][:, [3, 7]], 64, 64)
    a, b = np.zeros((64, 64), bool), np.zeros((64, 64), bool)
    a[np.ix_(low[0], low[1])], b[np.ix_(high[0], high[1])] = low[2], high[2]
    assert (a & b).sum() > 30 and (owner[a & b] <= case["overlap low"]).all()
    sl = np.argwhere(by_cover == case["sliver"])
    assert len(sl) >= 5 and len(np.unique(sl[:, 1])) == len(sl)                          # a texel here and there along its 53 columns
    assert np.isfinite(pts[:, 0:6]).all() and (pts[:, 3:6] != 0).any(axis=1).all() and len(pts) == (owner != NONE).sum()


def test_dilation_on_a_hand_made_image():
    img = np.zeros((5, 6, 4), F)
    img[2, 2] = [1, 2, 3, 1]
    img[2, 3] = [3, 2, 1, 1]
    one = LR.dilate(img)
    assert np.array_equal(one[1, 2], F([2, 2, 2, 0.5])) and np.array_equal(one[1, 1], F([1, 2, 3, 0.5])) and np.array_equal(one[3, 4], F([3, 2, 1, 0.5]))
    assert np.array_equal(one[2, 2], img[2, 2]) and (one[0] == 0).all() and (one[:, 0] == 0).all() and (one[:, 5] == 0).all()
    two = LR.dilate(one)
    assert two[0, 1, 3] == 0.5 and two[2, 5, 3] == 0.5 and np.array_equal(two[1:4, 1:5], one[1:4, 1:5])
    assert np.array_equal(two[0, 0], F([1, 2, 3, 0.5]))                                  # its one neighbour with alpha > 0: (1, 1)
    corner = np.zeros((2, 2, 4), F)
    corner[0, 0] = [4, 4, 4, 1]
    assert (LR.dilate(corner)[:, :, 3] == F([[1, 0.5], [0.5, 0.5]])).all()              # neighbours outside the atlas do not exist


def _desc(**kw):
    d = abi.LightmapDesc(16, 8, 0, 0, 0, 1, 0.0, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_refusals_come_before_the_device():
    """Each refusal: its status, a message that names the entry point, and nothing written - points, owner, count, image, statistics."""
    L = device.lib()
    INV, DEV = abi.HJ_ERR_INVALID, abi.LIGHTMAP_DEVICE_ARRAYS
    pts, own, img = np.full((128, 8), 7.0, F), np.full(128, 7, U), np.full((8, 16, 4), 7.0, F)
    count, st = C.c_size_t(77), abi.RenderStats()
    o0 = abi.RenderOpts.default()
    o0.max_bounces = 0
    o1 = abi.RenderOpts.default()
    o1.use_bvh = 0
    bad_desc = {"unknown flag bits": _desc(flags=2), "width 0": _desc(width=0), "height 0": _desc(height=0), "width above 16384": _desc(width=16385),
                "more than 2^26 texels": _desc(width=16384, height=8192), "a NaN offset": _desc(offset=float("nan")),
                "an infinite offset": _desc(offset=float("-inf"))}
    texels = {k: (INV, (C.byref(d), pts.ctypes.data, 128, own.ctypes.data, C.byref(count))) for k, d in bad_desc.items()}
    texels["null desc"] = (INV, (None, pts.ctypes.data, 128, own.ctypes.data, C.byref(count)))
    texels["null out_count"] = (INV, (C.byref(_desc()), pts.ctypes.data, 128, own.ctypes.data, None))
    texels["misaligned device points"] = (INV, (C.byref(_desc(flags=DEV)), pts.ctypes.data + 4, 127, None, C.byref(count)))
    texels["misaligned device owner"] = (INV, (C.byref(_desc(flags=DEV)), None, 0, own.ctypes.data + 8, C.byref(count)))
    bake = {k: (INV, (C.byref(d), 4, 2, None, img.ctypes.data, C.byref(count), C.byref(st))) for k, d in bad_desc.items()}
    bake["null desc"] = (INV, (None, 4, 2, None, img.ctypes.data, C.byref(count), C.byref(st)))
    bake["null image"] = (INV, (C.byref(_desc()), 4, 2, None, None, C.byref(count), C.byref(st)))
    bake["spp 0"] = (INV, (C.byref(_desc()), 0, 2, None, img.ctypes.data, C.byref(count), C.byref(st)))
    bake["spp above 65536"] = (INV, (C.byref(_desc()), 65537, 2, None, img.ctypes.data, C.byref(count), C.byref(st)))
    bake["gutter above 64"] = (INV, (C.byref(_desc()), 4, 65, None, img.ctypes.data, C.byref(count), C.byref(st)))
    bake["misaligned device image"] = (INV, (C.byref(_desc(flags=DEV)), 4, 2, None, img.ctypes.data + 4, C.byref(count), C.byref(st)))
    bake["max_bounces 0"] = (INV, (C.byref(_desc()), 4, 2, C.byref(o0), img.ctypes.data, C.byref(count), C.byref(st)))
    bake["use_bvh 0"] = (abi.HJ_ERR_UNSUPPORTED, (C.byref(_desc()), 4, 2, C.byref(o1), img.ctypes.data, C.byref(count), C.byref(st)))
    for fn, cases in ((L.hj_lightmap_texels, texels), (L.hj_bake_lightmap, bake)):
        for name, (status, args) in cases.items():
            L.hj_context_create(-1, None)                              # (leaves ITS text in hj_last_error(NULL))
            before = L.hj_last_error(None)
            assert fn(None, *args) == status, (fn.__name__, name)
            text = L.hj_last_error(None)
            assert text and text != before and fn.__name__.encode() in text, (name, text)
    assert (pts == 7.0).all() and (own == 7).all() and (img == 7.0).all() and count.value == 77
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)
    # two faults in one call: the earlier check's message
    assert L.hj_bake_lightmap(None, C.byref(_desc(width=0)), 0, 99, None, img.ctypes.data, None, None) == INV and b"atlas" in L.hj_last_error(None)
    assert L.hj_bake_lightmap(None, C.byref(_desc()), 0, 99, None, img.ctypes.data, None, None) == INV and b"spp" in L.hj_last_error(None)
    assert L.hj_bake_lightmap(None, C.byref(_desc()), 1, 99, C.byref(o0), img.ctypes.data, None, None) == INV and b"gutter" in L.hj_last_error(None)


def test_a_valid_call_without_a_context():
    """A process without a HIP device cannot hold a context: the valid call it can make gets HJ_ERR_DEVICE; with a device, a null
    context is HJ_ERR_INVALID.  Nothing is written either way."""
    L = device.lib()
    count, img = C.c_size_t(77), np.full((8, 16, 4), 7.0, F)
    for rc in (L.hj_lightmap_texels(None, C.byref(_desc()), None, 0, None, C.byref(count)),
               L.hj_bake_lightmap(None, C.byref(_desc(offset=1e-3)), 4, 0, None, img.ctypes.data, C.byref(count), None)):
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert count.value == 77 and (img == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    for kw in (dict(width=0, height=4), dict(width=4, height=16385), dict(width=16384, height=8192), dict(width=4, height=4, offset=float("nan")),
               dict(width=4, height=4, seed=-1), dict(width=4, height=4, seed_stride=1 << 32), dict(width=4, height=4, first_triangle=-2)):
        with pytest.raises(ValueError):
            r.lightmap_texels(**kw)
        with pytest.raises(ValueError):
            r.bake_lightmap(spp=1, **kw)
    for kw in (dict(spp=0), dict(spp=65537), dict(spp=1, gutter=65), dict(spp=1, gutter=-1)):
        with pytest.raises(ValueError):
            r.bake_lightmap(4, 4, **kw)


def test_lightmap_kernels_use_no_scratch():
    """The compiler's resource report of api/lightmap.hip, as `make` appended it to the library's report behind the line
    '# lightmap.hip': all seven kernels are there, none has scratch, and only the count, scan and emit kernels have LDS."""
    text = open(os.path.join(ROOT, "hijiki_amd", "lib", "resource_usage.txt")).read()
    assert "\n# lightmap.hip\n" in text
    report = _report(text.split("\n# lightmap.hip\n", 1)[1])
    names = {k.split("(")[0].split("::")[-1]: v for k, v in report.items()}
    assert sorted(names) == ["k_lm_count", "k_lm_dilate", "k_lm_emit", "k_lm_owner", "k_lm_owner_wide", "k_lm_scan", "k_lm_scatter"], sorted(report)
    for k, v in names.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert (v["LDS Size"] != 0) == (k in ("k_lm_count", "k_lm_scan", "k_lm_emit")), (k, v)
