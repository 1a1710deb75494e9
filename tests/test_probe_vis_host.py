"""hj_probe_visibility_rays / hj_bake_probe_visibility / hj_sample_probes_visible, the part that needs no GPU: the symbols are
declared, listed and exported and the ABI mirror has the header's layout; every argument refusal comes before the device is touched,
in the stated order, with a message, and writes nothing; the reference of the GPU tests (probe_vis_ref) maps a ray back into the
texel it was drawn in, its border rule is the header's and makes the bilinear fetch continuous across the octahedral map's edges and
corners, and with both factors off it is probe_ref.sample; the compiler's resource report of the unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import probe_ref as P
import probe_vis_ref as V
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_probe_visibility_rays", "hj_bake_probe_visibility", "hj_sample_probes_visible")
INF, NAN = float("inf"), float("nan")
DEV, NOB, NOC = abi.PROBE_VIS_DEVICE_ARRAYS, abi.PROBE_VIS_NO_BACKFACE, abi.PROBE_VIS_NO_CHEBYSHEV
_desc, _vis = P.abi_desc, V.abi_vis


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001400
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_PROBE_VIS_DEVICE_ARRAYS 1u", "#define HJ_PROBE_VIS_NO_BACKFACE 2u", "#define HJ_PROBE_VIS_NO_CHEBYSHEV 4u",
                 "#define HJ_PROBE_VIS_WORDS(res) (2u * ((res) + 2u) * ((res) + 2u))", "0.2f", "0.05f"):
        assert text in header, text
    slab = int(re.search(r"#define HJ_PROBE_VIS_SLAB_RAYS (\d+)u", header).group(1))
    assert slab == abi.PROBE_VIS_SLAB_RAYS and slab >= 16 * 16 * 64
    assert (DEV, NOB, NOC) == (1, 2, 4) and abi.PROBE_VIS_RES == (4, 8, 16)
    assert [abi.probe_vis_words(r) for r in (4, 8, 16)] == [72, 200, 648] == [V.words(r) for r in (4, 8, 16)]
    assert all(abi.probe_vis_words(r) * 4 % 16 == 0 for r in abi.PROBE_VIS_RES)
    for fn in ("probe_visibility_rays", "bake_probe_visibility", "sample_probes_visible"):
        assert callable(getattr(device.Renderer, fn))


def test_abi_mirror_matches_the_header(tmp_path):
    """size and field offsets of hj_probe_vis_desc as a C compiler lays the header's struct out, and the macro's values"""
    names = [n for n, _ in abi.ProbeVisDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hijiki_hip.h"\nint main(void) {\n  printf("%zu", sizeof(hj_probe_vis_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(hj_probe_vis_desc, {n}));\n' for n in names)
                   + '  printf(" %u %u %u %u", HJ_PROBE_VIS_WORDS(4u), HJ_PROBE_VIS_WORDS(8u), HJ_PROBE_VIS_WORDS(16u), HJ_PROBE_VIS_SLAB_RAYS);\n'
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got[:-4] == [C.sizeof(abi.ProbeVisDesc)] + [getattr(abi.ProbeVisDesc, n).offset for n in names], got
    assert got[0] == 20 and names == ["res", "rays_per_texel", "max_distance", "normal_bias", "flags"]
    assert got[-4:] == [72, 200, 648, abi.PROBE_VIS_SLAB_RAYS]


# -------------------------------------------------------------------------------------------------------------------- refusals

def _calls():
    """-> the three entry points as functions of (desc or None, vis or None, keywords), each over arrays this returns too"""
    L = device.lib()
    buf = dict(rays=np.full((8 * 16 * 2, 8), 7.0, F), atlas=np.full((8, 72), 7.0, F), volume=np.full((8, 28), 7.0, F), spts=np.zeros((4, 8), F),
               out=np.full((4, 4), 7.0, F))
    buf["spts"][:, 4] = 1.0
    ref = lambda s: C.byref(s) if s is not None else None                                    # noqa: E731

    def rays(d, v, first=0, num=8, rays=buf["rays"], **_):
        return L.hj_probe_visibility_rays(None, ref(d), ref(v), first, num, _p(rays))

    def bake(d, v, atlas=buf["atlas"], **_):
        return L.hj_bake_probe_visibility(None, ref(d), ref(v), _p(atlas))

    def sample(d, v, probes=buf["volume"], atlas=buf["atlas"], spts=buf["spts"], m=4, out=buf["out"], **_):
        return L.hj_sample_probes_visible(None, ref(d), ref(v), _p(probes), _p(atlas), _p(spts), m, _p(out))
    return {"hj_probe_visibility_rays": rays, "hj_bake_probe_visibility": bake, "hj_sample_probes_visible": sample}, buf


def _refused(call, name, word, *args, **kw):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call(*args, **kw) == abi.HJ_ERR_INVALID, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and name.encode() in text and word in text, (name, word, text)


# what every call refuses of the probe desc (probe_volume's own refusals, in its order), then of the visibility desc
DESC_REFUSALS = [(b"flag bits", dict(flags=2)), (b"count", dict(count=(2, 0, 2))), (b"count", dict(count=(1024, 1024, 5))), (b"origin", dict(origin=(0, NAN, 0))),
                 (b"spacing", dict(spacing=(1, 0, 1))), (b"spacing", dict(spacing=(INF, 1, 1))), (b"min_distance", dict(min_distance=-1.0))]
VIS_REFUSALS = [(b"flag bits", dict(flags=8)), (b"flag bits", dict(flags=0x80000000 | NOB)), (b"must agree", dict(flags=DEV)),
                (b"res", dict(res=0)), (b"res", dict(res=5)), (b"res", dict(res=32)), (b"res", dict(res=2))]
BAKE_REFUSALS = [(b"rays_per_texel", dict(rays_per_texel=0)), (b"rays_per_texel", dict(rays_per_texel=65)), (b"max_distance", dict(max_distance=0.0)),
                 (b"max_distance", dict(max_distance=-1.0)), (b"max_distance", dict(max_distance=NAN)), (b"max_distance", dict(max_distance=INF)),
                 (b"max_distance", dict(max_distance=2e18))]
LOOKUP_REFUSALS = [(b"normal_bias", dict(normal_bias=-0.5)), (b"normal_bias", dict(normal_bias=NAN)), (b"normal_bias", dict(normal_bias=INF))]


def test_argument_refusals_come_before_the_device():
    calls, buf = _calls()
    for name, call in calls.items():
        _refused(call, name, b"null desc", None, _vis())
        _refused(call, name, b"null vis", _desc(), None)
        for word, dkw in DESC_REFUSALS:
            _refused(call, name, word, _desc(**dkw), _vis())
        for word, vkw in VIS_REFUSALS:
            _refused(call, name, word, _desc(), _vis(**vkw))
        _refused(call, name, b"must agree", _desc(flags=abi.PROBES_DEVICE_ARRAYS), _vis())
        for word, vkw in (LOOKUP_REFUSALS if name == "hj_sample_probes_visible" else BAKE_REFUSALS):
            _refused(call, name, word, _desc(), _vis(**vkw))
    rays, bake, sample = calls["hj_probe_visibility_rays"], calls["hj_bake_probe_visibility"], calls["hj_sample_probes_visible"]
    on = (_desc(flags=abi.PROBES_DEVICE_ARRAYS), )
    _refused(rays, "hj_probe_visibility_rays", b"null rays", _desc(), _vis(), rays=None)
    _refused(rays, "hj_probe_visibility_rays", b"probes 1 ... 9 of 8", _desc(), _vis(), first=1, num=8)
    _refused(rays, "hj_probe_visibility_rays", b"probes", _desc(), _vis(), first=0xFFFFFFFF, num=2)
    _refused(rays, "hj_probe_visibility_rays", b"aligned", *on, _vis(flags=DEV), rays=buf["rays"].ctypes.data + 4)
    _refused(bake, "hj_bake_probe_visibility", b"null atlas", _desc(), _vis(), atlas=None)
    _refused(bake, "hj_bake_probe_visibility", b"aligned", *on, _vis(flags=DEV), atlas=buf["atlas"].ctypes.data + 8)
    for missing in ("probes", "atlas", "spts", "out"):
        _refused(sample, "hj_sample_probes_visible", b"null " + {"spts": b"points"}.get(missing, missing.encode()), _desc(), _vis(), **{missing: None})
    _refused(sample, "hj_sample_probes_visible", b"null atlas", _desc(), _vis(flags=NOB), atlas=None)
    _refused(sample, "hj_sample_probes_visible", b"null atlas", _desc(), _vis(flags=NOC), atlas=None)
    for where in ("probes", "atlas", "spts", "out"):
        a = buf["volume" if where == "probes" else where]
        _refused(sample, "hj_sample_probes_visible", b"aligned", *on, _vis(flags=DEV), **{where: a.ctypes.data + 4})
    _refused(sample, "hj_sample_probes_visible", b"points, at most", _desc(), _vis(), m=0x80000000)

    def bad(word, *v):
        p = buf["spts"].copy()
        p[2, word:word + len(v)] = v
        return p
    for p in (bad(1, NAN), bad(0, -INF), bad(3, NAN, 0, 1), bad(5, INF), bad(3, 0, 0, 0), bad(3, -0.0, -0.0, 0)):
        _refused(sample, "hj_sample_probes_visible", b"point 2", _desc(), _vis(), spts=p)
    assert all((buf[k] == 7.0).all() for k in ("rays", "atlas", "volume", "out"))


def test_refusals_come_in_the_stated_order():
    """Two faults in one call: the earlier check's message.  Each refusal is paired with everything behind it."""
    calls, buf = _calls()
    L = device.lib()
    order = [("flag bits", "d", dict(flags=2)), ("count", "d", dict(count=(0, 1, 1))), ("origin", "d", dict(origin=(NAN, 0, 0))),
             ("spacing", "d", dict(spacing=(0, 1, 1))), ("min_distance", "d", dict(min_distance=-1.0)),
             ("visibility flag bits", "v", dict(flags=8)), ("res", "v", dict(res=3))]
    tail = {"hj_sample_probes_visible": [("normal_bias", "v", dict(normal_bias=-1.0))]}
    both = [("rays_per_texel", "v", dict(rays_per_texel=0)), ("max_distance", "v", dict(max_distance=0.0))]
    odd = buf["rays"].ctypes.data + 4
    for name, call in calls.items():
        steps = order + tail.get(name, both)
        for i in range(len(steps)):
            kw = {"d": {}, "v": {}}
            for _, which, k in steps[i:]:
                kw[which].update(k)
            # behind the descs: a probe window past the end, an m that is too large
            assert call(_desc(**kw["d"]), _vis(**kw["v"]), first=5, num=8, m=0x80000000) == abi.HJ_ERR_INVALID
            assert steps[i][0].encode() in L.hj_last_error(None), (name, steps[i][0], L.hj_last_error(None))
        assert call(None, None, rays=None, atlas=None, probes=None) == abi.HJ_ERR_INVALID and b"null desc" in L.hj_last_error(None)
        assert call(_desc(flags=2), _vis(res=3), rays=None, atlas=None, probes=None) == abi.HJ_ERR_INVALID and b"null" in L.hj_last_error(None)
    on = _desc(flags=abi.PROBES_DEVICE_ARRAYS)
    # the flags' agreement stands between the unknown bits and res
    for name, call in calls.items():
        assert call(on, _vis(flags=8)) == abi.HJ_ERR_INVALID and b"flag bits" in L.hj_last_error(None)
        assert call(on, _vis(res=3)) == abi.HJ_ERR_INVALID and b"must agree" in L.hj_last_error(None)
    rays, sample = calls["hj_probe_visibility_rays"], calls["hj_sample_probes_visible"]
    assert rays(on, _vis(flags=DEV, max_distance=-1.0), first=5, num=8, rays=odd) == abi.HJ_ERR_INVALID and b"max_distance" in L.hj_last_error(None)
    assert rays(on, _vis(flags=DEV), first=5, num=8, rays=odd) == abi.HJ_ERR_INVALID and b"probes 5" in L.hj_last_error(None)
    assert rays(on, _vis(flags=DEV), rays=odd) == abi.HJ_ERR_INVALID and b"aligned" in L.hj_last_error(None)
    zero = buf["spts"].copy()
    zero[0, 3:6] = 0
    assert sample(on, _vis(flags=DEV), probes=odd, m=0x80000000) == abi.HJ_ERR_INVALID and b"aligned" in L.hj_last_error(None)
    assert sample(on, _vis(flags=DEV), m=0x80000000) == abi.HJ_ERR_INVALID and b"at most" in L.hj_last_error(None)
    assert sample(_desc(), _vis(), spts=zero, m=0x80000000) == abi.HJ_ERR_INVALID and b"at most" in L.hj_last_error(None)
    assert sample(_desc(), _vis(), spts=zero) == abi.HJ_ERR_INVALID and b"normal" in L.hj_last_error(None)
    assert all((buf[k] == 7.0).all() for k in ("rays", "atlas", "volume", "out"))


def test_a_valid_call_without_a_context_is_refused_last():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none: also with what a call
    does not use out of its domain (the look-up's bias for the bake, the bake's rays for the look-up), with both NO_ flags and no
    atlas, and with nothing to do."""
    calls, buf = _calls()
    L = device.lib()
    rays, bake, sample = calls["hj_probe_visibility_rays"], calls["hj_bake_probe_visibility"], calls["hj_sample_probes_visible"]
    for name, go in (("hj_probe_visibility_rays", lambda: rays(_desc(), _vis(normal_bias=-1.0, flags=NOB | NOC), first=3, num=5)),
                     ("hj_probe_visibility_rays", lambda: rays(_desc(), _vis(), first=8, num=0, rays=None)),
                     ("hj_bake_probe_visibility", lambda: bake(_desc(), _vis(res=4, rays_per_texel=64, max_distance=1e18, normal_bias=NAN))),
                     ("hj_sample_probes_visible", lambda: sample(_desc(), _vis(rays_per_texel=0, max_distance=NAN))),
                     ("hj_sample_probes_visible", lambda: sample(_desc(), _vis(res=16, flags=NOB | NOC), atlas=None)),
                     ("hj_sample_probes_visible", lambda: sample(_desc(), _vis(), m=0, probes=None, atlas=None, spts=None, out=None))):
        rc = go()
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None) and name.encode() in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert all((buf[k] == 7.0).all() for k in ("rays", "atlas", "volume", "out"))


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2))
    for kw in (dict(res=5), dict(res=32), dict(rays_per_texel=0), dict(rays_per_texel=65), dict(max_distance=0.0), dict(max_distance=NAN),
               dict(max_distance=1e19), dict(count=(0, 1, 1)), dict(spacing=(1, 0, 1)), dict(seed=-1)):
        with pytest.raises(ValueError):
            r.bake_probe_visibility(**dict(good, **kw))
        with pytest.raises(ValueError):
            r.probe_visibility_rays(**dict(good, **kw))
    for kw in (dict(first_probe=-1), dict(first_probe=8, num_probes=1), dict(first_probe=4, num_probes=5)):
        with pytest.raises(ValueError):
            r.probe_visibility_rays(**dict(good, **kw))
    vol, pts, atlas = np.zeros((2, 2, 2, 28), F), np.zeros((3, 8), F), np.zeros((2, 2, 2, 10, 10, 2), F)
    pts[:, 5] = 1.0
    for a, kw in ((np.zeros((2, 2, 2, 10, 10), F), {}), (np.zeros((2, 2, 3, 10, 10, 2), F), {}), (np.zeros((2, 2, 2, 10, 8, 2), F), {}),
                  (np.zeros((2, 2, 2, 9, 9, 2), F), {}), (None, {}), (None, dict(backface=False)), (atlas, dict(normal_bias=-1.0)), (atlas, dict(normal_bias=NAN))):
        with pytest.raises(ValueError):
            r.sample_probes_visible(vol, a, (0, 0, 0), (1, 1, 1), pts, **kw)
    bad = pts.copy()
    bad[1, 3:6] = 0
    with pytest.raises(ValueError):
        r.sample_probes_visible(vol, atlas, (0, 0, 0), (1, 1, 1), bad)


# ------------------------------------------------------------------------------------------------------- the reference's own checks

def test_border_rule_is_the_headers():
    """border_source at res 4, by hand from the header's rule: border (i + 1, 0) <- interior (3 - i, 0), (i + 1, 5) <- (3 - i, 3),
    (0, j + 1) <- (0, 3 - j), (5, j + 1) <- (3, 3 - j), corners <- the diagonally opposite interior corner."""
    want = [[15, 3, 2, 1, 0, 12], [12, 0, 1, 2, 3, 15], [8, 4, 5, 6, 7, 11], [4, 8, 9, 10, 11, 7], [0, 12, 13, 14, 15, 3], [3, 15, 14, 13, 12, 0]]
    assert V.border_source(4).reshape(6, 6).tolist() == want
    for res in (8, 16):
        src, T = V.border_source(res).reshape(res + 2, res + 2), res + 2
        assert (src[1:-1, 1:-1] == np.arange(res * res).reshape(res, res)).all()
        for i in range(res):
            assert src[0, i + 1] == res - 1 - i and src[T - 1, i + 1] == (res - 1) * res + res - 1 - i
            assert src[i + 1, 0] == (res - 1 - i) * res and src[i + 1, T - 1] == (res - 1 - i) * res + res - 1
        assert [src[0, 0], src[0, T - 1], src[T - 1, 0], src[T - 1, T - 1]] == [res * res - 1, (res - 1) * res, res - 1, 0]
    # reduce: two probes, res 4, s = 3, by hand for one texel; a miss and a clamp count as max_distance
    v = V.vis(4, 3, 2.0)
    ids, t = np.zeros(2 * 16 * 3, np.int32), np.arange(2 * 16 * 3, dtype=F) * F(0.125)
    ids[3] = -1
    atlas = V.reduce((ids, t), v)
    assert atlas.shape == (2, 6, 6, 2)
    a1 = (F(2.0) + F(0.5)) + F(0.625)                                   # texel (1, 0): rays 3 (t = 0.375, but a miss), 4, 5
    a2 = (F(2.0) * F(2.0) + F(0.5) * F(0.5)) + F(0.625) * F(0.625)
    assert atlas[0, 1, 2].tolist() == [a1 / F(3), a2 / F(3)] and atlas[0, 0, 3].tolist() == atlas[0, 1, 2].tolist()
    assert (atlas[1, 1:-1, 1:-1] == [2.0, 4.0]).all()                   # probe 1: every t beyond max_distance


@pytest.mark.parametrize("res", [4, 8, 16])
def test_a_ray_encodes_back_into_its_texel(res):
    """encode(normalize(decode(...))) of a draw lands in the texel the draw was made in: 4096 draws of a fixed seed; draws with u or v
    within 1e-3 of a texel edge are left out (there rounding may cross the edge), and they are at most 1 % of all."""
    d = P.desc((0, 0, 0), (1, 1, 1), (1, 1, 1), seed=12345, seed_stride=1)
    s = 4096 // (res * res)
    v = V.vis(res, s, 1.0)
    p, tx, ty, u, w = V.draws(d, v, 0, 1)
    assert len(u) == 4096 and (u >= 0).all() and (u < 1).all() and (w >= 0).all() and (w < 1).all()
    ex, ey = V.square(tx, ty, u, w, res)
    px, py = V.encode(V.normalize3(V.decode(ex, ey)))
    keep = (np.minimum(u, 1 - u) >= 1e-3) & (np.minimum(w, 1 - w) >= 1e-3)
    print(f"res {res}: {int((~keep).sum())} of 4096 draws within 1e-3 of an edge")
    assert (~keep).mean() <= 0.01
    # the nearest interior texel: the atlas coordinate c has texel t's centre at t + 1
    gx = np.floor(V.texel_coordinate(px, res) - F(0.5)).astype(np.int64)
    gy = np.floor(V.texel_coordinate(py, res) - F(0.5)).astype(np.int64)
    assert (gx[keep] == tx[keep]).all() and (gy[keep] == ty[keep]).all()
    assert np.abs(px - ex).max() <= 1e-5 and np.abs(py - ey).max() <= 1e-5    # (and the round trip itself, to a few ulps of 1)


@pytest.mark.parametrize("res", [4, 8, 16])
def test_border_makes_the_fetch_continuous_across_the_edges(res):
    """An atlas filled from a smooth function of direction, f(dir) = 2 + a . dir (and its square) at each texel's centre, with the
    border by the reference's rule.  Two points of the octahedral square that face each other across an edge - (1 - eps, y) and
    (1 - eps, -y), and so on every side, and the pairs of corners - are neighbouring DIRECTIONS; the fetches there agree to within the
    function's variation over one texel: |a| (its Lipschitz constant on the sphere's chords) times the largest chord between two
    corners of one texel, computed from decode alone."""
    a = np.array([0.6, -0.5, 0.7], F)
    f = lambda dirs: (F(2) + dirs @ a).astype(F)                                         # noqa: E731
    c = (np.arange(res, dtype=F) + F(0.5)) * (F(2) / F(res)) - F(1)
    cy, cx = np.meshgrid(c, c, indexing="ij")
    centre = f(V.normalize3(V.decode(cx.reshape(-1), cy.reshape(-1))))
    interior = np.stack([centre, centre * centre], 1)
    atlas = interior[V.border_source(res)].reshape(1, res + 2, res + 2, 2)
    # the bound: the largest chord between corners of one texel
    e = np.arange(res + 1, dtype=F) * (F(2) / F(res)) - F(1)
    gy, gx = np.meshgrid(e, e, indexing="ij")
    corner = V.normalize3(V.decode(gx.reshape(-1), gy.reshape(-1))).astype(np.float64).reshape(res + 1, res + 1, 3)
    quad = np.stack([corner[:-1, :-1], corner[:-1, 1:], corner[1:, :-1], corner[1:, 1:]], 2)      # (res, res, 4, 3)
    chord = np.linalg.norm(quad[:, :, :, None, :] - quad[:, :, None, :, :], axis=-1).max()
    bound = float(np.linalg.norm(a.astype(np.float64))) * chord
    eps = 1e-3
    y = np.linspace(-0.95, 0.95, 39).astype(F)
    near = np.full_like(y, 1 - eps)
    pairs = [((near, y), (near, -y)), ((-near, y), (-near, -y)), ((y, near), (-y, near)), ((y, -near), (-y, -near)),
             ((near[:1], near[:1]), (-near[:1], -near[:1])), ((near[:1], -near[:1]), (-near[:1], near[:1])), ((near[:1], near[:1]), (near[:1], -near[:1]))]
    worst = 0.0
    for q1, q2 in pairs:
        got = []
        for qx, qy in (q1, q2):
            dirs = V.normalize3(V.decode(qx, qy))
            px, py = V.encode(dirs)
            got.append((dirs, V.fetch(np.repeat(atlas, len(px), 0), V.texel_coordinate(px, res), V.texel_coordinate(py, res), res)[0]))
        assert np.linalg.norm(got[0][0] - got[1][0], axis=1).max() <= 4 * eps       # neighbouring directions indeed
        worst = max(worst, float(np.abs(got[0][1] - got[1][1]).max()))
        assert np.abs(got[0][1] - got[1][1]).max() <= bound, (res, bound)
        assert np.abs(got[0][1] - f(got[0][0])).max() <= 2 * bound                  # and the fetch is near the function itself
    print(f"res {res}: fetches across the edges differ by at most {worst:.3g}; the function varies by {bound:.3g} over a texel")


def test_sample_with_both_factors_off_is_probe_ref_sample():
    for count in ((1, 1, 1), (2, 1, 1), (5, 4, 3)):
        vol = P.fabricated_volume(count, 9)
        d = P.desc((0.5, -1.0, 2.0), (0.5, 0.25, 1.5), count)
        pts = P.sample_points(d, 260, 3, nonfinite=True)
        got = V.sample(d, V.vis(8, backface=False, chebyshev=False, normal_bias=0.5), vol, None, pts)
        assert (got.view(U) == P.sample(d, vol, pts).view(U)).all(), count
        n = count[0] * count[1] * count[2]
        out, wb, wv = V.sample(d, V.vis(8, normal_bias=0.25), vol, V.hashed_atlas(n, 8, 5), pts, detail=True)
        assert wb.shape == wv.shape == (260, 8) and (out.view(U) != got.view(U)).any()
        assert ((wv == 1) | ((wv >= F(0.05)) & (wv < 1))).all() and (wv == F(0.05)).any() and ((wv > F(0.05)) & (wv < 1)).any()
        finite = np.isfinite(pts[:, 0:3]).all(1)
        assert ((wb[finite] >= F(0.2)) & (wb[finite] <= F(1.2001))).all()


def test_fabricated_atlases_hold_what_they_claim():
    for res in (4, 8, 16):
        a = V.hashed_atlas(60, res, 3)
        assert a.shape == (60, res + 2, res + 2, 2) and a.dtype == F
        m1, m2 = a[..., 0], a[..., 1]
        ok = np.isfinite(m1) & np.isfinite(m2)
        assert np.isinf(m1).any() and np.isnan(m2).any() and (m1 == 0).any() and (m2 == 0).any()
        assert (m2[ok] < m1[ok] * m1[ok]).any() and (m2[ok] > m1[ok] * m1[ok]).any()


def test_probe_visibility_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/probe_visibility.hip (the flags are the Makefile's; read as
    test_gather_kernels_add_no_scratch reads its unit's): exactly the three k_pvv_* kernels are there - k_pv_sample is not compiled
    a second time -, none has scratch, the rays and the reduction have no LDS.  The look-up's occupancy is printed, not gated."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "probe_visibility.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "probe_visibility.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_[a-z]+_[a-z]+", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_pvv_rays", "k_pvv_reduce", "k_pvv_sample"] and len(report) == 3, sorted(report)
    for k, v in names.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
    assert names["k_pvv_rays"]["LDS Size"] == 0 and names["k_pvv_reduce"]["LDS Size"] == 0
    print("k_pvv_sample: occupancy", names["k_pvv_sample"]["Occupancy"], "waves per SIMD,", names["k_pvv_sample"]["VGPRs"], "VGPRs")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_probe_vis.h")).read()
    assert '#include "hj_probes.h"' in src and "pv_axis(" in src and "sh9_basis(" in src
