"""hj_update_probes / hj_update_probe_visibility, the part that needs no GPU: the symbols are declared, listed and exported and the
ABI mirror has the header's layout; every argument refusal comes before the device is touched, in the stated order - the descs' first -
with a message, and writes nothing; the reference of the GPU tests (probe_update_ref) on fabricated data: a zero hysteresis gives the
fresh bits over NaN memory, nothing outside the window changes, every branch of the rule is taken by a stated number of rows, and the
border of an atlas is repaired; the compiler's resource report of the unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import probe_ref as P
import probe_update_ref as PU
import probe_vis_ref as V
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_update_probes", "hj_update_probe_visibility")
INF, NAN = float("inf"), float("nan")
_desc, _vis, _upd = P.abi_desc, V.abi_vis, PU.abi_update


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def _opts(**kw):
    o = abi.RenderOpts.default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001600
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_PROBE_UPDATE_WORDS 8u", "Probe updates (ABI 0.22)", "0.15f", "A refused call writes nothing"):
        assert text in header, text
    assert abi.PROBE_UPDATE_WORDS == 8 and F(abi.PROBE_UPDATE_SOFT_STEP) == PU.SOFT_STEP and abi.PROBE_UPDATE_CHANGE == (0.25, 0.8)
    assert abi.PROBE_UPDATE_FRAME_STRIDE % 2 == 1 and 0 < abi.PROBE_UPDATE_FRAME_STRIDE < 1 << 32
    for fn in ("update_probes", "update_probe_visibility"):
        assert callable(getattr(device.Renderer, fn))


def test_abi_mirror_matches_the_header(tmp_path):
    """size and field offsets of hj_probe_update as a C compiler lays the header's struct out, and the macro's value"""
    names = [n for n, _ in abi.ProbeUpdate._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hijiki_hip.h"\nint main(void) {\n  printf("%zu", sizeof(hj_probe_update));\n'
                   + "".join(f'  printf(" %zu", offsetof(hj_probe_update, {n}));\n' for n in names)
                   + '  printf(" %u", HJ_PROBE_UPDATE_WORDS);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got[:-1] == [C.sizeof(abi.ProbeUpdate)] + [getattr(abi.ProbeUpdate, n).offset for n in names], got
    assert got[0] == 32 == 4 * got[-1] and got[1:-1] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert names == ["first_probe", "num_probes", "frame", "frame_stride", "hysteresis", "change_soft", "change_hard", "flags"]


# -------------------------------------------------------------------------------------------------------------------- refusals

def _calls():
    """-> the two entry points as functions of (desc or None, vis or None, update or None, keywords), each over arrays this returns too"""
    L = device.lib()
    buf = dict(volume=np.full((8, 28), 7.0, F), atlas=np.full((8, 72), 7.0, F), stats=abi.RenderStats())
    ref = lambda s: C.byref(s) if s is not None else None                                    # noqa: E731

    def probes(d, v, u, spp=1, opts=None, probes=buf["volume"], **_):
        return L.hj_update_probes(None, ref(d), ref(u), spp, opts, _p(probes), buf["stats"])

    def visibility(d, v, u, atlas=buf["atlas"], **_):
        return L.hj_update_probe_visibility(None, ref(d), ref(v), ref(u), _p(atlas))
    return {"hj_update_probes": probes, "hj_update_probe_visibility": visibility}, buf


def _untouched(buf):
    return (buf["volume"] == 7.0).all() and (buf["atlas"] == 7.0).all() and not any(getattr(buf["stats"], f) for f, _ in abi.RenderStats._fields_)


def _refused(call, name, word, *args, status=abi.HJ_ERR_INVALID, **kw):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call(*args, **kw) == status, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and name.encode() in text and word in text, (name, word, text)


# (the word its message holds, which struct, the struct's keywords), in the header's order
DESC_ORDER = [(b": unknown flag bits", "d", dict(flags=2)), (b"count", "d", dict(count=(0, 1, 1))), (b"origin", "d", dict(origin=(NAN, 0, 0))),
              (b"spacing", "d", dict(spacing=(0, 1, 1))), (b"min_distance", "d", dict(min_distance=-1.0))]
VIS_ORDER = [(b"visibility flag bits", "v", dict(flags=8)), (b"res", "v", dict(res=3)), (b"rays_per_texel", "v", dict(rays_per_texel=0)),
             (b"max_distance", "v", dict(max_distance=0.0))]
UPDATE_ORDER = [(b"update flag bits", "u", dict(flags=1)), (b"probes 5 ... 13 of 8", "u", dict(first_probe=5, num_probes=8)),
                (b"hysteresis", "u", dict(hysteresis=1.0)), (b"change_soft", "u", dict(change_soft=-0.5)), (b"change_hard", "u", dict(change_hard=NAN))]
UPDATE_REFUSALS = [(b"update flag bits", dict(flags=0x80000000)), (b"probes 8 ... 9 of 8", dict(first_probe=8, num_probes=1)),
                   (b"probes", dict(first_probe=0xFFFFFFFF, num_probes=2)), (b"probes", dict(first_probe=1, num_probes=0xFFFFFFFF)),
                   (b"hysteresis", dict(hysteresis=-0.25)), (b"hysteresis", dict(hysteresis=NAN)), (b"hysteresis", dict(hysteresis=INF)),
                   (b"hysteresis", dict(hysteresis=1.5)), (b"change_soft", dict(change_soft=NAN)), (b"change_soft", dict(change_soft=-INF)),
                   (b"change_hard", dict(change_hard=-1.0))]


def test_argument_refusals_come_before_the_device():
    calls, buf = _calls()
    for name, call in calls.items():
        _refused(call, name, b"null desc", None, _vis(), _upd())
        _refused(call, name, b"null update", _desc(), _vis(), None)
        for word, _, dkw in DESC_ORDER:
            _refused(call, name, word, _desc(**dkw), _vis(), _upd())
        for word, ukw in UPDATE_REFUSALS:
            _refused(call, name, word, _desc(), _vis(), _upd(**ukw))
    probes, visibility = calls["hj_update_probes"], calls["hj_update_probe_visibility"]
    DEV = abi.PROBES_DEVICE_ARRAYS
    _refused(probes, "hj_update_probes", b"null probes", _desc(), None, _upd(), probes=None)
    _refused(probes, "hj_update_probes", b"spp", _desc(), None, _upd(), spp=0)
    _refused(probes, "hj_update_probes", b"spp", _desc(), None, _upd(), spp=65537)
    _refused(probes, "hj_update_probes", b"aligned", _desc(flags=DEV), None, _upd(), probes=buf["volume"].ctypes.data + 8)
    _refused(probes, "hj_update_probes", b"max_bounces", _desc(), None, _upd(), opts=_opts(max_bounces=0))
    _refused(probes, "hj_update_probes", b"use_bvh", _desc(), None, _upd(), opts=_opts(use_bvh=0), status=abi.HJ_ERR_UNSUPPORTED)
    _refused(visibility, "hj_update_probe_visibility", b"null vis", _desc(), None, _upd())
    _refused(visibility, "hj_update_probe_visibility", b"null atlas", _desc(), _vis(), _upd(), atlas=None)
    for word, _, vkw in VIS_ORDER:
        _refused(visibility, "hj_update_probe_visibility", word, _desc(), _vis(**vkw), _upd())
    _refused(visibility, "hj_update_probe_visibility", b"must agree", _desc(flags=DEV), _vis(), _upd())
    _refused(visibility, "hj_update_probe_visibility", b"aligned", _desc(flags=DEV), _vis(flags=abi.PROBE_VIS_DEVICE_ARRAYS), _upd(),
             atlas=buf["atlas"].ctypes.data + 4)
    assert _untouched(buf)


def test_refusals_come_in_the_stated_order():
    """Several faults in one call: the earliest check's message.  Each refusal is paired with everything behind it: the descs' come
    before the update's, the update's before spp, alignment and opts."""
    calls, buf = _calls()
    L = device.lib()
    odd = buf["volume"].ctypes.data + 4
    for name, call in calls.items():
        steps = DESC_ORDER + (VIS_ORDER if name == "hj_update_probe_visibility" else []) + UPDATE_ORDER
        for i in range(len(steps)):
            kw = {"d": {}, "v": {}, "u": {}}
            for _, which, k in steps[i:]:
                kw[which].update(k)
            assert call(_desc(**kw["d"]), _vis(**kw["v"]), _upd(**kw["u"]), spp=0, opts=_opts(max_bounces=0)) == abi.HJ_ERR_INVALID
            assert steps[i][0] in L.hj_last_error(None), (name, steps[i][0], L.hj_last_error(None))
        # a bad desc and a bad (or no) update: the desc; a null array before either
        assert call(_desc(count=(0, 1, 1)), _vis(), _upd(hysteresis=2.0)) == abi.HJ_ERR_INVALID and b"count" in L.hj_last_error(None)
        assert call(_desc(min_distance=NAN), _vis(), None) == abi.HJ_ERR_INVALID and b"min_distance" in L.hj_last_error(None)
        assert call(_desc(flags=2), _vis(), None, probes=None, atlas=None) == abi.HJ_ERR_INVALID and b"null" in L.hj_last_error(None)
        assert b"null update" not in L.hj_last_error(None)
        assert call(None, None, None, probes=None, atlas=None) == abi.HJ_ERR_INVALID and b"null desc" in L.hj_last_error(None)
        # no update before what stands behind the update's checks
        assert call(_desc(), _vis(), None, spp=0, opts=_opts(max_bounces=0)) == abi.HJ_ERR_INVALID and b"null update" in L.hj_last_error(None)
    probes, visibility = calls["hj_update_probes"], calls["hj_update_probe_visibility"]
    assert visibility(_desc(), _vis(max_distance=-1.0), None) == abi.HJ_ERR_INVALID and b"max_distance" in L.hj_last_error(None)
    on = _desc(flags=abi.PROBES_DEVICE_ARRAYS)
    for kw, word in ((dict(spp=0, probes=odd, opts=_opts(max_bounces=0)), b"spp"), (dict(spp=1, probes=odd, opts=_opts(max_bounces=0)), b"aligned"),
                     (dict(spp=1, opts=_opts(max_bounces=0, use_bvh=0)), b"max_bounces")):
        assert probes(on, None, _upd(), **kw) == abi.HJ_ERR_INVALID and word in L.hj_last_error(None), (word, L.hj_last_error(None))
    assert probes(on, None, _upd(change_hard=-1.0), spp=0, probes=odd) == abi.HJ_ERR_INVALID and b"change_hard" in L.hj_last_error(None)
    assert visibility(on, _vis(flags=abi.PROBE_VIS_DEVICE_ARRAYS), _upd(hysteresis=NAN), atlas=odd) == abi.HJ_ERR_INVALID
    assert b"hysteresis" in L.hj_last_error(None)
    assert _untouched(buf)


def test_a_valid_call_without_a_context_is_refused_last():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none: also at the edges of the
    update's domain - a zero hysteresis, one just below 1, infinite and zero thresholds, a window that ends with the volume, an empty one."""
    calls, buf = _calls()
    L = device.lib()
    below_one = float(np.nextafter(F(1), F(0)))
    for u in (_upd(), _upd(hysteresis=0.0, change_soft=INF, change_hard=INF), _upd(hysteresis=below_one, change_soft=0.0, change_hard=0.0),
              _upd(first_probe=7, num_probes=1, frame=0xFFFFFFFF, frame_stride=0xFFFFFFFF), _upd(first_probe=8, num_probes=0)):
        for name, call in calls.items():
            rc = call(_desc(), _vis(), u, spp=65536)
            if L.hj_device_count() == 0:
                assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None) and name.encode() in L.hj_last_error(None)
            else:
                assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert _untouched(buf)


def test_wrapper_checks_its_arguments_before_any_call():
    import pytest
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    grid = dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2))
    vol, atlas = np.zeros((2, 2, 2, 28), F), np.zeros((2, 2, 2, 6, 6, 2), F)
    good = dict(frame=0, hysteresis=0.5)
    for kw in (dict(hysteresis=1.0), dict(hysteresis=-0.1), dict(hysteresis=NAN), dict(window=(5, 4)), dict(window=(-1, 2)), dict(window=(9, 0)),
               dict(frame=-1), dict(frame=1 << 32), dict(frame_stride=1 << 32)):
        with pytest.raises(ValueError):
            r.update_probes(grid, vol, 4, **dict(good, **kw))
        with pytest.raises(ValueError):
            r.update_probe_visibility(grid, dict(res=4, rays_per_texel=1, max_distance=5.0), atlas, **dict(good, **kw))
    for kw in (dict(change=(-1.0, 0.8)), dict(change=(0.25, NAN))):
        with pytest.raises(ValueError):
            r.update_probes(grid, vol, 4, **dict(good, **kw))
    for spp in (0, 65537):
        with pytest.raises(ValueError):
            r.update_probes(grid, vol, spp, **good)
    with pytest.raises(ValueError):
        r.update_probes(grid, np.zeros((2, 2, 3, 28), F), 4, **good)
    with pytest.raises(ValueError):
        r.update_probes(dict(grid, count=(0, 2, 2)), vol, 4, **good)
    with pytest.raises(ValueError):
        r.update_probe_visibility(grid, dict(res=8, rays_per_texel=1, max_distance=5.0), atlas, **good)       # (the atlas is res 4's)
    with pytest.raises(ValueError):
        r.update_probe_visibility(grid, dict(res=5), atlas, **good)


# ------------------------------------------------------------------------------------------------------- the reference's own checks

# the fabricated volume's rows, by what they are made for: (how many, the factor on the old coefficients, old validity, fresh validity)
ROWS = [("same", 2, 1.0, 1.0, 1.0), ("near", 2, 1.1, 0.25, 1.0), ("soft", 3, 1.5, 1.0, 1.0), ("hard", 2, 10.0, 1.0, 1.0), ("old_invalid", 2, None, 0.0, 1.0),
        ("fresh_invalid", 2, 1.0, 1.0, 0.0), ("nan_validity", 1, 1.0, NAN, 1.0), ("zero_band", 2, 0.0, 1.0, 1.0)]


def fabricated_update():
    """-> (old, fresh (16, 28), {kind: its rows}).  fresh: coefficients in [0.5, 2), so that a factor f on them moves the constant band
    by |f - 1| / f of the old magnitude: 0, 0.09 (below 0.25), 0.33 (soft), 0.9 (hard).  old_invalid: NaN coefficients behind validity 0.
    zero_band: the old constant band is 0 (m == 0), the other bands are fresh's."""
    rng = np.random.default_rng(22)
    n = sum(k for _, k, *_ in ROWS)
    fresh = rng.uniform(0.5, 2.0, (n, 28)).astype(F)
    old = fresh.copy()
    rows, at = {}, 0
    for kind, k, factor, ov, fv in ROWS:
        sl = slice(at, at + k)
        rows[kind] = np.arange(at, at + k)
        if factor is None:
            old[sl, 0:27] = np.nan
        elif kind == "zero_band":
            old[sl, 0:3] = 0.0
        else:
            old[sl, 0:27] = fresh[sl, 0:27] * F(factor)
        old[sl, 27], fresh[sl, 27] = ov, fv
        at += k
    return old, fresh, rows


def test_reference_takes_every_branch_the_stated_number_of_times():
    old, fresh, rows = fabricated_update()
    n = len(old)
    assert n == 16
    h = F(0.75)
    new, hh, masks = PU.blend_probes(old, fresh, PU.update(0, n, h, 0.25, 0.8), detail=True)
    count = {k: int(v.sum()) for k, v in masks.items()}
    # zero_band with finite thresholds: d > hard * 0 - a hard change
    assert count == dict(none=4, soft=3, hard=4, old_invalid=2, fresh_invalid=2, nan_validity=1), count
    for kind, branch in (("same", "none"), ("near", "none"), ("soft", "soft"), ("hard", "hard"), ("zero_band", "hard"), ("old_invalid", "old_invalid"),
                         ("fresh_invalid", "fresh_invalid"), ("nan_validity", "nan_validity")):
        assert masks[branch][rows[kind]].all(), (kind, branch)
    assert (hh[rows["same"]] == h).all() and (hh[rows["near"]] == h).all() and (hh[rows["soft"]] == h - F(0.15)).all()
    for kind in ("hard", "zero_band", "old_invalid", "fresh_invalid", "nan_validity"):
        assert (hh[rows[kind]] == 0).all(), kind
        assert (bits(new[rows[kind]]) == bits(fresh[rows[kind]])).all(), kind          # never a mix: the fresh record's bits
    assert (bits(new[:, 27]) == bits(fresh[:, 27])).all() and np.isfinite(new[:, 0:27]).all()
    # by hand, one rounding per operation: a kept row and a soft row
    i, j = rows["near"][0], rows["soft"][1]
    assert new[i, 5] == F(old[i, 5] * h) + F(fresh[i, 5] * F(F(1) - h))
    hs = F(h - F(0.15))
    assert new[j, 26] == F(old[j, 26] * hs) + F(fresh[j, 26] * F(F(1) - hs))
    # infinite thresholds: never a change - with m == 0 the product is a NaN and the comparison false
    new, hh, masks = PU.blend_probes(old, fresh, PU.update(0, n, h, INF, INF), detail=True)
    count = {k: int(v.sum()) for k, v in masks.items()}
    assert count == dict(none=11, soft=0, hard=0, old_invalid=2, fresh_invalid=2, nan_validity=1), count
    z = rows["zero_band"]
    assert masks["none"][z].all() and (hh[z] == h).all() and (new[z, 0:3] == F(fresh[z, 0:3] * F(F(1) - h))).all()
    # a hysteresis below the soft step: max(h - 0.15, 0) = 0, the fresh bits
    new, hh, masks = PU.blend_probes(old, fresh, PU.update(0, n, 0.1, 0.25, 0.8), detail=True)
    assert masks["soft"].sum() == 3 and (hh[rows["soft"]] == 0).all() and (bits(new[rows["soft"]]) == bits(fresh[rows["soft"]])).all()


def test_reference_zero_hysteresis_is_the_fresh_bake_and_the_window_is_respected():
    old, fresh, rows = fabricated_update()
    n = len(old)
    nan_old = np.full_like(old, np.nan)
    nan_old.view(U)[:] = 0x7FA12345                                    # (a signalling pattern with a payload: copied, never computed with)
    new = PU.blend_probes(nan_old, fresh, PU.update(0, n, 0.0, 0.25, 0.8))
    assert (bits(new) == bits(fresh)).all()
    for first, num in ((3, 1), (5, 7), (1, n - 1), (n, 0), (4, 0)):
        new = PU.blend_probes(nan_old, fresh, PU.update(first, num, 0.0))
        inside = np.zeros(n, bool)
        inside[first:first + num] = True
        assert (bits(new[inside]) == bits(fresh[inside])).all() and (bits(new[~inside]) == 0x7FA12345).all(), (first, num)
        new = PU.blend_probes(old, fresh, PU.update(first, num, 0.5, 0.25, 0.8))
        assert (bits(new[~inside]) == bits(old[~inside])).all() and (num == 0 or (bits(new[inside]) != bits(old[inside])).any())
    shaped = PU.blend_probes(old.reshape(2, 2, 4, 28), fresh.reshape(2, 2, 4, 28), PU.update(0, n, 0.5))
    assert shaped.shape == (2, 2, 4, 28)


def test_reference_repairs_the_border_of_an_atlas():
    """probe_vis_ref.hashed_atlas: borders that do not match their interior, zeros, an infinity, a NaN.  After one update every border
    texel of the window is its interior texel's new value, whatever it held; outside the window every bit stays."""
    for res in (4, 8, 16):
        n, T = 9, res + 2
        old, fresh = V.hashed_atlas(n, res, 3), V.hashed_atlas(n, res, 4)
        src = V.border_source(res)
        mismatched = lambda a: (bits(a.reshape(n, T * T, 2)) != bits(a[:, 1:-1, 1:-1].reshape(n, res * res, 2)[:, src])).any(axis=(1, 2))   # noqa: E731
        assert mismatched(old).all() and mismatched(fresh).all()
        for h in (0.0, 0.9):
            new = PU.blend_atlas(old, fresh, res, PU.update(2, 5, h))
            bad = mismatched(new)
            assert not bad[2:7].any() and bad[0:2].all() and bad[7:].all(), (res, h)
            assert (bits(new[0:2]) == bits(old[0:2])).all() and (bits(new[7:]) == bits(old[7:])).all()
            inner_new, inner_old, inner_fresh = (a[2:7, 1:-1, 1:-1] for a in (new, old, fresh))
            if h == 0.0:
                assert (bits(inner_new) == bits(inner_fresh)).all()    # (fresh's NaNs and infinities as they are)
            else:
                with np.errstate(invalid="ignore"):
                    want = (inner_old * F(h)).astype(F) + (inner_fresh * F(F(1) - F(h))).astype(F)
                assert (np.isnan(inner_new) == np.isnan(want)).all() and (inner_new[~np.isnan(want)] == want[~np.isnan(want)]).all()
                if res == 16:                                          # (1280 texels of the window: a few per cent of each kind)
                    assert np.isnan(want).any() and np.isinf(want).any()


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_probe_update_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/probe_update.hip (the flags are the Makefile's; read as
    test_probe_visibility_kernels_use_no_scratch reads its unit's): exactly the two k_pu_* kernels are there - no kernel of
    hj_probes.h or hj_probe_vis.h is compiled a second time -, neither has scratch or LDS.  The occupancy is printed, not gated."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "probe_update.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "probe_update.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_[a-z]+_[a-z]+", k).group(0): v for k, v in report.items()}
    assert sorted(names) == ["k_pu_reduce", "k_pu_resolve"] and len(report) == 2, sorted(report)
    for k, v in names.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0, (k, v)
        print(f"{k}: occupancy", v["Occupancy"], "waves per SIMD,", v["VGPRs"], "VGPRs")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_probe_update.h")).read()
    assert "pv_resolve_record(" in src and "pvv_moments(" in src and '#include "hj_probe_vis.h"' in src
    # one text per arithmetic: the resolve's constants and the moments' loop stand in the headers both units include, once
    csrc = os.path.join(ROOT, "hijiki_amd", "csrc")
    holds = [f for sub in ("api", "kernels") for f in sorted(os.listdir(os.path.join(csrc, sub))) if "2.09439516f" in open(os.path.join(csrc, sub, f)).read()]
    assert holds == ["hj_probes.h"], holds
