"""hj_place_probes and the placed updates and look-up, the part that needs no GPU: the symbols are declared, listed and exported and
the ABI mirror has the header's layout; every argument refusal comes before the device is touched, in the stated order, with a
message, and writes nothing; the reference of the GPU tests (probe_place_ref) on fabricated hits that take every branch of the step a
stated number of times; the purpose on a numpy cube intersected by brute force - a probe just inside a face leaves the cube and
wakes up, a probe deep inside stays and sleeps, a probe in empty space sleeps; the compiler's resource report of the unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import probe_place_ref as PP
import probe_ref as P
import probe_update_ref as PU
import probe_vis_ref as V
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
NAMES = ("hj_place_probes", "hj_update_probes_placed", "hj_update_probe_visibility_placed", "hj_sample_probes_visible_placed")
INF, NAN = float("inf"), float("nan")
_desc, _vis, _upd, _place = P.abi_desc, V.abi_vis, PU.abi_update, PP.abi_place


def _p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001700
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_PROBE_PLACE_WORDS 4u", "Probe placement (ABI 0.23)", "#define HJ_PROBE_PLACE_NO_RELOCATE 1u", "#define HJ_PROBE_PLACE_NO_CLASSIFY 2u",
                 "turns a probe coordinate of -0 into +0", "There are no placed bakes", "not values tuned here", "A refused call writes nothing"):
        assert text in header, text
    assert abi.PROBE_PLACE_WORDS == 4 == PP.WORDS and (abi.PROBE_PLACE_NO_RELOCATE, abi.PROBE_PLACE_NO_CLASSIFY) == (1, 2)
    assert (abi.PROBE_PLACE_BACKFACE_SHARE, abi.PROBE_PLACE_MAX_OFFSET) == (0.25, 0.45)
    for fn in ("place_probes", "new_placement"):
        assert callable(getattr(device.Renderer, fn))
    import inspect
    for fn in ("update_probes", "update_probe_visibility", "sample_probes_visible"):
        assert inspect.signature(getattr(device.Renderer, fn)).parameters["placement"].default is None


def test_abi_mirror_matches_the_header(tmp_path):
    """size and field offsets of hj_probe_place as a C compiler lays the header's struct out, and the macros' values"""
    names = [n for n, _ in abi.ProbePlace._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hijiki_hip.h"\nint main(void) {\n  printf("%zu", sizeof(hj_probe_place));\n'
                   + "".join(f'  printf(" %zu", offsetof(hj_probe_place, {n}));\n' for n in names)
                   + '  printf(" %u", HJ_PROBE_PLACE_WORDS);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got[:-1] == [C.sizeof(abi.ProbePlace)] + [getattr(abi.ProbePlace, n).offset for n in names], got
    assert got[0] == 32 and got[-1] == 4 and got[1:-1] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert names == ["first_probe", "num_probes", "frame", "frame_stride", "min_front_distance", "backface_share", "max_offset", "flags"]


# -------------------------------------------------------------------------------------------------------------------- refusals

def _calls():
    """-> the four entry points as functions of (desc, vis, update or place, keywords), each over arrays this returns too"""
    L = device.lib()
    buf = dict(volume=np.full((8, 28), 7.0, F), atlas=np.full((8, 72), 7.0, F), placement=np.full((8, 4), 0.125, F), points=np.ones((3, 8), F),
               out=np.full((3, 4), 7.0, F), stats=abi.RenderStats())
    ref = lambda s: C.byref(s) if s is not None else None                                    # noqa: E731

    def place(d, v, u, placement=buf["placement"], **_):
        return L.hj_place_probes(None, ref(d), ref(v), ref(u), _p(placement))

    def probes(d, v, u, spp=1, opts=None, probes=buf["volume"], placement=buf["placement"], **_):
        return L.hj_update_probes_placed(None, ref(d), ref(u), spp, opts, _p(placement), _p(probes), buf["stats"])

    def visibility(d, v, u, atlas=buf["atlas"], placement=buf["placement"], **_):
        return L.hj_update_probe_visibility_placed(None, ref(d), ref(v), ref(u), _p(placement), _p(atlas))

    def sample(d, v, u, probes=buf["volume"], atlas=buf["atlas"], points=buf["points"], m=3, placement=buf["placement"], out=buf["out"], **_):
        return L.hj_sample_probes_visible_placed(None, ref(d), ref(v), _p(probes), _p(atlas), _p(points), m, _p(placement), _p(out))
    return {NAMES[0]: place, NAMES[1]: probes, NAMES[2]: visibility, NAMES[3]: sample}, buf


def _untouched(buf):
    return ((buf["volume"] == 7.0).all() and (buf["atlas"] == 7.0).all() and (buf["placement"] == 0.125).all() and (buf["out"] == 7.0).all()
            and not any(getattr(buf["stats"], f) for f, _ in abi.RenderStats._fields_))


def _refused(call, name, word, *args, status=abi.HJ_ERR_INVALID, **kw):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call(*args, **kw) == status, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and (name.encode() + b":") in text and word in text, (name, word, text)


# (the word its message holds, which struct, the struct's keywords), in the header's order
DESC_ORDER = [(b": unknown flag bits", "d", dict(flags=2)), (b"count", "d", dict(count=(0, 1, 1))), (b"origin", "d", dict(origin=(NAN, 0, 0))),
              (b"spacing", "d", dict(spacing=(0, 1, 1))), (b"min_distance", "d", dict(min_distance=-1.0))]
VIS_ORDER = [(b"visibility flag bits", "v", dict(flags=8)), (b"res", "v", dict(res=3)), (b"rays_per_texel", "v", dict(rays_per_texel=0)),
             (b"max_distance", "v", dict(max_distance=0.0))]
PLACE_ORDER = [(b"place flag bits", "u", dict(flags=4)), (b"probes 5 ... 13 of 8", "u", dict(first_probe=5, num_probes=8)),
               (b"min_front_distance", "u", dict(min_front_distance=0.0)), (b"backface_share", "u", dict(backface_share=1.5)),
               (b"max_offset", "u", dict(max_offset=0.5))]
PLACE_REFUSALS = [(b"place flag bits", dict(flags=0x80000000)), (b"probes 8 ... 9 of 8", dict(first_probe=8, num_probes=1)),
                  (b"probes", dict(first_probe=0xFFFFFFFF, num_probes=2)), (b"probes", dict(first_probe=1, num_probes=0xFFFFFFFF)),
                  (b"min_front_distance", dict(min_front_distance=-1.0)), (b"min_front_distance", dict(min_front_distance=NAN)),
                  (b"min_front_distance", dict(min_front_distance=INF)), (b"backface_share", dict(backface_share=-0.1)),
                  (b"backface_share", dict(backface_share=NAN)), (b"max_offset", dict(max_offset=-0.1)), (b"max_offset", dict(max_offset=NAN)),
                  (b"max_offset", dict(max_offset=0.75))]
UPDATE_ORDER = [(b"update flag bits", "u", dict(flags=1)), (b"probes 5 ... 13 of 8", "u", dict(first_probe=5, num_probes=8)),
                (b"hysteresis", "u", dict(hysteresis=1.0)), (b"change_soft", "u", dict(change_soft=-0.5)), (b"change_hard", "u", dict(change_hard=NAN))]
DEV, VDEV = abi.PROBES_DEVICE_ARRAYS, abi.PROBE_VIS_DEVICE_ARRAYS


def _second(name):
    return _place if name == NAMES[0] else _upd


def test_argument_refusals_come_before_the_device():
    calls, buf = _calls()
    bad = buf["placement"].copy()
    bad[6, 1] = INF
    for name, call in calls.items():
        u = _second(name)
        _refused(call, name, b"null desc", None, _vis(), u())
        _refused(call, name, b"null placement", _desc(), _vis(), u(), placement=None)
        for word, _, dkw in DESC_ORDER:
            _refused(call, name, word, _desc(**dkw), _vis(), u())
        _refused(call, name, b"probe 6 has a non-finite offset", _desc(), _vis(), u(), placement=bad)
        flags = dict(d=_desc(flags=DEV), v=_vis(flags=VDEV))
        _refused(call, name, b"aligned", flags["d"], flags["v"], u(), placement=buf["placement"].ctypes.data + 8)
    place, probes, visibility, sample = (calls[n] for n in NAMES)
    _refused(place, NAMES[0], b"null place", _desc(), _vis(), None)
    _refused(place, NAMES[0], b"null vis", _desc(), None, _place())
    for word, pkw in PLACE_REFUSALS:
        _refused(place, NAMES[0], word, _desc(), _vis(), _place(**pkw))
    for word, _, vkw in VIS_ORDER:
        _refused(place, NAMES[0], word, _desc(), _vis(**vkw), _place())
        _refused(visibility, NAMES[2], word, _desc(), _vis(**vkw), _upd())
    _refused(place, NAMES[0], b"must agree", _desc(flags=DEV), _vis(), _place())
    # a window that leaves the bad offset out is not refused for it (without a device the call ends at the context)
    assert place(_desc(), _vis(), _place(first_probe=0, num_probes=6), placement=bad) != abi.HJ_ERR_INVALID or b"offset" not in device.lib().hj_last_error(None)
    for name, call in ((NAMES[1], probes), (NAMES[2], visibility)):
        _refused(call, name, b"null update", _desc(), _vis(), None)
        for word, _, ukw in UPDATE_ORDER:
            _refused(call, name, word, _desc(), _vis(), _upd(**ukw))
    _refused(probes, NAMES[1], b"null probes", _desc(), None, _upd(), probes=None)
    _refused(probes, NAMES[1], b"spp", _desc(), None, _upd(), spp=0)
    _refused(probes, NAMES[1], b"aligned", _desc(flags=DEV), None, _upd(), probes=buf["volume"].ctypes.data + 8)
    _refused(visibility, NAMES[2], b"null atlas", _desc(), _vis(), _upd(), atlas=None)
    _refused(sample, NAMES[3], b"null placement", _desc(), _vis(), None, placement=None, m=0)
    _refused(sample, NAMES[3], b"null points", _desc(), _vis(), None, points=None)
    _refused(sample, NAMES[3], b"normal_bias", _desc(), _vis(normal_bias=-1.0), None)
    nanp = buf["points"].copy()
    nanp[1, 0] = NAN
    _refused(sample, NAMES[3], b"point 1", _desc(), _vis(), None, points=nanp, placement=bad)      # (the points before the offsets)
    assert _untouched(buf)


def test_refusals_come_in_the_stated_order():
    """Several faults in one call: the earliest check's message.  Each refusal is paired with everything behind it."""
    calls, buf = _calls()
    L = device.lib()
    odd = buf["placement"].ctypes.data + 4
    bad = buf["placement"].copy()
    bad[0, 0] = NAN
    for name, call in calls.items():
        if name == NAMES[3]:
            continue
        u = _second(name)
        steps = DESC_ORDER + (VIS_ORDER if name != NAMES[1] else []) + (PLACE_ORDER if name == NAMES[0] else UPDATE_ORDER)
        for i in range(len(steps)):
            kw = {"d": {}, "v": {}, "u": {}}
            for _, which, k in steps[i:]:
                kw[which].update(k)
            assert call(_desc(**kw["d"]), _vis(**kw["v"]), u(**kw["u"]), spp=0, placement=bad) == abi.HJ_ERR_INVALID
            assert steps[i][0] in L.hj_last_error(None), (name, steps[i][0], L.hj_last_error(None))
        assert call(_desc(count=(0, 1, 1)), _vis(), None) == abi.HJ_ERR_INVALID and b"count" in L.hj_last_error(None)
        assert call(_desc(flags=2), _vis(), None, placement=None) == abi.HJ_ERR_INVALID and b"null placement" in L.hj_last_error(None)
        # alignment before a bad host offset cannot coincide (one is the device route's, one the host route's): each before the context
        assert call(_desc(flags=DEV), _vis(flags=VDEV), u(), placement=odd) == abi.HJ_ERR_INVALID and b"aligned" in L.hj_last_error(None)
        assert call(_desc(), _vis(), u(), placement=bad) == abi.HJ_ERR_INVALID and b"offset" in L.hj_last_error(None)
    place = calls[NAMES[0]]
    assert place(_desc(), _vis(), _place(max_offset=0.6), placement=bad) == abi.HJ_ERR_INVALID and b"max_offset" in L.hj_last_error(None)
    assert place(_desc(), _vis(max_distance=-1.0), None) == abi.HJ_ERR_INVALID and b"max_distance" in L.hj_last_error(None)
    assert calls[NAMES[1]](_desc(), None, _upd(), spp=0, placement=bad) == abi.HJ_ERR_INVALID and b"spp" in L.hj_last_error(None)
    assert _untouched(buf)


def test_a_valid_call_without_a_context_is_refused_last():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none: also at the edges of the
    step's domain - a share of 0 and of 1, a max_offset of 0 and just below 0.5, both flags, an empty window."""
    calls, buf = _calls()
    L = device.lib()
    below_half = float(np.nextafter(F(0.5), F(0)))
    cases = {NAMES[0]: (_place(), _place(backface_share=0.0, max_offset=0.0), _place(backface_share=1.0, max_offset=below_half, flags=3),
                        _place(first_probe=8, num_probes=0), _place(first_probe=7, num_probes=1, frame=0xFFFFFFFF, frame_stride=0xFFFFFFFF))}
    for name, call in calls.items():
        for u in cases.get(name, (_upd(), _upd(first_probe=8, num_probes=0))):
            rc = call(_desc(), _vis(), u)
            if L.hj_device_count() == 0:
                assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None) and name.encode() in L.hj_last_error(None)
            else:
                assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert _untouched(buf)


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    grid = dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2))
    vis = dict(res=4, rays_per_texel=1, max_distance=5.0)
    pl = device.Renderer.new_placement((2, 2, 2))
    assert pl.shape == (2, 2, 2, 4) and pl.dtype == F and not pl.any()
    good = dict(frame=0, min_front_distance=0.2)
    for kw in (dict(min_front_distance=0.0), dict(min_front_distance=NAN), dict(backface_share=1.5), dict(backface_share=NAN), dict(max_offset=0.5),
               dict(max_offset=-0.1), dict(window=(5, 4)), dict(frame=-1), dict(frame_stride=1 << 32)):
        with pytest.raises(ValueError):
            r.place_probes(grid, vis, pl, **dict(good, **kw))
    nonfinite = pl.copy()
    nonfinite[1, 0, 1, 2] = INF
    for arr in (nonfinite, np.zeros((2, 2, 3, 4), F), np.zeros((2, 2, 2, 3), F)):
        with pytest.raises(ValueError):
            r.place_probes(grid, vis, arr, **good)
        with pytest.raises(ValueError):
            r.update_probes(grid, np.zeros((2, 2, 2, 28), F), 4, frame=0, hysteresis=0.5, placement=arr)
        with pytest.raises(ValueError):
            r.update_probe_visibility(grid, vis, np.zeros((2, 2, 2, 6, 6, 2), F), frame=0, hysteresis=0.5, placement=arr)
        with pytest.raises(ValueError):
            r.sample_probes_visible(np.zeros((2, 2, 2, 28), F), np.zeros((2, 2, 2, 6, 6, 2), F), (0, 0, 0), (1, 1, 1), np.ones((1, 8), F), placement=arr)


def test_a_converted_placement_lives_until_the_call_returns(monkeypatch):
    """A placement that is not C-contiguous float32 - float64 (numpy's default dtype), a strided view, Fortran order - is converted, and
    the library gets the copy's address: the copy must be alive while the call runs and hold the caller's values.  The library is
    replaced by one that, at each placed call, looks at the array the wrapper made (through a weak reference) and reads the address."""
    import weakref
    r = object.__new__(device.Renderer)
    r._h, r.device = None, 0
    grid = dict(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2))
    vis = dict(res=4, rays_per_texel=1, max_distance=5.0)
    want = PP.with_state((np.arange(32, dtype=F).reshape(8, 4) - 16) / 64, [0, 1, 0, 0, 1, 0, 1, 0]).reshape(2, 2, 2, 4)
    seen, calls = {}, []
    real = device.Renderer._placement

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        seen["ref"], seen["ptr"] = weakref.ref(out[1]), out[2]
        return out

    class Lib:
        def _look(self, name, ptr):
            arr = seen["ref"]()
            assert arr is not None, f"{name}: the placement the wrapper made was freed before the call"
            assert ptr == seen["ptr"] == arr.ctypes.data and arr.dtype == F and arr.flags["C_CONTIGUOUS"]
            assert (np.frombuffer(C.string_at(ptr, want.nbytes), U) == bits(want).reshape(-1)).all(), name
            calls.append(name)
            return 0

        def hj_place_probes(self, h, d, v, pl, placement):
            return self._look("hj_place_probes", placement)

        def hj_update_probes_placed(self, h, d, u, spp, o, placement, probes, st):
            return self._look("hj_update_probes_placed", placement)

        def hj_update_probe_visibility_placed(self, h, d, v, u, placement, atlas):
            return self._look("hj_update_probe_visibility_placed", placement)

        def hj_sample_probes_visible_placed(self, h, d, v, vol, atl, pts, m, placement, out):
            return self._look("hj_sample_probes_visible_placed", placement)

    monkeypatch.setattr(device.Renderer, "_placement", spy)
    monkeypatch.setattr(device, "lib", lambda: Lib())
    wide = np.zeros((2, 2, 2, 8), F)
    wide[..., ::2] = want
    state_as_f64 = want.astype(np.float64)                               # (the states 0 and 1 as bits are 0.0 and a denormal: both exact in float64)
    forms = {"float64": state_as_f64, "strided": wide[..., ::2], "fortran": np.asfortranarray(want), "as it is": want}
    assert not forms["strided"].flags["C_CONTIGUOUS"] and not forms["fortran"].flags["C_CONTIGUOUS"] and forms["float64"].dtype == np.float64
    for name, arr in forms.items():
        r.update_probes(grid, np.zeros((2, 2, 2, 28), F), 4, frame=0, hysteresis=0.5, placement=arr)
        r.update_probe_visibility(grid, vis, np.zeros((2, 2, 2, 6, 6, 2), F), frame=0, hysteresis=0.5, placement=arr)
        r.sample_probes_visible(np.zeros((2, 2, 2, 28), F), np.zeros((2, 2, 2, 6, 6, 2), F), (0, 0, 0), (1, 1, 1), np.ones((1, 8), F), placement=arr)
        got = r.place_probes(grid, vis, arr, frame=0, min_front_distance=0.2)
        assert got is not arr and (bits(got) == bits(want)).all(), name
    assert len(calls) == 4 * len(forms) and set(calls) == set(NAMES)


# ------------------------------------------------------------------------------------------------------- the reference's own checks

MFD, MAXD = F(0.3), F(5.0)
KINDS = ["inside", "inside_tie", "near_turns", "near_same_side", "room_at_grid", "room_part_way", "room_all_the_way", "inside_too_far", "all_miss",
         "nan_normal", "exactly_at_min"]


def fabricated_step():
    """One probe per kind on a (11, 1, 1) grid of unit spacing, res 4, one ray a texel (R = 16): hits, distances and normals chosen by
    hand about the rays' real directions -> (d, v, pl, placement, ray, ids, t, normal, {kind: probe}, notes)"""
    n = len(KINDS)
    d = P.desc((0, 0, 0), (1, 1, 1), (n, 1, 1), seed=5, seed_stride=3)
    v = V.vis(res=4, s=1, max_distance=MAXD)
    at = {k: i for i, k in enumerate(KINDS)}
    placement = PP.zeros(n)
    placement[at["room_part_way"], 0:3] = (0.2, 0.0, 0.0)
    placement[at["room_all_the_way"], 0:3] = (0.1, 0.1, 0.0)
    placement[at["inside_too_far"], 0:3] = (0.4, 0.0, 0.0)
    placement.view(U)[at["inside"], 3] = 0
    placement.view(U)[at["nan_normal"], 3] = 1                            # (asleep: wakes up)
    ray = PP.rays(d, v, placement)
    R = 16
    dirs = ray[:, 3:6].reshape(n, R, 3)
    ids = np.zeros((n, R), np.int32)
    t = np.full((n, R), 2.0, F)
    normal = (-dirs).copy()                                               # front faces everywhere to begin with
    notes = {}

    def back(p, rs, dist):
        normal[p, rs] = dirs[p, rs]
        t[p, rs] = dist
    back(at["inside"], [2, 5, 7, 8, 12], [0.4, 0.05, 0.3, 0.2, 0.6])      # 5 of 16 > 0.25 * 16; the nearest is ray 5
    back(at["inside_tie"], [1, 3, 9, 10, 15], [0.5, 0.1, 0.1, 0.7, 0.9])  # rays 3 and 9 tie: ray 3
    p = at["inside_too_far"]
    east = [int(r) for r in np.argsort(-dirs[p, :, 0])[:5]]               # the five rays that point most along +x
    back(p, east, [0.05, 0.3, 0.3, 0.3, 0.3])
    assert dirs[p, east[0], 0] > 0.5
    notes["east"] = east[0]
    for kind, want in (("near_turns", False), ("near_same_side", True)):  # rf at 0.1, rq at 3.0, chosen by their directions' dot
        p = at[kind]
        dots = (dirs[p][:, None, :].astype(np.float64) * dirs[p][None, :, :]).sum(2)
        pairs = np.argwhere((dots > 0.6) & (dots < 0.99)) if want else np.argwhere(dots < 0.4)
        rf, rq = (int(x) for x in pairs[0])
        t[p, rf], t[p, rq] = 0.1, 3.0
        notes[kind] = (rf, rq)
    t[at["room_part_way"], :] = 2.0
    t[at["room_part_way"], 6] = 0.35                                      # cf - min_front = 0.05 < L = 0.2
    ids[at["all_miss"], :] = -1
    t[at["all_miss"], :] = 0.0
    normal[at["all_miss"]] = 0.0
    normal[at["nan_normal"]] = np.nan
    t[at["nan_normal"], :] = 0.1
    t[at["exactly_at_min"], :] = 2.0
    t[at["exactly_at_min"], [4, 11]] = MFD                                 # cf == min_front: neither near nor room
    pl = PP.place(0, n, MFD, 0.25, 0.45)
    return d, v, pl, placement, ray, ids.reshape(-1), t.reshape(-1), normal.reshape(-1, 3), at, notes


def test_reference_takes_every_branch_the_stated_number_of_times():
    d, v, pl, old, ray, ids, t, normal, at, notes = fabricated_step()
    new, masks, inside, st = PP.step(d, v, pl, old, ray, ids, t, normal, detail=True)
    count = {k: int(m.sum()) for k, m in masks.items()}
    assert count == dict(inside=3, near_moved=1, near_kept=2, back_moved=2, back_at_grid=2, none=1, rejected=1), count
    for kind, branch in (("inside", "inside"), ("inside_tie", "inside"), ("inside_too_far", "inside"), ("near_turns", "near_moved"),
                         ("near_same_side", "near_kept"), ("nan_normal", "near_kept"), ("room_part_way", "back_moved"), ("room_all_the_way", "back_moved"),
                         ("room_at_grid", "back_at_grid"), ("all_miss", "back_at_grid"), ("exactly_at_min", "none"), ("inside_too_far", "rejected")):
        assert masks[branch][at[kind]], (kind, branch)
    dirs = ray[:, 3:6].reshape(len(KINDS), 16, 3)
    by_hand = lambda O, dr, step: (O + (dr * F(step)).astype(F)).astype(F)                 # noqa: E731
    zero = np.zeros(3, F)
    # inside: through the nearest back face and half a min_front beyond; a tie takes the lower ray
    assert (bits(new[at["inside"], 0:3]) == bits(by_hand(zero, dirs[at["inside"], 5], F(0.05) + F(MFD * F(0.5))))).all()
    assert (bits(new[at["inside_tie"], 0:3]) == bits(by_hand(zero, dirs[at["inside_tie"], 3], F(0.1) + F(MFD * F(0.5))))).all()
    assert (bits(new[at["inside_tie"], 0:3]) != bits(by_hand(zero, dirs[at["inside_tie"], 9], F(0.1) + F(MFD * F(0.5))))).any()
    # beyond max_offset on x alone: the old offset, bit for bit
    p = at["inside_too_far"]
    cand = by_hand(old[p, 0:3], dirs[p, notes["east"]], F(0.05) + F(MFD * F(0.5)))
    assert cand[0] > F(0.45) and abs(cand[1]) <= F(0.45) and abs(cand[2]) <= F(0.45)
    assert (bits(new[p, 0:3]) == bits(old[p, 0:3])).all()
    # near: along the farthest ray, by min(ff, min_front); with both rays on one side nothing moves
    rf, rq = notes["near_turns"]
    assert (bits(new[at["near_turns"], 0:3]) == bits(by_hand(zero, dirs[at["near_turns"], rq], MFD))).all()
    for kind in ("near_same_side", "nan_normal", "room_at_grid", "all_miss", "exactly_at_min"):
        assert (bits(new[at[kind], 0:3]) == bits(old[at[kind], 0:3])).all(), kind
    # room: back towards the grid point by min(cf - min_front, L)
    p = at["room_part_way"]
    assert new[p, 0] == F(F(0.2) - F(F(F(0.2) / F(0.2)) * F(F(0.35) - MFD))) and new[p, 1] == 0 and new[p, 2] == 0
    assert np.abs(new[at["room_all_the_way"], 0:3]).max() < 1e-7
    # the states: inside and all_miss asleep; a NaN normal is no back face, and its hit 0.1 away wakes the probe up
    # By hand: a front face 2 away along a unit ray d is within the cells only if |O[a] + 2 d[a]| <= 1 on every axis.  From the grid
    # point that needs |d[a]| <= 0.5 thrice, a vector of length at most 0.87: no ray - room_at_grid sleeps.  From O = (0.1, 0.1, 0) it
    # needs -0.55 <= d.x, d.y <= 0.45 and |d.z| <= 0.5, at most 0.92 long: no ray either - room_all_the_way sleeps.  exactly_at_min has
    # two hits 0.3 away, room_part_way one 0.35 away, near_turns and near_same_side one 0.1 away: inside the cells whatever d - awake.
    want = {k: 0 for k in KINDS}
    want.update(inside=1, inside_tie=1, inside_too_far=1, all_miss=1, room_at_grid=1, room_all_the_way=1)
    for kind, s in want.items():
        assert st[at[kind]] == s and PP.state(new)[at[kind]] == s, kind
    for kind in ("room_at_grid", "room_all_the_way", "exactly_at_min", "near_turns"):
        p = at[kind]
        reach = old[p, 0:3][None, :] + dirs[p] * t.reshape(len(KINDS), 16)[p][:, None]
        assert bool(st[p] == 0) == bool((np.abs(reach) <= 1).all(1).any()), kind
    # both flags: nothing changes; each alone: the other half
    assert (bits(PP.step(d, v, dict(pl, flags=3), old, ray, ids, t, normal)) == bits(old)).all()
    only_state = PP.step(d, v, dict(pl, flags=PP.NO_RELOCATE), old, ray, ids, t, normal)
    only_offset = PP.step(d, v, dict(pl, flags=PP.NO_CLASSIFY), old, ray, ids, t, normal)
    assert (bits(only_state[:, 0:3]) == bits(old[:, 0:3])).all() and (bits(only_state[:, 3]) == bits(new[:, 3])).all()
    assert (bits(only_offset[:, 0:3]) == bits(new[:, 0:3])).all() and (bits(only_offset[:, 3]) == bits(old[:, 3])).all()
    # a window: everything outside keeps its bits (a NaN pattern included)
    odd = old.copy()
    odd.view(U)[[0, 1, 9, 10]] = 0x7FA12345
    R = 16
    win = PP.step(d, v, dict(pl, first=2, num=7), odd, ray[2 * R:9 * R], ids[2 * R:9 * R], t[2 * R:9 * R], normal[2 * R:9 * R])
    assert (bits(win[[0, 1, 9, 10]]) == 0x7FA12345).all() and (bits(win[2:9]) == bits(new[2:9])).all()


def test_reference_consumers_leave_inactive_probes_alone():
    rng = np.random.default_rng(23)
    n = 12
    old = rng.uniform(0.5, 2.0, (n, 28)).astype(F)
    old[:, 27] = 1.0
    placement = PP.with_state(PP.zeros(n), [0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0])
    upd = PU.update(2, 8, 0.5)
    act = PP.active(placement, 2, 8)
    assert act.tolist() == [2, 3, 6, 8, 9]
    fresh = rng.uniform(0.5, 2.0, (len(act), 28)).astype(F)
    fresh[:, 27] = 1.0
    new = PP.blend_probes(old, fresh, placement, upd)
    rest = np.setdiff1d(np.arange(n), act)
    assert (bits(new[rest]) == bits(old[rest])).all() and (bits(new[act]) != bits(old[act])).any()
    full = old.copy()
    full[act] = fresh
    assert (bits(new[act]) == bits(PU.blend_probes(old, full, upd)[act])).all()
    # with nobody asleep and no offset the placed reference is the unplaced one
    fresh_all = rng.uniform(0.5, 2.0, (n, 28)).astype(F)
    assert (bits(PP.blend_probes(old, fresh_all[2:10], PP.zeros(n), upd)) == bits(PU.blend_probes(old, fresh_all, upd))).all()
    res = 4
    a_old, a_fresh = V.hashed_atlas(n, res, 1), V.hashed_atlas(len(act), res, 2)
    a_new = PP.blend_atlas(a_old, a_fresh, res, placement, dict(upd, hysteresis=F(0)))
    assert (bits(a_new[rest]) == bits(a_old[rest])).all()
    assert (bits(a_new[act][:, 1:-1, 1:-1]) == bits(a_fresh[:, 1:-1, 1:-1])).all()
    # the look-up: zero placement is probe_vis_ref.sample; an inactive corner counts nothing, whatever its record holds
    d = P.desc((0, 0, 0), (1, 1, 1), (3, 2, 2))
    v = V.vis(res=res, normal_bias=0.05)
    vol, atl = P.fabricated_volume((3, 2, 2), 5), V.hashed_atlas(12, res, 3)
    pts = P.sample_points(d, 64, 7)
    assert (bits(PP.sample(d, v, vol, atl, pts, PP.zeros(12))) == bits(V.sample(d, v, vol, atl, pts))).all()
    asleep = PP.with_state(PP.zeros(12), [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1])
    poisoned = np.array(vol, F).reshape(12, 28).copy()
    poisoned[[1, 5, 11]] = np.nan
    got = PP.sample(d, v, poisoned, atl, pts, asleep)
    off = np.array(vol, F).reshape(12, 28).copy()
    off[[1, 5, 11], 27] = 0.0
    assert (bits(got) == bits(V.sample(d, v, off, atl, pts))).all() and np.isfinite(got).all()
    moved = PP.zeros(12)
    moved[:, 0:3] = rng.uniform(-0.4, 0.4, (12, 3)).astype(F)
    assert (bits(PP.sample(d, v, vol, atl, pts, moved)) != bits(V.sample(d, v, vol, atl, pts))).any()


# ----------------------------------------------------------------------------------------------------------------- the purpose

def cube_volume(half):
    """a (3, 1, 1) grid of spacing 1 along x about a cube of half-width `half` centred so that probe 0 sits `0.1` inside its -x face"""
    d = P.desc((0, 0, 0), (1, 1, 1), (3, 1, 1), seed=11, seed_stride=5)
    lo = np.array([-0.1, -half, -half])
    return d, PP.cube_trace(lo, lo + 2 * half)


def test_a_probe_just_inside_a_face_leaves_the_cube_and_wakes_up():
    """Probe 0 at the origin, 0.1 spacing inside the -x face of a cube of width 0.8; probe 1 at x = 1 stands 0.3 outside the +x face;
    probe 2 at x = 2 has no surface within one spacing."""
    d, trace = cube_volume(0.4)
    v = V.vis(res=8, s=2, max_distance=10.0)
    pl = PP.place(0, 3, 0.2)
    p0 = PP.zeros(3)
    p1, masks, inside, st = PP.trace_step(trace, d, v, pl, p0, detail=True)
    assert inside.tolist() == [True, False, False] and st.tolist() == [1, 0, 1]
    x = PP.placed_positions(d, p1, np.arange(3))
    assert x[0, 0] < -0.1 and np.abs(p1[0, 0:3]).max() <= 0.45 and (bits(p1[2, 0:3]) == 0).all()      # outside the face; empty space: stays
    p2, masks, inside, st = PP.trace_step(trace, d, v, pl, p1, seed=12, detail=True)
    assert inside.tolist() == [False, False, False] and st.tolist() == [0, 0, 1]                      # awake: the face it left is in its cells


def test_a_probe_deep_inside_a_wide_cube_stays_and_sleeps():
    """A cube wider than 0.9 spacings about a probe at its centre: every candidate lies beyond max_offset, the offset keeps its bits
    and the probe is inactive."""
    d = P.desc((0, 0, 0), (1, 1, 1), (1, 1, 1), seed=3)
    trace = PP.cube_trace((-0.48, -0.48, -0.48), (0.48, 0.48, 0.48))
    v = V.vis(res=8, s=2, max_distance=10.0)
    new, masks, inside, st = PP.trace_step(trace, d, v, PP.place(0, 1, 0.2), PP.zeros(1), detail=True)
    assert inside.all() and masks["rejected"].all() and (bits(new[0, 0:3]) == 0).all() and st.tolist() == [1]


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def _compile_report(tmp_path, unit):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / (unit + ".o")), os.path.join(ROOT, "hijiki_amd", "csrc", "api", unit + ".hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    return report, {re.search(r"k_[a-z]+_[a-z]+", k).group(0): v for k, v in report.items()}


def test_probe_place_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/probe_place.hip (the Makefile's flags): exactly the k_pp_* kernels - no kernel of the
    other probe headers is compiled a second time -, none has scratch; LDS only in the compaction.  Occupancy is printed, not gated."""
    report, names = _compile_report(tmp_path, "probe_place")
    want = ["k_pp_blend", "k_pp_count", "k_pp_points", "k_pp_rays", "k_pp_reduce", "k_pp_resolve", "k_pp_sample", "k_pp_scan", "k_pp_scatter"]
    assert sorted(names) == want and len(report) == len(want), sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert (v["LDS Size"] == 0) == (k not in ("k_pp_count", "k_pp_scan", "k_pp_scatter")), (k, v)
        print(f"{k}: occupancy", v["Occupancy"], "waves per SIMD,", v["VGPRs"], "VGPRs")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_probe_place.h")).read()
    for text in ("pu_resolve_probe(", "pu_reduce_texel(", "pvv_ray(", "compact_scan_tiles<", "HJ_COMPACT_RANK(", '#include "hj_probe_update.h"'):
        assert text in src, text
    assert "atomic" not in src.replace("no global atomics", "") and "asm" not in src.replace("no inline assembly", "")
    stamp = open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert '"hj_probe_place.h"' in stamp


def test_the_look_up_kernel_kept_its_registers(tmp_path):
    """A second compile of api/probe_visibility.hip: three kernels, and k_pvv_sample without scratch, as its own test demands - and
    at the 228 VGPRs and 2 waves per SIMD DESIGN.md records, which sharing its loop with k_pp_sample through a template did not keep."""
    report, names = _compile_report(tmp_path, "probe_visibility")
    assert sorted(names) == ["k_pvv_rays", "k_pvv_reduce", "k_pvv_sample"] and len(report) == 3
    s = names["k_pvv_sample"]
    print("k_pvv_sample:", s["VGPRs"], "VGPRs, occupancy", s["Occupancy"])
    assert s["ScratchSize"] == 0 and s["VGPRs"] == 228 and s["Occupancy"] == 2
