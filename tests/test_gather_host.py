"""hj_trace_irradiance, the part that needs no GPU: the symbol is declared, listed and exported; every argument refusal comes before
the device is touched, with its status and a message, and writes nothing; a valid call gets HJ_ERR_DEVICE where there is no device;
the Python wrapper's own checks raise before any call; the reference of the GPU tests (gather_ref.trace) IS path_query_ref.compose
when it is given compose's states and directions, and its directions are the header's; the compiler's resource report of the unit."""
import os
import re
import subprocess

import numpy as np
import pytest

import gather_ref as G
import path_query_ref as R
from hijiki_amd import abi, device
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32


def _call(points, n, spp, opts, flags, out, stats=None, ctx=None):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)  # noqa: E731
    return device.lib().hj_trace_irradiance(ctx, p(points), n, spp, opts, flags, p(out), stats)


def _points(n=4):
    pts = np.zeros((n, 8), F)
    pts[:, 4] = 1.0                                                    # normal +y
    return pts


def _opts(**kw):
    o = abi.RenderOpts.default()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_entry_point_is_declared_listed_and_exported():
    assert "hj_trace_irradiance" in declared_functions("hijiki_hip.h")
    assert "hj_trace_irradiance" in device.EXPORTS and hasattr(device.lib(), "hj_trace_irradiance")
    assert device.lib().hj_version() >= 0x000E00
    assert (abi.GATHER_DEVICE_ARRAYS, abi.GATHER_SPHERE, abi.GATHER_SH9) == (1, 2, 4)
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for line in ("#define HJ_GATHER_DEVICE_ARRAYS 1u", "#define HJ_GATHER_SPHERE 2u", "#define HJ_GATHER_SH9 4u"):
        assert line in header
    for name, c in zip(("c0", "c1", "c2", "c3", "c4"), (G.C0, G.C1, G.C2, G.C3, G.C4)):        # the reference's constants are the header's
        m = re.search(name + r" = (0x1\.[0-9a-f]+p[+-]\d+)f", header)
        assert m and F(float.fromhex(m.group(1))) == c, name
    assert callable(device.Renderer.trace_irradiance)


def test_sh_constants_are_the_basis():
    """The five float32 constants are the real spherical harmonics' normalisations, rounded to nearest."""
    pi = np.pi
    exact = (0.5 / np.sqrt(pi), np.sqrt(3 / (4 * pi)), np.sqrt(15 / (4 * pi)), np.sqrt(5 / (16 * pi)), np.sqrt(15 / (16 * pi)))
    assert [F(v) for v in exact] == [G.C0, G.C1, G.C2, G.C3, G.C4]


def test_argument_refusals_come_before_the_device():
    L = device.lib()
    pts, out = _points(), np.zeros((4, 36), F)
    keep = pts.copy()
    st = abi.RenderStats()
    INV, UNS = abi.HJ_ERR_INVALID, abi.HJ_ERR_UNSUPPORTED
    DEV, SPH, SH9 = abi.GATHER_DEVICE_ARRAYS, abi.GATHER_SPHERE, abi.GATHER_SH9

    def bad_normal(*v):
        p = _points()
        p[2, 3:6] = v
        return p
    cases = {
        "null points": (INV, (None, 4, 1, None, 0, out)),
        "null out": (INV, (pts, 4, 1, None, 0, None)),
        "unknown flag bits": (INV, (pts, 4, 1, None, 8, out)),
        "unknown flag bits beside the known ones": (INV, (pts, 4, 1, None, 0x80000007, out)),
        "SH9 without the sphere": (INV, (pts, 4, 1, None, SH9, out)),
        "SH9 without the sphere, device arrays": (INV, (pts, 4, 1, None, SH9 | DEV, out)),
        "spp 0": (INV, (pts, 4, 0, None, 0, out)),
        "spp above 65536": (INV, (pts, 4, 65537, None, SPH, out)),
        "too many points": (INV, (pts, 0x80000000, 1, None, SPH, out)),
        "misaligned device points": (INV, (pts.ctypes.data + 4, 3, 1, None, DEV, out)),
        "misaligned device out": (INV, (pts, 3, 1, None, DEV | SPH | SH9, out.ctypes.data + 8)),
        "max_bounces 0": (INV, (pts, 4, 1, _opts(max_bounces=0), 0, out)),
        "use_bvh 0": (UNS, (pts, 4, 1, _opts(use_bvh=0), SPH, out)),
        "split kernels": (INV, (pts, 4, 1, _opts(flags=abi.RENDER_SPLIT_KERNELS), 0, out)),
        "no drain beside the light grid bit": (INV, (pts, 4, 1, _opts(flags=abi.RENDER_NO_DRAIN | abi.RENDER_NO_LIGHT_GRID), 0, out)),
        "an all-zero normal": (INV, (bad_normal(0, 0, 0), 4, 1, None, 0, out)),
        "a negative-zero normal": (INV, (bad_normal(-0.0, 0, -0.0), 4, 1, None, 0, out)),
        "a NaN in a normal": (INV, (bad_normal(0, np.nan, 1), 4, 1, None, 0, out)),
        "an infinity in a normal": (INV, (bad_normal(-np.inf, 0, 1), 4, 5, None, 0, out)),
    }
    for name, (status, args) in cases.items():
        L.hj_context_create(-1, None)                                  # (leaves ITS text in hj_last_error(NULL))
        before = L.hj_last_error(None)
        assert _call(*args, stats=st) == status, name
        text = L.hj_last_error(None)
        assert text and text != before and b"hj_trace_irradiance" in text, (name, text)
    assert (out == 0).all() and (pts == keep).all()
    assert not any(getattr(st, f) for f, _ in abi.RenderStats._fields_)


def test_refusals_come_in_the_stated_order():
    """Two faults in one call: the earlier check's message."""
    L = device.lib()
    pts, out = _points(), np.zeros((4, 36), F)
    zero = _points()
    zero[0, 3:6] = 0
    for args, word in (((None, 4, 0, None, 8, out), b"null"), ((pts, 4, 0, None, 8, out), b"flag bits"),
                       ((pts, 4, 0, None, abi.GATHER_SH9, out), b"HJ_GATHER_SPHERE"), ((pts, 0x80000000, 0, None, 0, out), b"spp"),
                       ((pts, 0x80000000, 1, _opts(max_bounces=0), 0, out), b"points, at most"),
                       ((zero, 4, 1, _opts(max_bounces=0), 0, out), b"max_bounces"), ((zero, 4, 1, None, 0, out), b"normal")):
        assert _call(*args) == abi.HJ_ERR_INVALID
        assert word in L.hj_last_error(None), (word, L.hj_last_error(None))


def test_a_valid_call_without_a_gpu_is_a_device_error():
    """A process without a HIP device cannot hold a context, so the valid call it can make is one with none.  The normal is not
    read in sphere mode: all-zero normals are valid there."""
    L = device.lib()
    pts, out = _points(), np.full((4, 36), 7.0, F)
    SPH, SH9 = abi.GATHER_SPHERE, abi.GATHER_SH9
    for flags, p, n, spp, o in ((0, pts, 4, 1, None), (SPH, np.zeros((4, 8), F), 4, 65536, _opts(flags=abi.RENDER_NO_LIGHT_GRID)),
                                (SPH | SH9, pts, 4, 3, None), (0, pts, 0, 1, None)):
        rc = _call(p, n, spp, o, flags, out)
        if L.hj_device_count() == 0:
            assert rc == abi.HJ_ERR_DEVICE and b"no HIP device" in L.hj_last_error(None)
        else:
            assert rc == abi.HJ_ERR_INVALID and b"null context" in L.hj_last_error(None)
    assert (out == 7.0).all()


def test_wrapper_checks_its_arguments_before_any_call():
    r = object.__new__(device.Renderer)                                # no context: a check that let a call through would fail on it
    r._h, r.device = None, 0
    good = _points(3)
    keep = good.copy()
    for bad in (good.astype(np.float64), np.zeros((3, 7), F), np.zeros(8, F)):
        with pytest.raises(ValueError):
            r.trace_irradiance(bad)
    for seeds in (np.zeros(3, np.int32), np.zeros(4, U), np.zeros((3, 1), U), np.zeros(3, F)):
        with pytest.raises(ValueError):
            r.trace_irradiance(good, seeds=seeds)
    for spp in (0, 65537, -1):
        with pytest.raises(ValueError):
            r.trace_irradiance(good, spp=spp)
    with pytest.raises(ValueError):
        r.trace_irradiance(good, sh9=True)
    for v in ((0, 0, 0), (np.nan, 0, 1), (0, np.inf, 0)):
        bad = good.copy()
        bad[1, 3:6] = v
        with pytest.raises(ValueError):
            r.trace_irradiance(bad)
    import torch
    for bad in (torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.float64)):      # on the host: not the renderer's GPU
        with pytest.raises(ValueError):
            r.trace_irradiance(bad, sphere=True)
    assert (good == keep).all()


def test_trace_from_states_is_compose():
    """Premise: with the states rng_seed(seeds + k) and the caller's directions, the generalised loop equals
    path_query_ref.compose word for word on the cbox ray set (spp = 1: the cached expectation; spp = 3 on a prefix), counts too."""
    cs, rays = R.scene("cbox"), R.ray_set("cbox")
    want, counts, _ = R.expected("cbox", 40)
    got, got_counts = G.compose_from_states(cs, rays, 1, R.options(40))
    assert np.array_equal(got.view(U), want.view(U)), int((got.view(U) != want.view(U)).sum())
    assert got_counts == counts
    want3, counts3 = R.compose(cs, rays[:300], 3, R.options(40))
    got3, got_counts3 = G.compose_from_states(cs, rays[:300], 3, R.options(40))
    assert np.array_equal(got3.view(U), want3.view(U)) and got_counts3 == counts3


def test_directions_are_the_headers():
    """The reference's directions, from the oracle's scalar entry points one point at a time: the cosine sample in the frame about the
    normal as given (six axis normals: both sides of |n.x| > |n.y| and its tie), the uniform sample with the normal ignored; the
    state behind two draws; the seed wraps."""
    from oracle import hj_oracle as oracle
    pts = G.point_set("cbox")
    idx = [0, 1, 2, 400, 520] + list(range(G.N_POINTS - 6, G.N_POINTS))
    sub = pts[idx]
    assert sub.view(U)[0:3, 6].tolist() == [0, 0xFFFFFFFE, 0xFFFFFFFF]
    d, states = G.directions(sub, 3, False)
    ds, states_s = G.directions(sub, 3, True)
    assert np.array_equal(states, states_s)                             # two draws either way
    one = lambda op, *w: oracle.num_batch(op, U([[int(x) for x in w]]))[0]  # noqa: E731
    for j, p in enumerate(sub):
        n = p[3:6]
        bt = F([0, 1, 0]) if abs(n[0]) > abs(n[1]) else F([1, 0, 0])
        t = one("normalize3", *one("cross3", *n.view(U), *bt.view(U))[:3])[:3].view(F)
        b = one("cross3", *n.view(U), *t.view(U))[:3].view(F)
        for k in range(3):
            s = one("rng_seed", (int(p.view(U)[6]) + k) & 0xFFFFFFFF)[0]
            c = one("rand_cos_hemisphere", s)
            l = c[:3].view(F)
            want = (t * l[0] + b * l[1]) + n * l[2]
            assert np.array_equal(d[j, k].view(U), want.astype(F).view(U)) and states[j, k] == c[3]
            assert np.array_equal(ds[j, k].view(U), one("rand_uniform_sphere", s)[:3])
    tie = sub[-2:, 3:6]
    assert (tie[:, 0] == 0).all() and (tie[:, 1] == 0).all()            # |n.x| > |n.y| is false: bt = (1, 0, 0)
    assert np.isfinite(d).all() and np.isfinite(ds).all()
    assert np.abs(np.linalg.norm(ds.astype(np.float64), axis=2) - 1).max() < 1e-6


def test_point_sets_hold_what_they_claim():
    for name in G.SCENES:
        cs, pts = R.scene(name), G.point_set(name)
        assert pts.shape == (G.N_POINTS, 8) and 550 <= G.N_POINTS <= 650
        lo, hi = R.domain(cs)
        assert ((pts[:, 0:3] >= lo) & (pts[:, 0:3] <= hi)).all()
        length = np.linalg.norm(pts[:, 3:6].astype(np.float64), axis=1)
        free = length[G.N_SURFACE:]                                     # (a populated normal is the shape's: a skewed quad's is short)
        assert length.min() > 0.1 and free.min() >= 0.49 and free.max() <= 2.01 and (np.abs(length[500:560] - 1) > 1e-3).sum() >= 50
        assert pts.view(U)[0:3, 6].tolist() == [0, 0xFFFFFFFE, 0xFFFFFFFF]
        assert np.array_equal(pts[-6:, 3:6], G.AXES)


def test_closed_form_holds_in_the_reference():
    """Points above all geometry, facing up, under a constant environment of 0.5: every cosine sample leaves the scene, so the sum of
    64 samples is exactly 32 in every channel, no first segment hits, and the nearest hit is +inf - in the reference already."""
    cs, pts = G.closed_form_scene(), G.closed_form_points()
    out, counts = G.gather(cs, pts, 64, opts=R.options(40))
    assert (out[:, 0:3] == 32.0).all() and (out[:, 3] == 64.0).all() and (out[:, 4] == 0).all() and np.isposinf(out[:, 5]).all()
    assert (out[:, 6:8] == 0).all() and counts["hits"] == 0 and counts["closest_rays"] == 64 * len(pts)


def test_gather_kernels_add_no_scratch(tmp_path):
    """The compiler's resource report for api/gather_query.hip (the flags are the Makefile's; read as
    test_path_query_kernels_add_no_scratch reads its unit's): all eight k_gq_paths instantiations (pair nodes x environment x
    sphere) are there; each has no more scratch than, the LDS of and at least the occupancy of the fused kernel's explicit-record
    instantiation in the report `make` wrote (its environment twin for the environment instantiations); both k_gq_resolve have
    neither scratch nor LDS."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "gather_query.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "gather_query.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    fused = _report(open(os.path.join(ROOT, "hijiki_amd", "lib", "resource_usage.txt")).read())
    paths = {k: v for k, v in report.items() if "k_gq_paths<" in k}
    assert len(paths) == 8, sorted(report)                              # pair nodes x environment x sphere
    resolve = [v for k, v in report.items() if "k_gq_resolve<" in k]
    assert len(resolve) == 2 and all(v["ScratchSize"] == 0 and v["LDS Size"] == 0 for v in resolve), resolve
    twin = {False: [v for k, v in fused.items() if "k_path_wavefront<true, false, false>" in k],
            True: [v for k, v in fused.items() if "k_path_wavefront_env<true, false, false>" in k]}
    assert len(twin[False]) == 1 and len(twin[True]) == 1, sorted(fused)
    for k, v in paths.items():
        env = re.search(r"k_gq_paths<(?:true|false), true, (?:true|false)>", k) is not None
        print(k, v, "fused twin:", twin[env][0]["ScratchSize"])
        assert v["ScratchSize"] <= twin[env][0]["ScratchSize"], (k, v, twin[env][0])
        assert v["LDS Size"] == twin[env][0]["LDS Size"], (k, v)
        assert v["Occupancy"] >= twin[env][0]["Occupancy"], (k, v)
