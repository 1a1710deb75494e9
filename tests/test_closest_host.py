"""hj_closest_points and hj_distance_field, the part that needs no GPU: the symbols are declared, listed and exported, the version, the
header's defines and the sentences of the contract; every argument refusal in order without a device, with its message and with
nothing written; the reference of the GPU tests (closest_ref) against an independent float64 computation within the bound DESIGN.md
derives, and the skipping rule on that reference's own numbers; every region of the triangle and the quad function a stated number of
times; the sphere's three cases; ties; the radius cases; the compiler's resource report of the unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import closest_ref as R
from hijiki_amd import abi, device
from probe_ref import abi_desc
from test_abi import ROOT, declared_functions
from test_path_query_host import _report

U, F = np.uint32, np.float32
INF, NAN = float("inf"), float("nan")
NAMES = ("hj_closest_points", "hj_distance_field")
u24 = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def design():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    return text[text.index("### Distance queries"):]


def test_entry_points_are_declared_listed_and_exported():
    for name in NAMES:
        assert name in declared_functions("hijiki_hip.h") and name in device.EXPORTS and hasattr(device.lib(), name)
    assert device.lib().hj_version() >= 0x001800
    header = open(os.path.join(ROOT, "include", "hijiki_hip.h")).read()
    for text in ("#define HJ_CLOSEST_DEVICE_ARRAYS 1u", "#define HJ_CLOSEST_WORDS 8u", "#define HJ_DISTANCE_UNSIGNED 1u", "Distance queries (ABI 0.24)",
                 "smallest key (d2 as uint32 bits, global shape index)", "not on the tree, the visiting order", "rectangles only",
                 "NaN included", "trees whose boxes bound their subtrees", "whatever the skipping gives", "not a robust",
                 "A refused call writes nothing", "a miss is -1 followed by seven zeros"):
        assert text in header, text
    kernel = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_closest.h")).read()
    for text in ("Ericson", "whatever the skipping gives", "trees whose boxes bound their subtrees", "rectangles", "no global atomics"):
        assert text.lower() in kernel.lower(), text
    assert (abi.CLOSEST_DEVICE_ARRAYS, abi.CLOSEST_WORDS, abi.DISTANCE_UNSIGNED) == (1, 8, 1) and R.WORDS == 8
    for fn in ("closest_points", "distance_field"):
        assert callable(getattr(device.Renderer, fn)) and "not a robust" in " ".join(getattr(device.Renderer, fn).__doc__.split())


def test_the_slack_is_one_number_in_the_design_the_header_and_the_reference():
    d = design()
    m = re.search(r"slack = 2\^-(\d+) \* M", d)
    assert m and 2.0 ** -int(m.group(1)) == float(R.SLACK)
    g = re.search(r"grow = 1 \+ 2\^-(\d+)", d)
    assert g and F(1.0 + 2.0 ** -int(g.group(1))) == R.GROW
    kernel = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_closest.h")).read()
    assert float(re.search(r"kCqSlack = ([0-9.e+-]+)f", kernel).group(1)) == float(R.SLACK)
    assert F(float(re.search(r"kCqGrow = ([0-9.e+-]+)f", kernel).group(1))) == R.GROW
    a, r = re.search(r"sqrt\(d2\) >= \(1 - (\d+) u\) \* max\(0, D - (\d+) u M\)", d).groups()
    assert (int(r), int(a)) == (ABS_U, REL_U) and ABS_U * u24 < float(R.SLACK)


# -------------------------------------------------------------------------------------------------------------------- refusals

def _refused(call, name, word, status=abi.HJ_ERR_INVALID):
    L = device.lib()
    L.hj_context_create(-1, None)                                      # (leaves ITS text in hj_last_error(NULL))
    before = L.hj_last_error(None)
    assert call() == status, (name, word)
    text = L.hj_last_error(None)
    assert text and text != before and (name.encode() + b":") in text and word in text, (name, word, text)


def test_argument_refusals_come_before_the_device_in_order():
    L = device.lib()
    pts, out, st = np.full((3, 4), 7.0, F), np.full((3, 8), 7.0, F), (C.c_uint64 * 2)(7, 7)
    P, O = pts.ctypes.data, out.ctypes.data
    cp = lambda p=P, n=3, f=0, o=O, s=st: (lambda: L.hj_closest_points(None, p, n, f, o, s))      # noqa: E731
    name = NAMES[0]
    # each refusal alone, then each in front of every later one: the order
    order = [(b"null points", dict(p=None)), (b"unknown flag bits", dict(f=2)), (b"at most 2^31 - 1", dict(n=1 << 31)),
             (b"16-byte aligned", dict(f=1, p=P + 4))]
    for k, (word, kw) in enumerate(order):
        _refused(cp(**kw), name, word)
        for _, later in order[k + 1:]:
            merged = dict(later, **kw)
            if word == b"16-byte aligned" or (word == b"unknown flag bits" and "f" in later):
                continue
            _refused(cp(**merged), name, word)
    _refused(cp(o=None), name, b"null out")
    _refused(cp(f=0x80000000), name, b"unknown flag bits")
    _refused(cp(f=1, o=O + 8), name, b"16-byte aligned")
    _refused(cp(n=(1 << 31) - 1 + 1), name, b"points")
    # past the argument checks: no context (and here no device)
    status = abi.HJ_ERR_DEVICE if L.hj_device_count() == 0 else abi.HJ_ERR_INVALID
    _refused(cp(), name, b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context", status)
    _refused(cp(n=0, p=None, o=None), name, b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context", status)
    _refused(cp(f=1, p=P, o=O), name, b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context", status)   # (aligned host stats pass)

    field = np.full(8, 7.0, F)
    df = lambda d=abi_desc(), m=1.0, f=0, o=field.ctypes.data: (lambda: L.hj_distance_field(None, C.byref(d) if d is not None else None, m, f, o))   # noqa: E731
    name = NAMES[1]
    _refused(df(d=None), name, b"null desc")
    _refused(df(o=None), name, b"null field")
    for word, kw in ((b": unknown flag bits", dict(flags=2)), (b"count", dict(count=(0, 1, 1))), (b"origin", dict(origin=(NAN, 0, 0))),
                     (b"spacing", dict(spacing=(0, 1, 1))), (b"min_distance", dict(min_distance=-1.0))):
        _refused(df(d=abi_desc(**kw), f=2, m=-1.0), name, word)
    _refused(df(f=2, m=-1.0), name, b"unknown distance flag bits")
    for m in (-1.0, NAN, -INF):
        _refused(df(m=m, d=abi_desc(flags=abi.PROBES_DEVICE_ARRAYS), o=field.ctypes.data + 4), name, b"max_distance")
    _refused(df(d=abi_desc(flags=abi.PROBES_DEVICE_ARRAYS), o=field.ctypes.data + 4), name, b"16-byte aligned")
    _refused(df(m=INF), name, b"no HIP device" if status == abi.HJ_ERR_DEVICE else b"null context", status)
    assert (pts == 7.0).all() and (out == 7.0).all() and (field == 7.0).all() and list(st) == [7, 7]


# -------------------------------------------------------------------------------------------------- the reference and the bound

ABS_U, REL_U = 45, 6            # the bound DESIGN.md derives: sqrt(d2) >= (1 - 6 u) * max(0, D - 45 u M), u = 2^-24


def _random_shapes(rng, n, offset, rect=True):
    """n spheres, n rectangles, n triangles of size about 1 around `offset`, plus slivers and tiny ones"""
    c = rng.uniform(-1, 1, (n, 3)) + offset
    sph = np.concatenate([c, rng.uniform(0.05, 0.7, (n, 1))], 1).astype(F)
    a = rng.uniform(-1, 1, (n, 3))
    b = np.cross(a, rng.uniform(-1, 1, (n, 3)))                                # orthogonal to a in float64; float32 rounds it a little
    quads = np.stack([rng.uniform(-1, 1, (n, 3)) + offset, a, b / np.linalg.norm(b, axis=1, keepdims=True) * rng.uniform(0.1, 1, (n, 1))], 1).astype(F)
    tri = rng.uniform(-1, 1, (n, 3, 3)) + offset
    tri[n // 2:, 2] = tri[n // 2:, 0] + (tri[n // 2:, 1] - tri[n // 2:, 0]) * rng.uniform(0, 1, (n - n // 2, 1)) + rng.normal(size=(n - n // 2, 3)) * 1e-4   # slivers
    tri[: n // 8] = tri[: n // 8, 0:1] + (tri[: n // 8] - tri[: n // 8, 0:1]) * 1e-3                                                         # tiny
    tri = tri.astype(F)
    t = np.stack([tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]], 1).astype(F)
    return dict(spheres=sph, quads=quads, triangles=t)


def _points_about(rng, sh, m):
    """points for every shape: a random cloud, points ON the shapes (the reference's own q of the cloud) pushed 0, 1 and 2 ulps along
    each axis, and points 1e6 away"""
    lo = min(x[..., :3].min() for x in (sh["spheres"], sh["quads"][:, 0], sh["triangles"][:, 0])) - 2
    cloud = rng.uniform(lo, lo + 6, (m, 3)).astype(F)
    q = R.per_shape(sh, cloud)[0]                                               # (m, N, 3)
    on = q[np.arange(m), rng.integers(0, q.shape[1], m)]
    on = on[np.isfinite(on).all(1)]
    near = [on]
    for k in (1, 2):
        up, dn = on.copy(), on.copy()
        for _ in range(k):
            up, dn = np.nextafter(up, F(np.inf)), np.nextafter(dn, F(-np.inf))
        near += [up, dn]
    far = (rng.normal(size=(16, 3)) * 1e6).astype(F)
    return np.concatenate([cloud] + near + [far]).astype(F)


def test_reference_against_float64_within_the_derived_bound():
    """Per (point, shape): the reference's sqrt(d2) against the float64 distance D to the shape itself (>= the distance to any box
    around it), M the largest coordinate magnitude of the shapes' boxes, u = 2^-24:
      * the derivation's statement, on every pair:  sqrt(d2) >= (1 - 6 u) * max(0, D - 45 u M);
      * both ways within the slack, |sqrt(d2) - D| <= 45 u M + 6 u D, on every pair but the slivers': spheres, rectangles, ordinary
        and tiny (1e-3) triangles, points on the shapes and 1 and 2 floats off them, points 1e6 away, at offsets 0, 1000, 30000;
      * slivers (a third vertex 1e-4 off the opposite edge): the region tests decide on cancelled areas, q is a point of the
        triangle but need not be the nearest one, so only sqrt(d2) <= (1 + 6 u) * (D + diameter) + 45 u M holds;
      * the skipping rule at the pair's own d2 never skips the shape's own box.
    Observed (printed): off slivers the excess over 6 u D is at most 1.47 u M where 45 u M is allowed.  On slivers at most 0.09 % of
    a set's pairs leave the two-sided bound, and the largest error is 0.199 scene units on triangles about 1 unit long: the
    accuracy the text gives up on slivers - the answer there is the text's bit for bit, not the true nearest point."""
    rng = np.random.default_rng(2024)
    worst_lo, worst_abs, sliver_share, sliver_err = -INF, 0.0, 0.0, 0.0
    n = 24
    for offset in (0.0, 1000.0, 30000.0):
        sh = _random_shapes(rng, n, offset)
        pts = _points_about(rng, sh, 120)
        q, d2, u, v, side = R.per_shape(sh, pts)
        D = R.exact_distance(sh, pts)
        ok = ~np.isnan(d2)
        assert ok.mean() > 0.99
        # the shapes' boxes as the builders compute them (float32 min / max of float32 corners), and M of their union
        s, qd, t = sh["spheres"], sh["quads"], sh["triangles"]
        tri_c = np.stack([t[:, 0], (t[:, 0] + t[:, 1]).astype(F), (t[:, 0] + t[:, 2]).astype(F)], 1)
        quad_c = np.stack([qd[:, 0], (qd[:, 0] + qd[:, 1]).astype(F), (qd[:, 0] + qd[:, 2]).astype(F), ((qd[:, 0] + qd[:, 1]).astype(F) + qd[:, 2]).astype(F)], 1)
        lo = np.concatenate([(s[:, :3] - s[:, 3:]).astype(F), quad_c.min(1), tri_c.min(1)])
        hi = np.concatenate([(s[:, :3] + s[:, 3:]).astype(F), quad_c.max(1), tri_c.max(1)])
        M = float(max(np.abs(lo).max(), np.abs(hi).max()))
        diam = np.linalg.norm(hi.astype(np.float64) - lo, axis=1)[None]
        dist = np.sqrt(d2.astype(np.float64))
        lower = (1 - REL_U * u24) * np.maximum(0.0, D - ABS_U * u24 * M)
        assert (dist[ok] >= lower[ok]).all(), (offset, float((lower - dist)[ok].max() / (u24 * M)))
        upper = (1 + REL_U * u24) * (D + diam) + ABS_U * u24 * M
        assert (dist[ok] <= upper[ok]).all(), (offset, float((dist - upper)[ok].max() / (u24 * M)))
        worst_lo = max(worst_lo, float((lower - dist)[ok].max() / (u24 * M)))
        sliver = np.zeros(d2.shape, bool)
        sliver[:, 2 * n + n // 2:] = True
        good = ~sliver                                                          # far points and tiny triangles included
        err = np.abs(dist - D)
        assert ok[good].all() and (err[good] <= ABS_U * u24 * M + REL_U * u24 * D[good]).all(), (offset, float((err - REL_U * u24 * D)[good].max() / (u24 * M)))
        worst_abs = max(worst_abs, float(np.maximum(err - REL_U * u24 * D, 0)[good].max() / (u24 * M)))
        over = ok & sliver & (err > ABS_U * u24 * M + REL_U * u24 * D)
        sliver_share, sliver_err = max(sliver_share, float(over.sum() / sliver.sum())), max(sliver_err, float(err[ok & sliver].max()))
        # the skipping rule on its own leaf: with the limit at the pair's own d2 the shape's box must not be skipped
        p = np.broadcast_to(pts[:, None, :], q.shape)
        bd = R.box_d2(p, np.broadcast_to(lo[None], q.shape), np.broadcast_to(hi[None], q.shape))
        skipped = bd > R.skip_above(d2, R.SLACK * F(M))
        assert not skipped[ok].any(), (offset, int(skipped[ok].sum()))
    print(f"largest (lower bound - sqrt(d2)) / (u M), all pairs: {worst_lo:.2f}; largest (|sqrt(d2) - D| - 6 u D) / (u M) off slivers: {worst_abs:.2f}; "
          f"slivers: at most {sliver_share:.4f} of a set's pairs beyond the bound, largest error {sliver_err:.4f} scene units")


# ------------------------------------------------------------------------------------------------------ regions and special cases

TRI = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)                          # (a, ab, ac)


def test_every_region_of_the_triangle_function_once_each_and_twice_off_plane():
    """7 points in the plane, one per region in the header's numbering, and the same 7 lifted to z = +2 and z = -2: regions 1 ... 7 three
    times each, known answers exactly (every value is a dyadic rational)."""
    xy = np.array([[-1, -1], [2, -0.5], [-0.5, 2], [0.5, -1], [-1, 0.5], [1, 1], [0.25, 0.25]], F)
    uv = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5], [0.25, 0.25]], F)
    for z in (0.0, 2.0, -2.0):
        p = np.concatenate([xy, np.full((7, 1), z, F)], 1)
        q, d2, u, v, side, region = R.triangle(p, TRI, region=True)
        assert region.tolist() == [1, 2, 3, 4, 5, 6, 7]
        assert (u == uv[:, 0]).all() and (v == uv[:, 1]).all() and (q[:, :2] == uv).all() and (q[:, 2] == 0).all()
        assert (d2 == ((xy - uv) ** 2).sum(1) + F(z * z)).all()
        assert (side == (1.0 if z >= 0 else -1.0)).all()
    # a degenerate triangle is what the text computes: a zero edge ab gives 0 / 0 on the edge ab, a point triangle its vertex
    q, d2, u, v, side = R.triangle(np.array([[0.5, 0.5, 0]], F), np.array([[[0, 0, 0], [0, 0, 0], [0, 1, 0]]], F))
    assert np.isnan(d2).all() and np.isnan(u).all()
    q, d2, u, v, side = R.triangle(np.array([[3, 4, 0]], F), np.zeros((1, 3, 3), F))
    assert d2.tolist() == [25.0] and (u, v) == (0, 0)


def test_every_region_of_the_quad_function_once_each():
    """4 corners, 4 edges, the face: the nine (s, t) clamp classes once each on a 2 x 1 rectangle, known answers exactly."""
    quad = np.array([[[0, 0, 0], [2, 0, 0], [0, 1, 0]]], F)
    xs, ys = [-1.0, 0.5, 3.0], [-1.0, 0.5, 2.0]
    p = np.array([[x, y, 0.5] for y in ys for x in xs], F)
    q, d2, u, v, side, (cs, ct) = R.quad(p, quad, region=True)
    assert sorted(zip(cs.tolist(), ct.tolist())) == [(a, b) for a in range(3) for b in range(3)]
    want = np.stack([np.clip(p[:, 0], 0, 2), np.clip(p[:, 1], 0, 1), np.zeros(9, F)], 1)
    assert (q == want).all() and (u == want[:, 0] / 2).all() and (v == want[:, 1]).all() and (side == 1).all()
    assert (d2 == ((p - want) ** 2).sum(1)).all()
    assert (R.quad(p * F([1, 1, -1]), quad)[4] == -1).all()
    # a sheared quad: a point of the quad, not the nearest (the header says so)
    sheared = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0]]], F)
    q, d2 = R.quad(np.array([[2, 0.5, 0]], F), sheared)[:2]
    assert d2[0] == 0.25 and R.exact_distance(dict(spheres=np.zeros((0, 4), F), quads=sheared, triangles=np.zeros((0, 3, 3), F)), np.array([[2, 0.5, 0]], F))[0, 0] ** 2 < 0.126


def test_the_sphere_at_its_centre_inside_and_on_the_surface():
    s = np.array([[1, -0.0, 3, 2]], F)
    q, d2, u, v, side = R.sphere(np.array([[1, 0, 3], [1, 1, 3], [1, 0, 5], [1, 0, 7]], F), s)
    assert (q == np.array([[3, 0, 3], [1, 2, 3], [1, 0, 5], [1, 0, 5]], F)).all() and bits(q[0, 1]) == 0
    assert d2.tolist() == [4.0, 1.0, 0.0, 4.0] and side.tolist() == [-1.0, -1.0, 1.0, 1.0] and not u.any() and not v.any()


def _one(sh, p, r=INF):
    return R.closest(sh, np.array([list(p) + [r]], F))[0]


def test_ties_resolve_to_the_lower_index_and_the_radius_cases():
    none4, none33 = np.zeros((0, 4), F), np.zeros((0, 3, 3), F)
    # the same triangle twice behind a sphere that is farther: index 1, not 2; with the sphere as near as the triangles: index 0
    sh = dict(spheres=np.array([[0.25, 0.25, 5, 2]], F), quads=none33, triangles=np.concatenate([TRI, TRI]))
    rec = _one(sh, (0.25, 0.25, 1))
    assert R.ids(rec[None])[0] == 1 and rec[1] == 1.0
    sh["spheres"][0, 3] = 3.0
    rec = _one(sh, (0.25, 0.25, 1))
    assert R.ids(rec[None])[0] == 0 and rec[1] == 1.0 and rec[7] == 1.0
    # radius: +inf, 0 (only a point ON a shape), the distance itself, one float below it, NaN, negative; a non-finite point
    sh = dict(spheres=none4, quads=none33, triangles=TRI)
    miss = np.zeros(8, F)
    miss[0] = np.int32(-1).view(F)
    p = (0.25, 0.25, 0.75)
    hit = _one(sh, p)
    assert R.ids(hit[None])[0] == 0 and hit[1] == 0.75 and hit.tolist()[2:] == [0.25, 0.25, 0.0, 0.25, 0.25, 1.0]
    assert (bits(_one(sh, p, 0.75)) == bits(hit)).all()
    for r in (0.0, float(np.nextafter(F(0.75), F(0))), NAN, -1.0, -INF):
        assert (bits(_one(sh, p, r)) == bits(miss)).all(), r
    assert R.ids(_one(sh, (0.25, 0.25, 0.0), 0.0)[None])[0] == 0 and R.ids(_one(sh, (0.25, 0.25, 0.0), -0.0)[None])[0] == 0
    for bad in ((NAN, 0, 0), (0, INF, 0), (0, 0, -INF)):
        assert (bits(_one(sh, bad)) == bits(miss)).all()
    # no shapes at all
    assert (bits(_one(dict(spheres=none4, quads=none33, triangles=none33), p)) == bits(miss)).all()
    # the field: a miss gives +max_distance, signed or not
    f = R.distance_field(sh, (0.25, 0.25, -2), (1, 1, 1), (1, 1, 5), 1.5)
    assert f.shape == (5, 1, 1) and f.ravel().tolist() == [1.5, -1.0, 0.0, 1.0, 1.5]
    assert R.distance_field(sh, (0.25, 0.25, -2), (1, 1, 1), (1, 1, 5), 1.5, signed=False).ravel().tolist() == [1.5, 1.0, 0.0, 1.0, 1.5]


# ------------------------------------------------------------------------------------------------------------- the compiled unit

def test_closest_query_kernels_use_no_scratch(tmp_path):
    """The compiler's resource report for api/closest_query.hip (the Makefile's flags): exactly the kernels of hj_closest.h (the walk in its four instantiations) - no
    kernel of hj_probes.h is compiled a second time -, none has scratch, LDS only for the statistics' sums and the ordered walk's stack.  The flags are read from the Makefile.  Occupancy is
    printed, not gated."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    joined = mk.replace("\\\n", " ")                                                                 # (continuation lines)
    var = lambda name: re.search(rf"^{name} = (.*)$", joined, re.M).group(1)                          # noqa: E731
    flags = var("HIP_FLAGS").replace("$(ARCH)", "gfx950").replace("$(FP_STRICT)", var("FP_STRICT")).replace("$(HIP_EXTRA)", "").split()
    assert "-fPIC" in flags and "-fvisibility=hidden" in flags and "-ffp-contract=off" in flags and "-O3" in flags
    cmd = ["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "closest_query.o"),
           os.path.join(ROOT, "hijiki_amd", "csrc", "api", "closest_query.hip")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr[-2000:]
    report = _report(out.stderr)
    names = {re.search(r"k_cq_[a-z]+(<\w+, \w+>)?", k).group(0): v for k, v in report.items()}
    walks = [f"k_cq_walk<{a}, {b}>" for a in ("false", "true") for b in ("false", "true")]                # <STATS, ORDERED>
    assert sorted(names) == ["k_cq_pack", "k_cq_resolve"] + walks and len(report) == 6, sorted(report)
    for k, v in names.items():
        assert v["ScratchSize"] == 0, (k, v)
        lds = (64 if "<true," in k else 0) + (32 * 256 * 4 if ", true>" in k else 0)                    # the statistics' sums, the stack
        assert v["LDS Size"] == lds, (k, v)
        print(f"{k}: {v['VGPRs']} VGPRs, {v['TotalSGPRs']} SGPRs, LDS {v['LDS Size']} B, occupancy {v['Occupancy']} waves per SIMD")
    src = open(os.path.join(ROOT, "hijiki_amd", "csrc", "kernels", "hj_closest.h")).read()
    assert "atomic" not in src.replace("no global atomics", "") and "asm" not in src.replace("no inline assembly", "")
    assert '"hj_closest.h"' in open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
