"""k_pv_points, k_pv_resolve and k_pv_sample at their size and value edges, bit for bit against probe_ref (test_probes_gpu.py runs
them in the middle of their domain): the points at 1024 planes an axis and at 2^22 probes with seed products that pass 2^32 many
times; the look-up on 1024-plane axes around planes 0, 1, 255, 256, 1022 and 1023 and in a 2^22-probe volume that exists on the
device alone (probe_ref.hashed_volume; the reference reads the probes it needs through a callable); the bake beyond one resolve
workgroup and at 65536 spp; the look-up's arithmetic edges (probe_edges: subnormal weights and quotients, spacings of 1e-45 and 3e38,
pos - origin overflowing, one ulp either side of every plane, -0.0, validities that cancel, are huge, infinite or NaN, non-finites
behind a zero validity, normals no unit vector comes from) under DESIGN.md's rule "a NaN equals any NaN"; the validity rule at
min_distance = FLT_MAX, at the smallest nearest hit and one ulp above it; the context's kept buffers across sizes that shrink."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G
import path_query_ref as R
import probe_edges as E
import probe_ref as P
from hijiki_amd import abi, device
from test_probes_gpu import assert_bits, grid_kw

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
GRID = dict(origin=(0.5, -1.0, 2.0), spacing=(0.5, 0.25, 1.5))
SEED, STRIDE = 0xFFFFFFF0, 7


@pytest.fixture(scope="module")
def pv():
    with device.Renderer(0) as ctx:
        yield ctx


def cuda():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, F, order="C")).to(cuda())       # (a copy: the shared cases are read-only)


# ------------------------------------------------------------------------------------------------------------------ size edges

def wrapped(count):
    return P.desc((-1.25, 0.5, 3.0), (0.3, 0.7, 0.011), count, E.WRAP_SEED, E.WRAP_STRIDE)


@pytest.mark.parametrize("count", E.AXIS_LIMIT)
def test_points_at_the_axis_limit(pv, count):
    """1024 planes on each axis in turn; seed + p * 0x9E3779B1 from a seed near 2^32: the product passes 2^32 from p = 2 on"""
    d = wrapped(count)
    want = P.points(d)
    p = np.arange(len(want), dtype=object)
    assert int((p * E.WRAP_STRIDE >= 1 << 32).sum()) == len(want) - 2 and int(p[-1] * E.WRAP_STRIDE) >> 32 >= 632
    kw = grid_kw(d, seed=E.WRAP_SEED, seed_stride=E.WRAP_STRIDE)
    assert_bits(pv.probe_points(**kw), want, f"points {count}, host arrays")
    assert_bits(pv.probe_points(**kw, device=True).cpu().numpy(), want, f"points {count}, device arrays")


@pytest.mark.parametrize("count", E.PROBE_LIMIT)
def test_points_at_the_probe_limit(pv, count):
    """2^22 probes, 16384 workgroups: every index word, every position, every wrapped seed"""
    d = wrapped(count)
    want = P.points(d)
    assert len(want) == 1 << 22
    got = pv.probe_points(**grid_kw(d, seed=E.WRAP_SEED, seed_stride=E.WRAP_STRIDE), device=True).cpu().numpy()
    assert_bits(got, want, f"points {count}, device arrays")


@pytest.mark.parametrize("count", E.LONG_AXES)
def test_lookup_on_long_axes(pv, count):
    """an axis of 1024 planes in each place: 4161 points of probe_ref.sample_points (NaN and infinite positions on the device route),
    points on and one ulp either side of planes 0, 1, 255, 256, 1022 and 1023, points in the first, a middle and the last cell"""
    d = P.desc(GRID["origin"], GRID["spacing"], count)
    vol = P.fabricated_volume(count, 9)
    assert vol.size // 28 <= 4096
    pts = E.limit_points(d, 3)
    want, w, wsum, q = P.sample(d, vol, pts, detail=True)
    assert q.max() == vol.size // 28 - 1 and q.min() == 0 and np.isfinite(want).all()
    got = pv.sample_probes(to_dev(vol), GRID["origin"], GRID["spacing"], to_dev(pts))
    assert_bits(got.cpu().numpy(), want, f"sample {count}, device arrays")
    ok = E.host_route(pts)
    assert ok.sum() > 3300
    assert_bits(pv.sample_probes(vol, GRID["origin"], GRID["spacing"], pts[ok]), want[ok], f"sample {count}, host arrays")


@pytest.mark.parametrize("count", E.PROBE_LIMIT)
def test_lookup_at_the_probe_limit(pv, count):
    """2^22 probes (470 MB) built on the device as a function of (probe, word); the reference asks for the 8 x 4206 records it reads.
    The float4 index q * 7 + 6 reaches 2^22 * 7 - 1."""
    import torch
    d = P.desc(GRID["origin"], GRID["spacing"], count)
    n = count[0] * count[1] * count[2]
    tvol = P.hashed_volume(count, cuda(), slab=1 << 18)
    pts = E.limit_points(d, 5)
    seen = []

    def records(q):
        seen.append(q)
        return P.hashed_records(q)
    want = P.sample(d, records, pts)
    read = np.concatenate(seen)
    assert read.max() == n - 1 and read.min() == 0 and int((read > 1 << 21).sum()) > 1000
    assert np.isfinite(want).all() and (want[:, 3] == 0).any() and (want[:, 3] > 0).sum() > 3000
    got = pv.sample_probes(tvol, GRID["origin"], GRID["spacing"], to_dev(pts))
    assert_bits(got.cpu().numpy(), want, f"sample {count}, device arrays")
    # a slab boundary and the two ends of what torch built, against the numpy records
    for a in (0, (1 << 18) - 2, n - 4):
        assert_bits(tvol.reshape(n, 28)[a:a + 4].cpu().numpy(), P.hashed_records(np.arange(a, a + 4)), f"hashed_volume, probes {a} ...")
    del tvol
    torch.cuda.empty_cache()


def composed(r, d, spp):
    """the bake from its public parts: probe_points -> trace_irradiance(sphere, sh9) -> probe_ref.resolve; also the records"""
    pts = r.probe_points(**grid_kw(d, seed=SEED, seed_stride=STRIDE))
    rec, stats = r.trace_irradiance(pts, spp=spp, sphere=True, sh9=True, opts=R.options(40), stats=True)
    return P.resolve(rec, spp, d["min_distance"]), stats, rec


def check_bake(pv, d, spp, what):
    """host arrays, device arrays, and the raw call into a tensor with a guard pattern behind the volume"""
    import torch
    want, want_stats, rec = composed(pv, d, spp)
    n = len(want)
    kw = grid_kw(d, seed=SEED, seed_stride=STRIDE, min_distance=float(d["min_distance"]))
    for dev in (False, True):
        got, stats = pv.bake_probes(**kw, spp=spp, opts=R.options(40), stats=True, device=dev)
        got = got.cpu().numpy() if dev else got
        assert_bits(got.reshape(-1, 28), want, f"{what}, {'device' if dev else 'host'} arrays")
        assert {k: stats[k] for k in G.COUNTS} == {k: want_stats[k] for k in G.COUNTS}, what
    out = torch.full((n + 64, 28), 7.0, dtype=torch.float32, device=cuda())
    torch.cuda.synchronize()
    dd = P.abi_desc(d["origin"], d["spacing"], d["count"], SEED, STRIDE, float(d["min_distance"]), abi.PROBES_DEVICE_ARRAYS)
    assert device.lib().hj_bake_probes(pv._h, C.byref(dd), spp, C.byref(R.options(40)), out.data_ptr(), None) == abi.HJ_OK
    assert_bits(out[:n].cpu().numpy(), want, f"{what}, raw call")
    assert (out[n:] == 7.0).all(), "written beyond the volume"
    return want, rec


def test_bake_beyond_one_resolve_workgroup(pv):
    """315 probes: a second workgroup of k_pv_resolve with 59 live threads.  min_distance is the median of the distinct finite nearest
    hits of those 59 (the GPU's own records), so that word 27 is not one constant among them."""
    cs = R.scene("cbox")
    pv.upload_scene(cs)
    d = P.grid_in_domain(cs, (9, 5, 7))
    near = composed(pv, d, 3)[2][256:, 5]
    near = np.unique(near[np.isfinite(near)])
    assert len(near) >= 2, near
    d = dict(d, min_distance=near[len(near) // 2])
    want, rec = check_bake(pv, d, 3, f"bake (9, 5, 7), spp 3, min_distance {near[len(near) // 2]!r}")
    print("valid", int(want[:, 27].sum()), "of", len(want), "; beyond probe 255:", int(want[256:, 27].sum()))
    assert len(want) == 315 and (want[256:, 0:27] != 0).any() and len(np.unique(want[256:, 27])) == 2


def test_bake_at_the_spp_limit(pv):
    """(2, 1, 1) at spp 65536: s = 12.5663706f / 65536.0f, 131 072 paths"""
    cs = R.scene("cbox")
    pv.upload_scene(cs)
    d = P.grid_in_domain(cs, (2, 1, 1))
    want, rec = check_bake(pv, d, 65536, "bake (2, 1, 1), spp 65536")
    assert (rec[:, 3] == 65536).all() and np.isfinite(want).all() and (want[:, 0:3] > 0).all()


# ----------------------------------------------------------------------------------------------------------------- value edges

FAMILIES = {"grids": lambda n: "; mixed validity" in n, "subnormal weights": lambda n: "spacing" in n and "invalid with NaN behind" in n,
            "volumes": lambda n: ", ordinary; " in n and "; mixed validity" not in n and "the normals" not in n, "normals": lambda n: "the normals" in n}


def test_the_families_split_the_edge_set():
    names = [g["name"] for g in E.edge_cases()]
    assert sorted(n for f in FAMILIES.values() for n in names if f(n)) == sorted(names)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_lookup_at_value_edges(pv, family):
    """Every group of the edge set on the device route, and on the host route the rows it admits (finite positions, finite normals
    that are not all zero).  Where the reference's word is a NaN the GPU's must be one; every other word by its bits."""
    groups = [g for g in E.edge_cases() if FAMILIES[family](g["name"])]
    assert groups
    rows = covered = 0
    for g in groups:
        d, pts = g["d"], g["pts"]
        vol = g["volume"].reshape(d["count"][2], d["count"][1], d["count"][0], 28)
        want = P.sample(d, vol, pts)
        got = pv.sample_probes(to_dev(vol), d["origin"], d["spacing"], to_dev(pts))
        covered += E.assert_bits_or_nan(got.cpu().numpy(), want, g["name"] + ", device arrays", g["names"])
        rows += len(pts)
        ok = E.host_route(pts)
        names = [n for n, k in zip(g["names"], ok) if k]
        E.assert_bits_or_nan(pv.sample_probes(vol, d["origin"], d["spacing"], pts[ok]), want[ok], g["name"] + ", host arrays", names)
    print(f"{family}: {len(groups)} groups, {rows} rows, the NaN rule covered {covered}")


@pytest.mark.parametrize("name,d", E.point_grids(), ids=[n for n, _ in E.point_grids()])
def test_points_at_value_edges(pv, name, d):
    want = P.points(d)
    kw = grid_kw(d, seed=d["seed"], seed_stride=d["seed_stride"])
    assert_bits(pv.probe_points(**kw), want, name + ", host arrays")
    assert_bits(pv.probe_points(**kw, device=True).cpu().numpy(), want, name + ", device arrays")


# ------------------------------------------------------------------------------------------------------- the validity rule's ends

def test_validity_rule_at_its_ends(pv):
    """rich, (5, 4, 3), spp 1: the GPU's own nearest-hit column holds +inf (the probe's one sample hit nothing) and finite values.
    min_distance = FLT_MAX: exactly the probes without a hit are valid; the smallest finite nearest hit: every probe; one ulp
    above it: that probe alone is not.  The coefficients are the same words in all three."""
    cs = R.scene("rich")
    pv.upload_scene(cs)
    d0 = P.grid_in_domain(cs, (5, 4, 3))
    _, _, rec = composed(pv, d0, 1)
    near = rec[:, 5]
    assert np.isposinf(near).any() and np.isfinite(near).any() and not np.isnan(near).any(), near
    least = near.min()
    assert least > 0
    vols = []
    for md, valid in ((F(3.4028235e38), np.isposinf(near)), (least, np.ones(len(near), bool)), (np.nextafter(least, F(np.inf)), near != least)):
        d = dict(d0, min_distance=md)
        want = P.resolve(rec, 1, md)
        assert (want[:, 27] == valid).all() and (near != least).sum() == len(near) - (near == least).sum() and (near == least).sum() >= 1
        for dev in (False, True):
            got = pv.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE, min_distance=float(md)), spp=1, opts=R.options(40), device=dev)
            got = (got.cpu().numpy() if dev else got).reshape(-1, 28)
            assert_bits(got, want, f"min_distance {md!r}, {'device' if dev else 'host'} arrays")
            vols.append(got)
    for v in vols[1:]:
        assert_bits(v[:, 0:27], vols[0][:, 0:27], "the coefficients under another min_distance")
    assert (near == least).sum() == 1


# ----------------------------------------------------------------------------------------------------- kept buffers across sizes

@pytest.mark.parametrize("dev", [False, True], ids=["host arrays", "device arrays"])
def test_kept_buffers_across_sizes(pv, dev):
    """One fresh context, sizes that shrink and grow: a larger call leaves nothing behind that a smaller one picks up."""
    cs = R.scene("cbox")
    pv.upload_scene(cs)
    big, small = P.desc(GRID["origin"], GRID["spacing"], (5, 4, 3)), P.desc(GRID["origin"], GRID["spacing"], (2, 2, 2))
    vol_big, vol_small = P.fabricated_volume((5, 4, 3), 9), P.fabricated_volume((2, 2, 2), 9)
    pts_big, pts_one = P.sample_points(big, 260, 3), P.sample_points(small, 1, 3)
    bake_small, bake_big = P.grid_in_domain(cs, (3, 2, 2)), P.grid_in_domain(cs, (5, 4, 3))
    want_small, want_big = composed(pv, bake_small, 4)[0], composed(pv, bake_big, 4)[0]      # (the module's context: another one's buffers)
    grid = P.desc((-1.25, 0.5, 3.0), (0.3, 0.7, 0.011), (64, 1, 65), SEED, STRIDE)

    def host(x):
        return x.cpu().numpy() if dev else x

    def lookup(r, d, vol, pts):
        if dev:
            return host(r.sample_probes(to_dev(vol), d["origin"], d["spacing"], to_dev(pts)))
        return r.sample_probes(vol, d["origin"], d["spacing"], pts)

    def bake(r, d):
        return host(r.bake_probes(**grid_kw(d, seed=SEED, seed_stride=STRIDE), spp=4, opts=R.options(40), device=dev)).reshape(-1, 28)
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        first = lookup(r, big, vol_big, pts_big)
        assert_bits(first, P.sample(big, vol_big, pts_big), "1. look-up (5, 4, 3), 260 points")
        assert_bits(bake(r, bake_small), want_small, "2. bake (3, 2, 2)")
        assert_bits(lookup(r, small, vol_small, pts_one), P.sample(small, vol_small, pts_one), "3. look-up (2, 2, 2), 1 point")
        assert_bits(host(r.probe_points(**grid_kw(grid, seed=SEED, seed_stride=STRIDE), device=dev)), P.points(grid), "4. points (64, 1, 65)")
        assert_bits(bake(r, bake_big), want_big, "5. bake (5, 4, 3)")
        assert_bits(lookup(r, big, vol_big, pts_big), first, "6. the first look-up again")
        assert_bits(bake(r, bake_small), want_small, "7. the small bake again")
