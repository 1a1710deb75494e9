"""The value edges of hj_sample_probes and hj_probe_points as fabricated, deterministic cases: grids whose spacing or origin sits at
an end of float32, positions one ulp either side of every plane, volumes whose validity or coefficients are zero of either sign,
subnormal, huge, infinite or NaN, normals no unit vector can be made from.  Every row carries a name, so a failure says which edge
broke.  Nothing here is random but the ordinary coefficients, and those come from a seeded generator.

  grids(count)        (name, desc) of every edge grid of a count
  edge_points(d)      (names, (n, 8) points) about the grid d
  edge_normals()      (names, (k, 3) normals)
  edge_volume(count)  (names, (cases, n, 28) volumes)
  edge_cases()        the whole edge set: groups of rows that share a grid and a volume, one look-up each"""
import functools

import numpy as np

import probe_ref as P

U, F = np.uint32, np.float32
TINY, MIN_NORMAL, HUGE = F(1e-45), F(1.17549435e-38), F(3e38)
COUNTS = ((3, 2, 2), (2, 3, 1))
ORIGIN, SPACING = (0.5, -1.0, 2.0), (0.5, 0.25, 1.5)
NORMALS = F([[0.3, -0.5, 0.8], [0, 0, 1], [-2, 0.5, 0.25], [0.6, 0.6, -0.2]])


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def grids(count):
    """an ordinary grid; one axis at a time with a spacing of 1e-45 (the least subnormal), 1.17549435e-38 (the least normal) and 3e38
    - the small ones about an origin of 0 on that axis, or every plane would be the origin -; every origin at +3e38 and at -3e38"""
    out = [("ordinary", P.desc(ORIGIN, SPACING, count))]
    for a in range(3):
        for tag, s in (("1e-45", TINY), ("1.17549435e-38", MIN_NORMAL), ("3e38", HUGE)):
            o, sp = list(ORIGIN), list(SPACING)
            sp[a] = s
            if s < 1:
                o[a] = 0.0
            out.append((f"spacing[{a}] {tag}", P.desc(o, sp, count)))
    out.append(("origin +3e38", P.desc((HUGE,) * 3, SPACING, count)))
    out.append(("origin -3e38", P.desc((-HUGE,) * 3, SPACING, count)))
    return out


def edge_points(d):
    """Rows about the grid d, by name.  `base` is a quarter of a cell inside on every axis; a row moves one axis off it, unless it says
    that the other axes sit on their plane 0 (there their weight f is exactly 0, so that one far corner alone counts)."""
    o, s, cnt = d["origin"], d["spacing"], d["count"]
    names, rows = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        base = (o + F(0.25) * s).astype(F)
        planes = [[F(o[a] + F(i) * s[a]) for i in range(cnt[a])] for a in range(3)]

        def add(name, pos):
            names.append(name)
            rows.append(np.array(pos, F))

        def moved(a, v, frm=base):
            p = frm.copy()
            p[a] = v
            return p
        add("the origin", o)
        add("midway between planes 0 and 1 of axis 0, the other axes on their plane 0", moved(0, F(o[0] + F(0.5) * s[0]), o))
        for a in range(3):
            add(f"axis {a}: the float below the origin", moved(a, down(o[a])))
            if o[a] == 0:
                add(f"axis {a}: -0.0 before an origin of +0.0", moved(a, F(-0.0)))
            for i, v in enumerate(planes[a]):
                add(f"axis {a}: one ulp below plane {i}", moved(a, down(v)))
                add(f"axis {a}: on plane {i}", moved(a, v))
                add(f"axis {a}: one ulp above plane {i}", moved(a, up(v)))
            if s[a] >= F(1e38):
                add(f"axis {a}: a subnormal f (1e-3 behind the origin), the other axes on their plane 0", moved(a, F(o[a] + F(1e-3)), o))
            if abs(o[a]) >= F(1e38):
                add(f"axis {a}: the opposite extreme (pos - origin overflows)", moved(a, -o[a], o))
    pts = np.zeros((len(rows), 8), F)
    pts[:, 0:3] = rows
    pts[:, 3:6] = NORMALS[np.arange(len(rows)) % len(NORMALS)]
    pts.view(U)[:, 6] = np.arange(len(rows), dtype=U) * U(0x01000193)       # (ignored words: anything)
    pts.view(U)[:, 7] = 0xFFFFFFFF
    return names, pts


def edge_normals():
    """normals the contract's normalize3 makes no unit vector from - it gives NaN or zero, not a fault - and lengths at which the
    squared length is subnormal, underflows or overflows, in one and in two components"""
    names = ["all zero", "all -0.0", "a NaN component", "an infinite component"]
    rows = [(0, 0, 0), (-0.0, -0.0, -0.0), (0.5, np.nan, 0.5), (0.5, 0.5, -np.inf)]
    for length in ("1e-42", "1e-30", "1e-20", "1e19", "3e30"):
        v = F(float(length))
        names += [f"length {length}, one component", f"length {length}, two components"]
        rows += [(0, v, 0), (v, 0, -v)]
    return names, np.array(rows, F)


def host_route(pts):
    """the rows the host route admits: finite positions, finite normals that are not all zero"""
    return np.isfinite(pts[:, 0:6]).all(1) & (pts[:, 3:6] != 0).any(1)


def ordinary_volume(count):
    """finite coefficients in [-2, 4) from a seeded generator, every probe valid"""
    n = count[0] * count[1] * count[2]
    vol = np.random.default_rng([17, *count]).uniform(-2.0, 4.0, (n, P.WORDS)).astype(F)
    vol[:, 27] = 1.0
    return vol


def edge_volume(count):
    """One volume a named case: the ordinary volume with probe 0 or probe 1 (its neighbour along x) changed, unless the name says
    otherwise.  +-inf below alternates by word."""
    nx, ny, nz = count
    assert nx >= 2
    n = nx * ny * nz
    pm_inf = np.where(np.arange(27) % 2 == 0, np.inf, -np.inf).astype(F)
    names, vols = [], []

    def case(name, probe=None, validity=None, coef=None):
        v = ordinary_volume(count)
        if probe is not None:
            if coef is not None:
                v[probe, 0:27] = coef
            if validity is not None:
                v[probe, 27] = validity
        names.append(name)
        vols.append(v)
        return v
    names.append("mixed validity: 1, 0.25 and 0 with NaN behind")
    vols.append(P.fabricated_volume(count, 9).reshape(n, P.WORDS))
    p = np.arange(n)
    idx = (p % nx, (p // nx) % ny, p // (nx * ny))
    for a in range(3):
        if count[a] >= 2:
            v = case(f"plane 0 of axis {a} invalid with NaN behind, the rest valid")
            v[idx[a] == 0, 0:27] = np.nan
            v[idx[a] == 0, 27] = 0.0
    case("validity -0.0 (skipped) with NaN behind", 0, F(-0.0), np.nan)
    case("validity subnormal (1e-40)", 0, F(1e-40))
    case("validity 3e38 (the products overflow)", 0, HUGE)
    v = case("validity -1 and +1 on probes 0 and 1, every other probe invalid with +-inf behind")
    v[:, 0:27], v[:, 27] = pm_inf, 0.0
    v[0:2] = ordinary_volume(count)[0:2]
    v[0, 27], v[1, 27] = -1.0, 1.0
    case("validity NaN", 0, np.nan)
    case("validity +inf on probe 1", 1, np.inf)
    case("validity -inf on probe 1", 1, -np.inf)
    case("+-inf coefficients behind a zero validity", 0, 0.0, pm_inf)
    case("coefficients 3e38 behind a valid probe", 0, 1.0, HUGE)
    case("+-inf coefficients behind a valid probe", 0, 1.0, pm_inf)
    return names, np.stack(vols)


CANCEL = "validity -1 and +1"
MIDWAY = "midway between planes 0 and 1 of axis 0"


@functools.lru_cache(maxsize=None)
def edge_cases():
    """The edge set -> a tuple of groups, each a dict: name, d, volume (n, 28), names (one a row), pts (rows, 8).
      A  every grid of grids() under the mixed volume, at edge_points
      B  the grids with a spacing of 3e38 under the volume whose near plane of that axis is invalid: the row with a subnormal f then
         has the far corner alone, wsum == f is subnormal and acc / wsum divides subnormals
      C  the ordinary grid under every other volume of edge_volume, at edge_points
      D  edge_normals at one interior position of the ordinary (3, 2, 2) grid, every probe valid
    Computed once, never written to."""
    groups = []

    def group(name, d, volume, names, pts):
        volume, pts = np.ascontiguousarray(volume, F), np.ascontiguousarray(pts, F)
        volume.setflags(write=False)
        pts.setflags(write=False)
        groups.append(dict(name=name, d=d, volume=volume, names=tuple(names), pts=pts))
    for count in COUNTS:
        vnames, vols = edge_volume(count)
        for gname, d in grids(count):
            names, pts = edge_points(d)
            group(f"{count}, {gname}; {vnames[0]}", d, vols[0], names, pts)
            for a in range(3):
                if d["spacing"][a] >= F(1e38) and count[a] >= 2:
                    k = vnames.index(f"plane 0 of axis {a} invalid with NaN behind, the rest valid")
                    group(f"{count}, {gname}; {vnames[k]}", d, vols[k], names, pts)
        d = P.desc(ORIGIN, SPACING, count)
        names, pts = edge_points(d)
        for k in range(1, len(vnames)):
            group(f"{count}, ordinary; {vnames[k]}", d, vols[k], names, pts)
    count = COUNTS[0]
    d = P.desc(ORIGIN, SPACING, count)
    names, normals = edge_normals()
    pts = np.zeros((len(names), 8), F)
    pts[:, 0:3] = (d["origin"] + F(0.25) * d["spacing"]).astype(F)
    pts[:, 3:6] = normals
    group(f"{count}, ordinary; every probe valid; the normals", d, ordinary_volume(count), names, pts)
    return tuple(groups)


def point_grids():
    """hj_probe_points at value edges: (name, desc)"""
    return [("origin 3e38, spacing 3e38: positions overflow to +inf", P.desc((HUGE,) * 3, (HUGE,) * 3, (3, 2, 2), 0xFFFFFFF0, 7)),
            ("origin -3e38, ordinary spacing", P.desc((-HUGE,) * 3, SPACING, (3, 2, 2), 0xFFFFFFF0, 7)),
            ("origin -3e38, spacing 3e38", P.desc((-HUGE,) * 3, (HUGE,) * 3, (3, 2, 2), 0xFFFFFFF0, 7)),
            ("spacing 1e-45 at count 3", P.desc((0.0, -1.0, 2.0), (TINY, TINY, TINY), (3, 3, 3), 0xFFFFFFF0, 7))]


def assert_bits_or_nan(got, want, what, names=None):
    """Bit for bit, with DESIGN.md's rule for the numeric primitives, "a NaN equals any NaN": where the reference's word is a NaN the
    other's must be a NaN, of any sign and payload; every other word is compared by its bits.  names: one a record, for the message.
    -> the number of records the NaN rule covered."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    width = want.shape[-1]
    g2, w2 = got.reshape(-1, width), want.reshape(-1, width)
    nan = np.isnan(w2)
    diff = np.where(nan, ~np.isnan(g2), g2.view(U) != w2.view(U))
    if diff.any():
        i = int(np.argmax(diff.any(axis=1)))
        label = f" ({names[i]})" if names is not None else ""
        raise AssertionError(f"{what}: {int(diff.sum())} differing words in {int(diff.any(axis=1).sum())} of {len(w2)} records, first at record {i}{label}, "
                             f"words {np.flatnonzero(diff[i]).tolist()} (a NaN equals any NaN):\n  got  {g2[i].tolist()} {[hex(v) for v in g2[i].view(U)]}\n"
                             f"  want {w2[i].tolist()} {[hex(v) for v in w2[i].view(U)]}")
    return int(nan.any(axis=1).sum())


# ------------------------------------------------------------------------------------------------------------------ size edges

WRAP_SEED, WRAP_STRIDE = 0xFFFFFFF0, 0x9E3779B1      # p * stride passes 2^32 at p = 2, and about 2530 times by p = 4095
AXIS_LIMIT = ((1024, 1, 1), (1, 1024, 1), (1, 1, 1024), (1024, 2, 3))
PROBE_LIMIT = ((1024, 1024, 4), (4, 1024, 1024), (1024, 4, 1024))
LONG_AXES = ((1024, 2, 2), (2, 1024, 2), (2, 2, 1024), (1024, 1, 1))
LONG_PLANES = (0, 1, 255, 256, 1022, 1023)
N_LONG = 4161


def plane_points(d):
    """points on, one ulp below and one ulp above the planes LONG_PLANES of the longest axis of d, the other axes a quarter of a cell
    inside -> (names, (18, 8))"""
    o, s, cnt = d["origin"], d["spacing"], d["count"]
    a = int(np.argmax(cnt))
    names, rows = [], []
    for i in LONG_PLANES:
        v = F(o[a] + F(i) * s[a])
        for tag, x in (("one ulp below", down(v)), ("on", v), ("one ulp above", up(v))):
            p = (o + F(0.25) * s).astype(F)
            p[a] = x
            names.append(f"axis {a}: {tag} plane {i}")
            rows.append(p)
    pts = np.zeros((len(rows), 8), F)
    pts[:, 0:3] = rows
    pts[:, 3:6] = NORMALS[np.arange(len(rows)) % len(NORMALS)]
    return names, pts


def cell_points(d):
    """27 points: every combination of the first, a middle and the last cell of the three axes, 0.37 of a cell inside each"""
    o, s = d["origin"].astype(np.float64), d["spacing"].astype(np.float64)
    cells = [(0, max(c - 1, 1) // 2, max(c - 2, 0)) for c in d["count"]]
    pts = np.zeros((27, 8), F)
    for k in range(27):
        pts[k, 0:3] = [o[a] + (cells[a][(k // 3 ** a) % 3] + 0.37) * s[a] for a in range(3)]
    pts[:, 3:6] = NORMALS[np.arange(27) % len(NORMALS)]
    return pts


def limit_points(d, seed):
    """the points of a look-up on a long axis or at the probe limit: probe_ref.sample_points at N_LONG (NaN and infinite positions
    with it: the device route), the plane points, the cell points - 4206 rows"""
    return np.concatenate([P.sample_points(d, N_LONG, seed, nonfinite=True), plane_points(d)[1], cell_points(d)])
