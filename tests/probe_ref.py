"""The reference of hj_probe_points, hj_bake_probes and hj_sample_probes: include/hijiki_hip.h's text restated in numpy float32, one
rounding per operation, in the stated order.  The normal of a sample point is normalised by oracle.num_batch("normalize3"), the SH
basis is gather_ref.sh9, and bake() is gather_ref.gather followed by resolve() - nothing of the gather is restated.

A desc is a dict: origin (3,), spacing (3,), count (nx, ny, nz), and for points() / bake() seed, seed_stride, min_distance."""
import functools

import numpy as np

import gather_ref as G
import path_query_ref as R

U, F = np.uint32, np.float32
WORDS = 28
SPHERE_WEIGHT = F(12.5663706)                        # 4 pi
A_BAND = (F(3.14159274), F(2.09439516), F(0.785398185))   # pi, 2 pi / 3, pi / 4
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)                    # of Y_j


def desc(origin, spacing, count, seed=0, seed_stride=1, min_distance=0.0):
    return dict(origin=np.asarray(origin, F), spacing=np.asarray(spacing, F), count=tuple(int(c) for c in count), seed=int(seed),
                seed_stride=int(seed_stride), min_distance=F(min_distance))


def abi_desc(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2), seed=0, seed_stride=1, min_distance=0.0, flags=0):
    """an abi.ProbeDesc for the raw entry points"""
    import ctypes as C
    from hijiki_amd import abi
    f3, u3 = C.c_float * 3, C.c_uint32 * 3
    return abi.ProbeDesc(f3(*origin), f3(*spacing), u3(*count), seed, seed_stride, min_distance, flags)


def points(d):
    """-> (n, 8) float32: the gather points of the grid in ascending p = (z * ny + y) * nx + x"""
    nx, ny, nz = d["count"]
    p = np.arange(nx * ny * nz, dtype=np.int64)
    idx = (p % nx, (p // nx) % ny, p // (nx * ny))
    out = np.zeros((len(p), 8), F)
    with np.errstate(over="ignore", invalid="ignore"):   # (a grid whose positions overflow: +-inf, as float32 gives them)
        for a in range(3):
            out[:, a] = d["origin"][a] + idx[a].astype(F) * d["spacing"][a]
    out.view(U)[:, 6] = ((d["seed"] + p * d["seed_stride"]) & 0xFFFFFFFF).astype(U)
    out.view(U)[:, 7] = p.astype(U)
    return out


def resolve(records36, spp, min_distance):
    """(n, 36) gather records (sphere, SH9) -> (n, 28): word 3 j + c = (sum[8 + 3 j + c] * s) * A_band(j), word 27 the validity"""
    rec = np.ascontiguousarray(records36, F).reshape(-1, 36)
    s = SPHERE_WEIGHT / F(spp)
    out = np.zeros((len(rec), WORDS), F)
    for j in range(9):
        out[:, 3 * j:3 * j + 3] = (rec[:, 8 + 3 * j:11 + 3 * j] * s) * A_BAND[BAND[j]]
    with np.errstate(invalid="ignore"):
        out[:, 27] = np.where(rec[:, 5] >= F(min_distance), F(1), F(0))
    return out


def axis(pos, origin, spacing, count):
    """one axis of the look-up -> (i0, i1 as int64, the weights of i0 and of i1 as float32)"""
    m = count - 1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = (pos - F(origin)) / F(spacing)
        g = np.where(g >= F(0), g, F(0)).astype(F)     # (a NaN becomes 0)
        g = np.where(g <= F(m), g, F(m)).astype(F)
    i0 = np.minimum(g.astype(U).astype(np.int64), m - 1 if m > 0 else 0)
    f = (g - i0.astype(F)).astype(F)
    i1 = np.minimum(i0 + 1, m)
    return i0, i1, (F(1) - f).astype(F), f


def sample(d, volume, pts, detail=False):
    """volume (nz, ny, nx, 28) or (n, 28), pts (n, 8) -> (n, 4) float32 as hj_sample_probes defines it.  volume may also be a
    callable that maps probe indices q (an int64 array) to their records (len(q), 28): a volume that does not exist on the host.
    detail: -> (out, w (n, 8): the corners' weights in the order dz, dy, dx, the wsum before the zero rule, q (n, 8) int64)"""
    nx, ny, nz = d["count"]
    if callable(volume):
        fetch = lambda q: np.ascontiguousarray(volume(q), F).reshape(len(q), WORDS)      # noqa: E731
    else:
        vol = np.ascontiguousarray(volume, F).reshape(nx * ny * nz, WORDS)
        fetch = lambda q: vol[q]                                                         # noqa: E731
    pts = np.ascontiguousarray(pts, F).reshape(-1, 8)
    n = len(pts)
    ax = [axis(pts[:, a], d["origin"][a], d["spacing"][a], d["count"][a]) for a in range(3)]
    acc, wsum = np.zeros((n, 27), F), np.zeros(n, F)
    ws, qs = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    q = (ax[2][dz] * ny + ax[1][dy]) * nx + ax[0][dx]
                    rec = fetch(q)
                    w = ((ax[0][2 + dx] * ax[1][2 + dy]) * ax[2][2 + dz]) * rec[:, 27]
                    ws.append(w)
                    qs.append(q)
                    on = w != 0                       # (a NaN weight counts: it is not zero)
                    acc = np.where(on[:, None], acc + rec[:, 0:27] * w[:, None], acc).astype(F)
                    wsum = np.where(on, wsum + w, wsum).astype(F)
        nn = G._vec("normalize3", np.ascontiguousarray(pts[:, 3:6])) if n else np.zeros((0, 3), F)
        Y = G.sh9(nn)
        out = np.zeros((n, 4), F)
        zero = wsum == 0
        safe = np.where(zero, F(1), wsum)
        c = (acc / safe[:, None]).astype(F)
        for ch in range(3):
            e = np.zeros(n, F)
            for j in range(9):
                e = e + c[:, 3 * j + ch] * Y[:, j]
            out[:, ch] = e
        out[:, 3] = wsum
    out[zero] = 0
    if detail:
        return out, np.stack(ws, 1).astype(F).reshape(n, 8), wsum, np.stack(qs, 1).reshape(n, 8)
    return out


def bake(cs, d, spp, opts=None):
    """-> (volume (n, 28), the gather's 36-word records, the gather's counts)"""
    rec, counts = G.gather(cs, points(d), spp, sphere=True, sh=True, opts=opts)
    return resolve(rec, spp, d["min_distance"]), rec, counts


# ------------------------------------------------------------------------------------------------------------------ shared cases

def grid_in_domain(cs, count, seed=0xFFFFFFF0, seed_stride=7, min_distance=0.0):
    """a grid of `count` probes spread over the middle 80 % of path_query_ref.domain(cs)"""
    lo, hi = R.domain(cs)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    a, b = lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)
    spacing = [(b[k] - a[k]) / max(count[k] - 1, 1) for k in range(3)]
    d = desc(a, spacing, count, seed, seed_stride, min_distance)
    p = points(d)[:, 0:3]
    assert ((p >= R.domain(cs)[0]) & (p <= R.domain(cs)[1])).all()
    return d


BAKE_COUNT, BAKE_SPP = (3, 2, 2), 4


@functools.lru_cache(maxsize=None)
def expected_bake(name):
    """bake() of scene `name` on BAKE_COUNT at BAKE_SPP, max_bounces = 40: computed once, never written to"""
    cs = R.scene(name)
    d = grid_in_domain(cs, BAKE_COUNT)
    vol, rec, counts = bake(cs, d, BAKE_SPP, R.options(40))
    vol.setflags(write=False)
    rec.setflags(write=False)
    return d, vol, rec, counts


def fabricated_volume(count, seed):
    """a volume from a seeded generator: finite coefficients in [-2, 4); validity 1, 0 and 0.25 at random, with probe 0 valid at
    every count, probe 1 at 0.25 where there is one, the last probe invalid where there are three or more, and - where every axis has at
    least three planes, so that other cells remain: (5, 4, 3) here - one whole cell invalid; NaN coefficients behind every zero
    validity.  So every count has corners that count, fully and fractionally, and none is all invalid."""
    nx, ny, nz = count
    n = nx * ny * nz
    rng = np.random.default_rng([seed, nx, ny, nz])
    vol = rng.uniform(-2.0, 4.0, (nz, ny, nx, WORDS)).astype(F)
    kind = rng.choice(3, (nz, ny, nx), p=[0.6, 0.2, 0.2])
    valid = np.choose(kind, [F(1), F(0), F(0.25)]).astype(F)
    flat = valid.reshape(-1)
    if n >= 3:
        flat[-1] = 0.0
    flat[0] = 1.0
    if n >= 2:
        flat[1] = 0.25
    if min(count) >= 3:
        valid[0:2, 0:2, 0:2] = 0.0                   # a whole cell of a grid that has others
    vol[..., 27] = valid
    vol[valid == 0, 0:27] = np.nan
    return vol


def sample_points(d, n, seed, nonfinite=False):
    """n >= 1 points about the grid of d: in cyclic order interior points, points exactly on a probe plane of every axis, points on
    the last planes, points outside beyond each face, the domain's corners; normals unit, of lengths in [0.5, 2], and the six axes.
    nonfinite: also NaN and +-inf positions (device route only)."""
    rng = np.random.default_rng([seed, n])
    cnt = np.array(d["count"], np.int64)
    o, s = d["origin"].astype(np.float64), d["spacing"].astype(np.float64)
    hi = o + (cnt - 1) * s
    span = np.maximum(hi - o, s)
    pts = np.zeros((n, 8), F)
    pos = rng.uniform(o, o + span, (n, 3))
    kind = np.arange(n) % (16 if nonfinite else 13)
    k = np.arange(n)
    plane = o + rng.integers(0, cnt, (n, 3)) * s
    for a in range(3):
        on = kind == 1 + a                           # exactly on a probe plane of axis a (float32 of the product form)
        pos[on, a] = (d["origin"][a] + rng.integers(0, cnt[a], n).astype(F) * d["spacing"][a])[on]
        last = kind == 4                             # the last plane of every axis
        pos[last, a] = F(d["origin"][a] + F(cnt[a] - 1) * d["spacing"][a])
        below, above = kind == 5 + 2 * a, kind == 6 + 2 * a
        pos[below, a] = o[a] - rng.uniform(0.01, 3.0, n)[below] * span[a]
        pos[above, a] = hi[a] + rng.uniform(0.01, 3.0, n)[above] * span[a]
    on_all = kind == 11                              # on a probe: planes of all three axes
    pos[on_all] = plane[on_all]
    corner = kind == 12
    pos[corner] = np.where(((k[:, None] // 13) >> np.arange(3)) & 1, hi, o)[corner]
    pts[:, 0:3] = pos
    if nonfinite:
        pts[kind == 13, (k[kind == 13] // 16) % 3] = np.nan
        pts[kind == 14, (k[kind == 14] // 16) % 3] = np.inf
        pts[kind == 15, (k[kind == 15] // 16) % 3] = -np.inf
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    scaled = (k // 3) % 3 == 1
    v[scaled] *= rng.uniform(0.5, 2.0, (n, 1))[scaled]
    axes = (k // 3) % 3 == 2
    v[axes] = G.AXES[k[axes] % 6]
    pts[:, 3:6] = v
    pts.view(U)[:, 6:8] = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(U)      # (ignored words: anything)
    return pts


# --------------------------------------------------------------------------------------------- a volume that is a function of (p, k)

M32 = 0xFFFFFFFF
HASH_VALID = (1.0, 1.0, 0.0, 0.25)                   # the validity of a probe by the low two bits of its word 27's hash


def _mix(x):
    """An integer hash of uint32 values in uint32 arithmetic, written for int64 carriers (numpy arrays and torch tensors alike): both
    multipliers are below 2^31, so no product reaches 2^63, and every step is masked back to 32 bits."""
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & M32
    x = ((x ^ (x >> 15)) * 0x2C1B3C6D) & M32
    return x ^ (x >> 16)


def hashed_records(q):
    """probe indices q (int64) -> (len(q), 28) float32, the records of hashed_volume: word k of probe p from h = _mix(p * 28 + k).
    Coefficients (float)(h >> 8) * 2^-23 - 1 in [-1, 1) - 24 bits, a power of two, a difference of multiples of 2^-23 below 2: every
    step exact in float32.  Validity HASH_VALID[h(p, 27) & 3]; behind a zero validity word k is NaN, +inf, -inf by k % 3."""
    q = np.asarray(q, np.int64).reshape(-1)
    h = _mix(q[:, None] * WORDS + np.arange(WORDS, dtype=np.int64)[None, :])
    out = ((h >> 8).astype(F) * F(2.0 ** -23) - F(1)).astype(F)
    valid = np.array(HASH_VALID, F)[h[:, 27] & 3]
    bad = np.array([np.nan, np.inf, -np.inf], F)[np.arange(27) % 3]
    out[:, 0:27] = np.where((valid == 0)[:, None], bad[None, :], out[:, 0:27])
    out[:, 27] = valid
    return out


def hashed_volume(count, device="cpu", slab=1 << 16):
    """the whole volume of hashed_records as a torch tensor (nz, ny, nx, 28) on `device`, built `slab` probes at a time (the int64
    temporaries of a slab: 28 * 8 * slab bytes each)"""
    import torch
    nx, ny, nz = count
    n = nx * ny * nz
    dev = torch.device(device)
    vol = torch.empty((n, WORDS), dtype=torch.float32, device=dev)
    k = torch.arange(WORDS, dtype=torch.int64, device=dev)[None, :]
    table = torch.tensor(HASH_VALID, dtype=torch.float32, device=dev)
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=torch.float32, device=dev)[torch.arange(27, device=dev) % 3]
    for a in range(0, n, slab):
        p = torch.arange(a, min(a + slab, n), dtype=torch.int64, device=dev)
        h = _mix(p[:, None] * WORDS + k)
        out = (h >> 8).to(torch.float32) * (2.0 ** -23) - 1.0
        valid = table[h[:, 27] & 3]
        out[:, 0:27] = torch.where((valid == 0)[:, None], bad[None, :], out[:, 0:27])
        out[:, 27] = valid
        vol[a:a + len(p)] = out
    return vol.reshape(nz, ny, nx, WORDS)
