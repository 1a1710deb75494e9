"""The reference of hj_probe_visibility_rays, hj_bake_probe_visibility and hj_sample_probes_visible: include/hijiki_hip.h's text
restated in numpy float32, one rounding per operation, in the stated order.  Where fmaf matters - dot3, normalize3, the RNG - the
value is oracle.num_batch's, as in gather_ref; sqrt, division, min and max are numpy's (IEEE).  The probe positions, the axes and the
accumulation behind the corner weights are probe_ref's text, not restated: sample() with both factors off IS probe_ref.sample.

d is a probe_ref desc (a dict); v is a dict: res, s (rays per texel), max_distance, normal_bias, backface, chebyshev."""
import numpy as np

import gather_ref as G
import probe_ref as P
from hijiki_amd import abi

U, F = np.uint32, np.float32
BACKFACE_FLOOR, CHEBYSHEV_FLOOR = F(0.2), F(0.05)    # Majercik et al. 2019


def vis(res=8, s=4, max_distance=1e18, normal_bias=0.0, backface=True, chebyshev=True):
    return dict(res=int(res), s=int(s), max_distance=F(max_distance), normal_bias=F(normal_bias), backface=bool(backface), chebyshev=bool(chebyshev))


def abi_vis(res=8, rays_per_texel=4, max_distance=10.0, normal_bias=0.0, flags=0):
    """an abi.ProbeVisDesc for the raw entry points"""
    return abi.ProbeVisDesc(res, rays_per_texel, max_distance, normal_bias, flags)


def words(res):
    return 2 * (res + 2) * (res + 2)


def _num(op, w):
    """oracle.num_batch in pieces of at most its cap; no rows: no call"""
    w = np.ascontiguousarray(w, U)
    w = w.reshape(len(w), -1)
    if len(w) == 0:
        return np.zeros((0, abi.NUM_OUT_WORDS), U)
    cap = abi.NUM_MAX_RECORDS
    return np.concatenate([G._num(op, w[a:a + cap]) for a in range(0, len(w), cap)], 0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def normalize3(p):
    return _num("normalize3", _bits(p).reshape(-1, 3))[:, 0:3].copy().view(F)


def dot3(p, q):
    return _num("dot3", np.concatenate([_bits(p).reshape(-1, 3), _bits(q).reshape(-1, 3)], 1))[:, 0].copy().view(F)


def len3(p):
    with np.errstate(invalid="ignore"):
        return np.sqrt(dot3(p, p)).astype(F)


def sg(x):
    with np.errstate(invalid="ignore"):
        return np.where(x >= F(0), F(1), F(-1)).astype(F)


def decode(ex, ey):
    """a point of the octahedral square -> its direction before normalize (n, 3)"""
    ex, ey = np.asarray(ex, F), np.asarray(ey, F)
    az = ((F(1) - np.abs(ex)) - np.abs(ey)).astype(F)
    up = az >= 0
    x = np.where(up, ex, (F(1) - np.abs(ey)) * sg(ex)).astype(F)
    y = np.where(up, ey, (F(1) - np.abs(ex)) * sg(ey)).astype(F)
    return np.stack([x, y, az], 1).astype(F)


def encode(e):
    """directions of any length (n, 3) -> (px, py) in the octahedral square"""
    e = np.asarray(e, F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l1 = ((np.abs(e[:, 0]) + np.abs(e[:, 1])) + np.abs(e[:, 2])).astype(F)
        px, py = (e[:, 0] / l1).astype(F), (e[:, 1] / l1).astype(F)
        low = e[:, 2] < 0
        fx = ((F(1) - np.abs(py)) * sg(px)).astype(F)
        fy = ((F(1) - np.abs(px)) * sg(py)).astype(F)
    return np.where(low, fx, px).astype(F), np.where(low, fy, py).astype(F)


def texel_coordinate(p, res):
    """an octahedral coordinate in [-1, 1] -> the atlas coordinate the look-up clamps: interior texel t's centre is at t + 1"""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((p * F(0.5) + F(0.5)) * F(res) + F(0.5)).astype(F)


def draws(d, v, first, num):
    """-> (p, tx, ty (int64), u, w (float32)) of the rays of probes first ... first + num - 1, probe-major, ascending r"""
    res, s = v["res"], v["s"]
    per = res * res * s
    i = np.arange(num * per, dtype=np.int64)
    p, r = first + i // per, i % per
    t = r // s
    seeds = ((d["seed"] + p * d["seed_stride"] + r) & 0xFFFFFFFF).astype(U)
    state = _num("rng_seed", seeds.reshape(-1, 1))[:, 0]
    a = _num("rng_float", state.reshape(-1, 1))
    b = _num("rng_float", a[:, 1].reshape(-1, 1))
    return p, t % res, t // res, a[:, 0].copy().view(F), b[:, 0].copy().view(F)


def square(tx, ty, u, w, res):
    """the draws -> (ex, ey), the point of the octahedral square"""
    scale = F(2) / F(res)
    return ((tx.astype(F) + u) * scale - F(1)).astype(F), ((ty.astype(F) + w) * scale - F(1)).astype(F)


def positions(d, p):
    """probe indices -> (len(p), 3) positions: probe_ref.points' expression"""
    nx, ny, _ = d["count"]
    idx = (p % nx, (p // nx) % ny, p // (nx * ny))
    out = np.zeros((len(p), 3), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            out[:, a] = d["origin"][a] + idx[a].astype(F) * d["spacing"][a]
    return out


def rays(d, v, first=0, num=None):
    """-> (num * res * res * s, 8) float32: hj_probe_visibility_rays"""
    nx, ny, nz = d["count"]
    num = nx * ny * nz - first if num is None else num
    p, tx, ty, u, w = draws(d, v, first, num)
    ex, ey = square(tx, ty, u, w, v["res"])
    out = np.zeros((len(p), 8), F)
    out[:, 0:3] = positions(d, p)
    out[:, 3:6] = normalize3(decode(ex, ey))
    out[:, 7] = v["max_distance"]
    return out


def border_source(res):
    """-> (T * T,) int64: the interior texel ty * res + tx each atlas texel by * T + bx takes its rays from"""
    T = res + 2
    bx, by = np.meshgrid(np.arange(T), np.arange(T))           # [by, bx]
    tx, ty = bx - 1, by - 1
    row, col = (by == 0) | (by == T - 1), (bx == 0) | (bx == T - 1)
    tx = np.where(row & ~col, res - bx, tx)                     # border (i + 1, .) copies interior res - 1 - i
    ty = np.where(row & ~col, np.where(by == 0, 0, res - 1), ty)
    ty = np.where(col & ~row, res - by, ty)
    tx = np.where(col & ~row, np.where(bx == 0, 0, res - 1), tx)
    tx = np.where(row & col, np.where(bx == 0, res - 1, 0), tx)  # corners: diagonally opposite
    ty = np.where(row & col, np.where(by == 0, res - 1, 0), ty)
    return (ty * res + tx).reshape(-1).astype(np.int64)


def reduce(hits, v):
    """hits: (ids (m,) int32, t (m,) float32) of whole probes' rays in rays()' order -> (probes, T, T, 2) float32"""
    ids, t = hits
    res, s = v["res"], v["s"]
    ids, t = np.asarray(ids).reshape(-1, res * res, s), np.asarray(t, F).reshape(-1, res * res, s)
    md = v["max_distance"]
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.where(ids >= 0, np.fmin(t, md), md).astype(F)
        a1, a2 = np.zeros(dist.shape[0:2], F), np.zeros(dist.shape[0:2], F)
        for k in range(s):
            a1 = (a1 + dist[:, :, k]).astype(F)
            a2 = (a2 + dist[:, :, k] * dist[:, :, k]).astype(F)
        m = np.stack([a1 / F(s), a2 / F(s)], 2).astype(F)
    T = res + 2
    return m[:, border_source(res), :].reshape(-1, T, T, 2)


def bake(trace, d, v, first=0, num=None):
    """rays -> trace -> reduce.  trace: a Renderer (its trace_rays) or a function of (n, 8) rays -> (ids, t, ...)"""
    fn = trace.trace_rays if hasattr(trace, "trace_rays") else trace
    out = fn(rays(d, v, first, num))
    return reduce((out[0], out[1]), v)


def fetch(atlas_p, cx, cy, res):
    """atlas_p (n, T, T, 2): each row's probe's map; cx, cy atlas coordinates -> (m1, m2) by the look-up's bilinear fetch"""
    T = res + 2
    x0, x1, gx, fx = P.axis(cx, 0.0, 1.0, T)
    y0, y1, gy, fy = P.axis(cy, 0.0, 1.0, T)
    k = np.arange(len(cx))
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(2):
            t00, t10, t01, t11 = atlas_p[k, y0, x0, m], atlas_p[k, y0, x1, m], atlas_p[k, y1, x0, m], atlas_p[k, y1, x1, m]
            out.append(((t00 * gx + t10 * fx) * gy + (t01 * gx + t11 * fx) * fy).astype(F))
    return out


def corner_factors(d, v, atlas, pts):
    """-> (wb (n, 8), wv (n, 8)) float32 in probe_ref's corner order dz, dy, dx"""
    nx, ny, nz = d["count"]
    res = v["res"]
    pts = np.ascontiguousarray(pts, F).reshape(-1, 8)
    n = len(pts)
    x = pts[:, 0:3]
    nn = normalize3(pts[:, 3:6])
    with np.errstate(invalid="ignore", over="ignore"):
        xb = (x + nn * v["normal_bias"]).astype(F)
    ax = [P.axis(pts[:, a], d["origin"][a], d["spacing"][a], d["count"][a]) for a in range(3)]
    maps = None if atlas is None else np.ascontiguousarray(atlas, F).reshape(nx * ny * nz, res + 2, res + 2, 2)
    wb, wv = np.ones((n, 8), F), np.ones((n, 8), F)
    c = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    ix, iy, iz = ax[0][dx], ax[1][dy], ax[2][dz]
                    q = (iz * ny + iy) * nx + ix
                    Pp = positions(d, q)
                    if v["backface"]:
                        t = normalize3((Pp - x).astype(F))
                        h = ((dot3(t, nn) + F(1)) * F(0.5)).astype(F)
                        wb[:, c] = np.where((Pp == x).all(1), F(1), h * h + BACKFACE_FLOOR)
                    if v["chebyshev"]:
                        e = (xb - Pp).astype(F)
                        rr = len3(e)
                        px, py = encode(e)
                        m1, m2 = fetch(maps[q], texel_coordinate(px, res), texel_coordinate(py, res), res)
                        var = np.abs(m1 * m1 - m2).astype(F)
                        dl = (rr - m1).astype(F)
                        k = (var / (var + dl * dl)).astype(F)
                        cheb = np.fmax((k * k) * k, CHEBYSHEV_FLOOR).astype(F)
                        wv[:, c] = np.where((e == 0).all(1), F(1), np.where(rr > m1, cheb, F(1)))
                    c += 1
    return wb, wv


def sample(d, v, volume, atlas, pts, detail=False):
    """-> (n, 4) float32 as hj_sample_probes_visible defines it [, wb (n, 8), wv (n, 8): the corners' factors, dz, dy, dx]"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 8)
    wb, wv = corner_factors(d, v, atlas, pts)
    out = sample_weighted(d, volume, pts, wb, wv)
    return (out, wb, wv) if detail else out


def sample_weighted(d, volume, pts, wb, wv):
    """probe_ref.sample's accumulation with w = ((((wx * wy) * wz) * validity) * wb) * wv: its corner order, its skip, its sums, its
    basis and its zero rule, restated only where the weight enters (probe_ref.sample offers no hook for a further factor); with wb
    = wv = 1 the result is probe_ref.sample's bit for bit, which test_probe_vis_host.py asserts."""
    nx, ny, nz = d["count"]
    vol = np.ascontiguousarray(volume, F).reshape(nx * ny * nz, P.WORDS)
    n = len(pts)
    ax = [P.axis(pts[:, a], d["origin"][a], d["spacing"][a], d["count"][a]) for a in range(3)]
    acc, wsum = np.zeros((n, 27), F), np.zeros(n, F)
    c = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    q = (ax[2][dz] * ny + ax[1][dy]) * nx + ax[0][dx]
                    rec = vol[q]
                    w = (((((ax[0][2 + dx] * ax[1][2 + dy]) * ax[2][2 + dz]) * rec[:, 27]) * wb[:, c]) * wv[:, c]).astype(F)
                    on = w != 0
                    acc = np.where(on[:, None], acc + rec[:, 0:27] * w[:, None], acc).astype(F)
                    wsum = np.where(on, wsum + w, wsum).astype(F)
                    c += 1
        nn = normalize3(pts[:, 3:6])
        Y = G.sh9(nn)
        out = np.zeros((n, 4), F)
        zero = wsum == 0
        safe = np.where(zero, F(1), wsum)
        cf = (acc / safe[:, None]).astype(F)
        for ch in range(3):
            e = np.zeros(n, F)
            for j in range(9):
                e = e + cf[:, 3 * j + ch] * Y[:, j]
            out[:, ch] = e
        out[:, 3] = wsum
    out[zero] = 0
    return out


# ------------------------------------------------------------------------------------------------------------------ shared cases

def hashed_atlas(n, res, seed=0):
    """a fabricated atlas (n, T, T, 2): moments from an integer hash of (probe, texel, moment) - m1 in [0, 4), m2 in [0, 16) with no
    relation to m1^2 (so m2 < m1^2 occurs about as often as not) -, and by the hash's low bits a zero m1, a zero m2, an infinite m1 and
    a NaN m2 now and then (a few per cent each)."""
    T = res + 2
    i = np.arange(n * T * T * 2, dtype=np.int64) + 7919 * int(seed)
    h = P._mix(i & P.M32)
    val = ((h >> 8).astype(F) * F(2.0 ** -24)).astype(F)         # [0, 1)
    out = (val.reshape(n, T, T, 2) * np.array([4, 16], F)).astype(F)
    kind = (P._mix((i * 3 + 1) & P.M32) % 64).reshape(n, T, T, 2)
    out[..., 0][kind[..., 0] == 0] = 0.0
    out[..., 1][kind[..., 1] == 1] = 0.0
    out[..., 0][kind[..., 0] == 2] = np.inf
    out[..., 1][kind[..., 1] == 3] = np.nan
    return out
