"""The reference of hj_place_probes and of the placed consumers: include/hijiki_hip.h's text ("Probe placement") restated in numpy
float32, one rounding per operation, in the stated order, over GIVEN rays, hits and surface records - nothing of a trace is restated
here.  The rays' draws, the probe positions and the weighted look-up are probe_vis_ref's (rays, positions, sample_weighted), the
blend is probe_update_ref's; dot and length are probe_vis_ref.dot3 and len3 (oracle.num_batch's fmaf).  Every comparison is written
the way the header writes it, so that a NaN falls where the header says it falls.

d is a probe_ref desc, v a probe_vis_ref vis, pl a dict (place()), placement an (n, 4) float32 array: the offset, the state's bits."""
import numpy as np

import probe_ref as P
import probe_update_ref as PU
import probe_vis_ref as V
from hijiki_amd import abi

U, F = np.uint32, np.float32
WORDS = 4
NO_RELOCATE, NO_CLASSIFY = 1, 2
BRANCHES = ("inside", "near_moved", "near_kept", "back_moved", "back_at_grid", "none", "rejected")


def place(first, num, min_front_distance, backface_share=0.25, max_offset=0.45, flags=0):
    return dict(first=int(first), num=int(num), min_front=F(min_front_distance), share=F(backface_share), max_offset=F(max_offset), flags=int(flags))


def abi_place(first_probe=0, num_probes=8, frame=0, frame_stride=1, min_front_distance=0.5, backface_share=0.25, max_offset=0.45, flags=0):
    """an abi.ProbePlace for the raw entry points"""
    return abi.ProbePlace(first_probe, num_probes, frame, frame_stride, min_front_distance, backface_share, max_offset, flags)


def zeros(n):
    return np.zeros((n, WORDS), F)


def state(placement):
    """-> the states as uint32 (n,)"""
    return np.ascontiguousarray(placement, F).reshape(-1, WORDS).view(U)[:, 3].copy()


def with_state(placement, st):
    out = np.ascontiguousarray(placement, F).reshape(-1, WORDS).copy()
    out.view(U)[:, 3] = np.asarray(st, U)
    return out


def placed_positions(d, placement, p):
    """probe indices -> (len(p), 3): the grid's product and sum (probe_vis_ref.positions), then one more sum"""
    pl = np.ascontiguousarray(placement, F).reshape(-1, WORDS)
    with np.errstate(invalid="ignore", over="ignore"):
        return (V.positions(d, p) + pl[p, 0:3]).astype(F)


def rays(d, v, placement, first=0, num=None, probes=None):
    """-> (len * R, 8): probe_vis_ref.rays of the probes first ... first + num - 1 (or of the listed `probes`, in that order) with the
    origin at the placed position"""
    per = v["res"] * v["res"] * v["s"]
    if probes is None:
        nx, ny, nz = d["count"]
        num = nx * ny * nz - first if num is None else num
        probes = np.arange(first, first + num, dtype=np.int64)
    probes = np.asarray(probes, np.int64)
    if len(probes) == 0:
        return np.zeros((0, 8), F)
    runs = np.split(probes, np.flatnonzero(np.diff(probes) != 1) + 1)         # (probe_vis_ref.rays takes a contiguous range)
    out = np.concatenate([V.rays(d, v, int(r[0]), len(r)) for r in runs], 0)
    out[:, 0:3] = np.repeat(placed_positions(d, placement, probes), per, 0)
    return out


def _least(dist, mask):
    """per row the least dist over mask and its column, ties to the lowest column -> (value, column, any)"""
    key = np.where(mask, dist, np.inf)
    col = np.argmin(key, 1)                                                 # (the first of equal values)
    return key[np.arange(len(key)), col].astype(F), col, mask.any(1)


def step(d, v, pl, placement, ray, ids, t, normal, detail=False):
    """One hj_place_probes step.  placement: the whole volume's (n, 4); ray: (num * R, 8), ids (num * R,) int32, t (num * R,) float32,
    normal (num * R, 3) (surface words 3-5) of the window's probes in rays()' order -> the new placement (n, 4); detail: -> (new,
    {branch: a mask over the window's probes}, inside, the new states)"""
    res, s = v["res"], v["s"]
    R = res * res * s
    a, num = pl["first"], pl["num"]
    out = np.ascontiguousarray(placement, F).reshape(-1, WORDS).copy()
    assert 0 <= a and a + num <= len(out) and len(ray) == num * R
    O = out[a:a + num, 0:3].copy()
    dirs = np.ascontiguousarray(ray, F)[:, 3:6].reshape(num, R, 3)
    ids = np.asarray(ids).reshape(num, R)
    t = np.asarray(t, F).reshape(num, R)
    md, mfd, spacing = v["max_distance"], pl["min_front"], np.asarray(d["spacing"], F)
    k = np.arange(num)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        hit = ids >= 0
        dist = np.where(hit, np.fmin(t, md), md).astype(F)
        dn = V.dot3(dirs.reshape(-1, 3), np.ascontiguousarray(normal, F).reshape(-1, 3)).reshape(num, R)
        back = hit & (dn > F(0))
        nb = back.sum(1)
        cb, rb, _ = _least(dist, back)
        cf, rf, front = _least(dist, ~back)
        far = np.where(~back, dist, -np.inf)
        rq = np.argmax(far, 1)
        ff = far[k, rq].astype(F)
        inside = nb.astype(F) > (pl["share"] * F(R)).astype(F)
        # relocation
        cand = O.copy()
        step_in = (cb + (mfd * F(0.5)).astype(F)).astype(F)
        c_in = (O + (dirs[k, rb] * step_in[:, None]).astype(F)).astype(F)
        near = ~inside & front & (cf < mfd)
        turn = V.dot3(dirs[k, rf], dirs[k, rq]) <= F(0.5)
        c_near = (O + (dirs[k, rq] * np.fmin(ff, mfd).astype(F)[:, None]).astype(F)).astype(F)
        room = ~inside & front & ~(cf < mfd) & (cf > mfd)
        L = V.len3(O)
        away = L > F(0)
        backstep = np.fmin((cf - mfd).astype(F), L).astype(F)
        c_back = (O - ((O / L[:, None]).astype(F) * backstep[:, None]).astype(F)).astype(F)
        cand = np.where(inside[:, None], c_in, cand)
        cand = np.where((near & turn)[:, None], c_near, cand)
        cand = np.where((room & away)[:, None], c_back, cand)
        ok = (np.abs(cand) <= (pl["max_offset"] * spacing).astype(F)[None, :]).all(1)
        # classification: from the old O
        reach = (O[:, None, :] + (dirs * t[:, :, None]).astype(F)).astype(F)
        seen = (hit & ~back & (np.abs(reach) <= spacing[None, None, :]).all(2)).any(1)
    new_state = np.where(~inside & seen, 0, 1).astype(U)
    if not pl["flags"] & NO_RELOCATE:
        out[a:a + num, 0:3] = np.where(ok[:, None], cand, O)
    if not pl["flags"] & NO_CLASSIFY:
        out.view(U)[a:a + num, 3] = new_state
    if not detail:
        return out
    moved = dict(inside=inside, near_moved=near & turn, near_kept=near & ~turn, back_moved=room & away, back_at_grid=room & ~away,
                 none=~inside & ~near & ~room)
    moved["rejected"] = ~ok
    return out, moved, inside, new_state


def trace_step(trace, d, v, pl, placement, seed=None, detail=False):
    """rays -> trace -> step.  trace: a function of (m, 8) rays -> (ids, t, normal (m, 3)); seed: the frame's seed' in place of d's"""
    dd = d if seed is None else dict(d, seed=int(seed))
    ray = rays(dd, v, placement, pl["first"], pl["num"])
    ids, t, normal = trace(ray)
    return step(dd, v, pl, placement, ray, ids, t, normal, detail=detail)


def active(placement, first, num):
    """-> the window's active probes, ascending (int64)"""
    return first + np.flatnonzero(state(placement)[first:first + num] == 0).astype(np.int64)


def points(d, placement, probes):
    """-> (len(probes), 8): probe_ref.points' records of the listed probes with the placed position in words 0-2"""
    probes = np.asarray(probes, np.int64)
    out = np.zeros((len(probes), 8), F)
    out[:, 0:3] = placed_positions(d, placement, probes)
    out.view(U)[:, 6] = ((d["seed"] + probes * d["seed_stride"]) & 0xFFFFFFFF).astype(U)
    out.view(U)[:, 7] = probes.astype(U)
    return out


def blend_probes(old, fresh_active, placement, upd):
    """old: the whole volume (n, 28); fresh_active: the fresh records of active(placement, window), in its order -> the volume after
    hj_update_probes_placed: probe_update_ref.blend_probes on the active probes one by one, every other record old's bits"""
    out = np.ascontiguousarray(old, F).reshape(-1, P.WORDS).copy()
    act = active(placement, upd["first"], upd["num"])
    fresh = out.copy()
    fresh[act] = np.ascontiguousarray(fresh_active, F).reshape(-1, P.WORDS)
    full = PU.blend_probes(out, fresh, upd)
    out[act] = full.reshape(-1, P.WORDS)[act]
    return out.reshape(np.shape(old))


def blend_atlas(old, fresh_active, res, placement, upd):
    """old: the whole atlas (n, T, T, 2); fresh_active: (len(active), T, T, 2) -> the atlas after hj_update_probe_visibility_placed"""
    T = res + 2
    out = np.ascontiguousarray(old, F).reshape(-1, T, T, 2).copy()
    act = active(placement, upd["first"], upd["num"])
    fresh = out.copy()
    fresh[act] = np.ascontiguousarray(fresh_active, F).reshape(-1, T, T, 2)
    full = PU.blend_atlas(out, fresh, res, upd).reshape(-1, T, T, 2)
    out[act] = full[act]
    return out.reshape(np.shape(old))


def corner_factors(d, v, atlas, pts, placement):
    """probe_vis_ref.corner_factors with P the placed position -> (wb, wv, off (n, 8) bool: the corner's probe is inactive)"""
    nx, ny, nz = d["count"]
    res = v["res"]
    pts = np.ascontiguousarray(pts, F).reshape(-1, 8)
    n = len(pts)
    x = pts[:, 0:3]
    nn = V.normalize3(pts[:, 3:6])
    st = state(placement)
    with np.errstate(invalid="ignore", over="ignore"):
        xb = (x + nn * v["normal_bias"]).astype(F)
    ax = [P.axis(pts[:, a], d["origin"][a], d["spacing"][a], d["count"][a]) for a in range(3)]
    maps = None if atlas is None else np.ascontiguousarray(atlas, F).reshape(nx * ny * nz, res + 2, res + 2, 2)
    wb, wv, off = np.ones((n, 8), F), np.ones((n, 8), F), np.zeros((n, 8), bool)
    c = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    q = (ax[2][dz] * ny + ax[1][dy]) * nx + ax[0][dx]
                    Pp = placed_positions(d, placement, q)
                    off[:, c] = st[q] != 0
                    if v["backface"]:
                        tt = V.normalize3((Pp - x).astype(F))
                        h = ((V.dot3(tt, nn) + F(1)) * F(0.5)).astype(F)
                        wb[:, c] = np.where((Pp == x).all(1), F(1), h * h + V.BACKFACE_FLOOR)
                    if v["chebyshev"]:
                        e = (xb - Pp).astype(F)
                        rr = V.len3(e)
                        px, py = V.encode(e)
                        m1, m2 = V.fetch(maps[q], V.texel_coordinate(px, res), V.texel_coordinate(py, res), res)
                        var = np.abs(m1 * m1 - m2).astype(F)
                        dl = (rr - m1).astype(F)
                        kk = (var / (var + dl * dl)).astype(F)
                        cheb = np.fmax((kk * kk) * kk, V.CHEBYSHEV_FLOOR).astype(F)
                        wv[:, c] = np.where((e == 0).all(1), F(1), np.where(rr > m1, cheb, F(1)))
                    c += 1
    return wb, wv, off


def sample(d, v, volume, atlas, pts, placement):
    """-> (n, 4) as hj_sample_probes_visible_placed defines it: an inactive corner's weight is 0 whatever its record holds - the
    validity word behind it is replaced by 0 and its back-face factor by 1 before probe_vis_ref.sample_weighted forms the product"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 8)
    wb, wv, off = corner_factors(d, v, atlas, pts, placement)
    vol = np.ascontiguousarray(volume, F).reshape(-1, P.WORDS).copy()
    vol[state(placement) != 0] = 0                                         # (w = 0 by a select: nothing of the record may leak)
    wb, wv = np.where(off, F(1), wb).astype(F), np.where(off, F(1), wv).astype(F)
    return V.sample_weighted(d, vol, pts, wb, wv)


# ---------------------------------------------------------------------------------------------------------- a scene without a GPU

def cube_trace(lo, hi):
    """-> a trace function over the closed axis-aligned cube [lo, hi] with outward normals, by brute force in float64 (the purpose
    tests need outcomes, not bits): the nearest face crossed at t > 0 within tMax, from inside or outside"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    def trace(ray):
        ray = np.asarray(ray, np.float64)
        o, dr, tmax = ray[:, 0:3], ray[:, 3:6], ray[:, 7]
        best = np.full(len(ray), np.inf)
        normal = np.zeros((len(ray), 3))
        for a in range(3):
            for side, plane in ((-1.0, lo[a]), (1.0, hi[a])):
                with np.errstate(divide="ignore", invalid="ignore"):
                    tt = (plane - o[:, a]) / dr[:, a]
                    hitp = o + dr * tt[:, None]
                ok = (tt > 1e-9) & (tt <= tmax) & (tt < best)
                for b in range(3):
                    if b != a:
                        ok &= (hitp[:, b] >= lo[b]) & (hitp[:, b] <= hi[b])
                best = np.where(ok, tt, best)
                normal[ok] = 0.0
                normal[ok, a] = side
        ids = np.where(np.isfinite(best), 0, -1).astype(np.int32)
        return ids, np.where(ids >= 0, best, 0.0).astype(F), normal.astype(F)
    return trace
