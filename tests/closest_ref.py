"""The reference of hj_closest_points and hj_distance_field: the text of kernels/hj_closest.h ("Distance queries")
restated in numpy float32, one rounding per operation, in the stated order.  dot3 and cross3 - the only places where fmaf matters -
are oracle.num_batch's, as in probe_vis_ref; sqrt and division are numpy's (IEEE).  The answer is BRUTE FORCE over all shapes with
the key rule: no tree, no bound, no slack - what the device's walk must equal bit for bit.

Shapes are a dict of float32 arrays in global shape order: spheres (ns, 4), quads (nq, 3, 3) = (origin, edge1, edge2), triangles
(nt, 3, 3) = (a, ab, ac) with ab = b - a, ac = c - a each one float32 subtraction (the uploaded tri_isect record)."""
import numpy as np

from hijiki_amd import abi
from probe_vis_ref import _bits, _num

U, F = np.uint32, np.float32
SLACK = F(2.0 ** -18)        # the absolute slack of the skipping bound, times the largest coordinate magnitude M
WORDS = abi.CLOSEST_WORDS


def shapes_of(cs):
    """the shape records of a compiled scene as the device holds them"""
    tri = cs.vertices[:, 0:3][cs.triangles.astype(np.int64)].astype(F).reshape(-1, 3, 3)
    t = np.stack([tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]], 1).astype(F) if len(tri) else np.zeros((0, 3, 3), F)
    q = np.stack([cs.quads[:, 0:3], cs.quads[:, 4:7], cs.quads[:, 8:11]], 1).astype(F) if len(cs.quads) else np.zeros((0, 3, 3), F)
    return dict(spheres=np.array(cs.spheres, F).reshape(-1, 4), quads=q, triangles=t)


def count(sh):
    return len(sh["spheres"]) + len(sh["quads"]) + len(sh["triangles"])


def dot3(p, q):
    p, q = np.broadcast_arrays(np.asarray(p, F), np.asarray(q, F))
    out = _num("dot3", np.concatenate([_bits(p).reshape(-1, 3), _bits(q).reshape(-1, 3)], 1))[:, 0].copy().view(F)
    return out.reshape(p.shape[:-1])


def cross3(p, q):
    p, q = np.broadcast_arrays(np.asarray(p, F), np.asarray(q, F))
    out = _num("cross3", np.concatenate([_bits(p).reshape(-1, 3), _bits(q).reshape(-1, 3)], 1))[:, 0:3].copy().view(F)
    return out.reshape(p.shape)


def _side(pq, n):
    return np.where(dot3(pq, n) >= F(0), F(1), F(-1)).astype(F)


def sphere(p, s):
    """p (..., 3), s (..., 4) broadcast together -> q, d2, u, v, side"""
    with np.errstate(all="ignore"):
        c, r = s[..., 0:3], s[..., 3]
        w = (p - c).astype(F)
        c, w = np.broadcast_arrays(c, w)
        l = np.sqrt(dot3(w, w)).astype(F)
        r = np.broadcast_to(r, l.shape)
        k = (r / l).astype(F)
        q = (c + (w * k[..., None]).astype(F)).astype(F)
        at = np.zeros_like(q)
        at[..., 0] = r
        q = np.where((l == 0)[..., None], (c + at).astype(F), q)
        t = (l - r).astype(F)
        return q, (t * t).astype(F), np.zeros_like(l), np.zeros_like(l), np.where(l >= r, F(1), F(-1)).astype(F)


def _floor0(x):
    return np.where(x < 0, F(0), x).astype(F)


def _clamp01(x):
    return np.where(x < 0, F(0), np.where(x > 1, F(1), x)).astype(F)


def triangle(p, t, region=False):
    """p (..., 3), t (..., 3, 3) = (a, ab, ac) broadcast together -> q, d2, u, v, side [, region 1 ... 7 in the header's numbering]"""
    with np.errstate(all="ignore"):
        a, ab, ac = t[..., 0, :], t[..., 1, :], t[..., 2, :]
        ap = (p - a).astype(F)
        ap, ab, ac, a = np.broadcast_arrays(ap, ab, ac, a)
        bp, cp = (ap - ab).astype(F), (ap - ac).astype(F)
        d1, d2, d3, d4, d5, d6 = dot3(ab, ap), dot3(ac, ap), dot3(ab, bp), dot3(ac, bp), dot3(ab, cp), dot3(ac, cp)
        vc = ((d1 * d4).astype(F) - (d3 * d2).astype(F)).astype(F)
        vb = ((d5 * d2).astype(F) - (d1 * d6).astype(F)).astype(F)
        va = ((d3 * d6).astype(F) - (d5 * d4).astype(F)).astype(F)
        m43, m56 = (d4 - d3).astype(F), (d5 - d6).astype(F)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (m43 >= 0) & (m56 >= 0)]
        w = (m43 / (m43 + m56).astype(F)).astype(F)
        fa, fb, fc = _floor0(va), _floor0(vb), _floor0(vc)
        k = (F(1) / ((fa + fb).astype(F) + fc).astype(F)).astype(F)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        us = [zero, one, zero, (d1 / (d1 - d3).astype(F)).astype(F), zero, (one - w).astype(F)]
        vs = [zero, zero, one, zero, (d2 / (d2 - d6).astype(F)).astype(F), w]
        u = np.select(conds, us, (fb * k).astype(F)).astype(F)
        v = np.select(conds, vs, (fc * k).astype(F)).astype(F)
        q = ((a + (ab * u[..., None]).astype(F)).astype(F) + (ac * v[..., None]).astype(F)).astype(F)
        pq = (p - q).astype(F)
        out = (q, dot3(pq, pq), u, v, _side(pq, cross3(ab, ac)))
        return out + (np.select(conds, [1, 2, 3, 4, 5, 6], 7),) if region else out


def quad(p, t, region=False):
    """p (..., 3), t (..., 3, 3) = (origin, edge1, edge2) -> q, d2, u, v, side [, (s, t) each 0 / 1 / 2: clamped low, inside, clamped high]"""
    with np.errstate(all="ignore"):
        o, e1, e2 = t[..., 0, :], t[..., 1, :], t[..., 2, :]
        w = (p - o).astype(F)
        w, o, e1, e2 = np.broadcast_arrays(w, o, e1, e2)
        s0, t0 = (dot3(w, e1) / dot3(e1, e1)).astype(F), (dot3(w, e2) / dot3(e2, e2)).astype(F)
        s, t_ = _clamp01(s0), _clamp01(t0)
        q = ((o + (e1 * s[..., None]).astype(F)).astype(F) + (e2 * t_[..., None]).astype(F)).astype(F)
        pq = (p - q).astype(F)
        out = (q, dot3(pq, pq), s, t_, _side(pq, cross3(e1, e2)))
        cls = lambda x: np.where(x < 0, 0, np.where(x > 1, 2, 1))                                # noqa: E731
        return out + ((cls(s0), cls(t0)),) if region else out


def per_shape(sh, pts):
    """every shape function on every point -> q (n, N, 3), d2, u, v, side (n, N), global shape order"""
    p = np.ascontiguousarray(pts, F)[:, None, 0:3]
    parts = []
    if len(sh["spheres"]): parts.append(sphere(p, sh["spheres"][None]))
    if len(sh["quads"]): parts.append(quad(p, sh["quads"][None]))
    if len(sh["triangles"]): parts.append(triangle(p, sh["triangles"][None]))
    return tuple(np.concatenate([x[k] for x in parts], 1) for k in range(5))


def closest(sh, points, block=512, ties=False):
    """points (n, 4) = (p, r) -> (n, 8) float32 records, by brute force: the candidate (d2 not NaN, d2 <= r * r) with the smallest key
    (d2 as uint32 bits, shape index); -1 and seven zeros for a miss, a NaN or negative r, a non-finite p.  ties=True: also, per point,
    how many candidates have the smallest d2 bits (0 for a miss)."""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    out = np.zeros((len(pts), WORDS), F)
    out[:, 0] = np.int32(-1).view(F)
    tied = np.zeros(len(pts), np.int64)
    if count(sh) == 0:
        return (out, tied) if ties else out
    for at in range(0, len(pts), block):
        pb = pts[at:at + block]
        q, d2, u, v, side = per_shape(sh, pb)
        with np.errstate(all="ignore"):
            r = pb[:, 3]
            r2 = (r * r).astype(F)
            ok = (d2 <= r2[:, None]) & (r >= 0)[:, None] & np.isfinite(pb[:, 0:3]).all(1)[:, None]
            key = np.where(ok, _bits(d2).reshape(d2.shape).astype(np.uint64), np.uint64(1) << np.uint64(40))
            best = np.argmin(key, 1)                                   # (the first smallest: the lower index)
            rows = np.arange(len(pb))
            hit = ok[rows, best]
            rec = np.zeros((len(pb), WORDS), F)
            rec[:, 0] = best.astype(np.int32).view(F)
            rec[:, 1] = np.sqrt(d2[rows, best]).astype(F)
            rec[:, 2:5] = q[rows, best]
            rec[:, 5], rec[:, 6], rec[:, 7] = u[rows, best], v[rows, best], side[rows, best]
            out[at:at + block][hit] = rec[hit]
            tied[at:at + block] = np.where(hit, (key == key[rows, best][:, None]).sum(1), 0)
    return (out, tied) if ties else out


def ids(rec):
    return np.ascontiguousarray(rec[:, 0]).view(np.int32)


def distance_field(sh, origin, spacing, cnt, max_distance, signed=True):
    """the grid of hj_probe_points (position = origin + (float)i * spacing per axis: a product, then a sum) through closest()
    -> (nz, ny, nx) float32"""
    origin, spacing = np.asarray(origin, F), np.asarray(spacing, F)
    ax = [(origin[a] + (np.arange(cnt[a]).astype(F) * spacing[a]).astype(F)).astype(F) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(x.size, F(max_distance), F)], 1).astype(F)
    rec = closest(sh, pts)
    val = (rec[:, 7] * rec[:, 1]).astype(F) if signed else rec[:, 1]
    return np.where(ids(rec) >= 0, val, F(max_distance)).astype(F).reshape(cnt[2], cnt[1], cnt[0])


# ---------------------------------------------------------------- an independent float64 computation (test_closest_host)

def exact_distance(sh, pts):
    """The distance from each point to each shape in float64 by other formulas than the text above: spheres analytically, a
    parallelogram or triangle as the minimum over its plane projection (when it falls inside, by solving the 2 x 2 normal equations)
    and its edges as clamped segments.  -> (n, N) float64.  For a sheared quad this is the true distance, which the text's
    projection does not claim to reach: callers compare rectangles."""
    p = np.asarray(pts, np.float64)[:, None, 0:3]

    def seg(a, b):
        ab = b - a
        den = (ab * ab).sum(-1)
        t = np.clip(((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        return np.linalg.norm(p - (a + ab * t[..., None]), axis=-1)

    def planar(o, e1, e2, tri):
        g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
        w = p - o
        b1, b2 = (w * e1).sum(-1), (w * e2).sum(-1)
        det = g11 * g22 - g12 * g12
        det = np.where(det != 0, det, np.nan)
        s, t = (b1 * g22 - b2 * g12) / det, (b2 * g11 - b1 * g12) / det
        inside = (s >= 0) & (t >= 0) & ((s + t <= 1) if tri else ((s <= 1) & (t <= 1)))
        face = np.where(inside, np.linalg.norm(w - e1 * s[..., None] - e2 * t[..., None], axis=-1), np.inf)
        if tri:
            edges = [seg(o, o + e1), seg(o, o + e2), seg(o + e1, o + e2)]
        else:
            edges = [seg(o, o + e1), seg(o, o + e2), seg(o + e1, o + e1 + e2), seg(o + e2, o + e1 + e2)]
        return np.minimum(face, np.minimum.reduce(edges))

    parts = []
    if len(sh["spheres"]):
        s = sh["spheres"].astype(np.float64)[None]
        parts.append(np.abs(np.linalg.norm(p - s[..., 0:3], axis=-1) - s[..., 3]))
    for name, tri in (("quads", False), ("triangles", True)):
        if len(sh[name]):
            t = sh[name].astype(np.float64)[None]
            parts.append(planar(t[..., 0, :], t[..., 1, :], t[..., 2, :], tri))
    return np.concatenate(parts, 1)


# ---------------------------------------------------------------- the skipping rule, restated (the tree walk itself is the device's)

GROW = F(1.0 + 2.0 ** -19)


def box_d2(p, lo, hi):
    """cq_box_d2: per axis max(lo - p, p - hi, 0), then dot3"""
    d = np.maximum(np.maximum((lo - p).astype(F), (p - hi).astype(F)), F(0)).astype(F)
    return dot3(d, d)


def skip_above(limit, slack):
    """cq_skip_above: a node whose box_d2 is above this is skipped at that limit"""
    with np.errstate(all="ignore"):
        t = ((np.sqrt(np.asarray(limit, F)).astype(F) + F(slack)).astype(F) * GROW).astype(F)
        return (t * t).astype(F)
