"""The reference of hj_trace_rays_all and hj_points_inside: the text of kernels/hj_multihit.h ("All-hit queries") restated
in numpy float32, one rounding per operation, in the stated order.  dot3 and cross3 - the only places where fmaf matters - are
oracle.num_batch's, as in closest_ref; sqrt and division are numpy's (IEEE).  The box test has no fused operation at all: np.where
and ~(a > b) are its selects and negated comparisons.

Shapes are closest_ref's dict (spheres (ns, 4), quads (nq, 3, 3) = (origin, edge1, edge2), triangles (nt, 3, 3) = (a, b - a, c - a)) in
global shape order; nodes are (N, 8) uint32 skip-link records in the uploaded layout (lo.xyz, shape index or abi.BVH_INNER, hi.xyz,
exit; the left child of record i is record i + 1; an exit >= N ends the walk); rays are (n, 8) float32 (o, d, tMin, tMax).

all_hits() walks the tree; all_hits(..., brute=True) takes every shape for reached, whatever the boxes say."""
import numpy as np

from closest_ref import count, cross3, dot3, shapes_of   # noqa: F401  (shapes_of, count: for the callers)
from hijiki_amd import abi

U, F = np.uint32, np.float32
MAX_HITS = abi.ALLHITS_MAX_HITS
DIRECTIONS = np.array(abi.INSIDE_DIRECTIONS, F)
MISS = np.array([np.int32(-1).view(F), 0, 0, 0], F)
END_OF_WALK = 0x3FFFFFFF                                 # the device's exit of a tree's last records (nodes_of_device)


def box_enter(o, inv, tmin, tmax, lo, hi):
    """mh_box_enter: o, inv, lo, hi (..., 3), tmin, tmax (...) -> bool"""
    with np.errstate(all="ignore"):
        t1 = ((lo - o).astype(F) * inv).astype(F)
        t2 = ((hi - o).astype(F) * inv).astype(F)
        lt = t1 < t2
        tn, tp = np.where(lt, t1, t2), np.where(lt, t2, t1)
        T0 = np.where(tn[..., 0] < tn[..., 1], tn[..., 1], tn[..., 0])
        T0 = np.where(T0 < tn[..., 2], tn[..., 2], T0)
        T1 = np.where(tp[..., 0] < tp[..., 1], tp[..., 0], tp[..., 1])
        T1 = np.where(T1 < tp[..., 2], T1, tp[..., 2])
        return ~(T0 > T1) & ~(T0 > tmax) & ~(T1 < tmin)


def inverse(d):
    with np.errstate(all="ignore"):
        return (F(1) / np.asarray(d, F)).astype(F)


def reached(nodes, rays):
    """the vectorised skip-link walk -> (ray index, shape index) of every leaf a ray reaches, and the nodes visited per ray"""
    nodes = np.ascontiguousarray(nodes, U).reshape(-1, 8)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    N, n = len(nodes), len(rays)
    f = nodes.view(F)
    lo, hi, a = f[:, 0:3], f[:, 4:7], nodes[:, 3]
    ex = np.minimum(nodes[:, 7].astype(np.int64), N)
    inner = a == abi.BVH_INNER
    o, inv, tmin, tmax = rays[:, 0:3], inverse(rays[:, 3:6]), rays[:, 6], rays[:, 7]
    cur = np.zeros(n, np.int64)
    act = np.arange(n) if N else np.zeros(0, np.int64)
    out_r, out_s, visited = [], [], np.zeros(n, np.int64)
    while len(act):
        c = cur[act]
        visited[act] += 1
        isin = inner[c]
        enter = box_enter(o[act], inv[act], tmin[act], tmax[act], lo[c], hi[c])
        out_r.append(act[~isin])
        out_s.append(a[c[~isin]].astype(np.int64))
        nxt = np.where(isin & enter, c + 1, ex[c])
        cur[act] = nxt
        act = act[nxt < N]
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, np.int64)             # noqa: E731
    return cat(out_r), cat(out_s), visited


def every_pair(sh, rays):
    """brute force: every shape is reached by every ray"""
    n, N = len(rays), count(sh)
    return np.repeat(np.arange(n), N), np.tile(np.arange(N), n)


def sphere_roots(r, s):
    """r (m, 8), s (m, 4) -> t0, t1, ok0, ok1: intersect_sphere's arithmetic up to the roots, each root under the caller's range"""
    with np.errstate(all="ignore"):
        o, d, tmin, tmax = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
        l = (o - s[:, 0:3]).astype(F)
        b = (F(2) * dot3(d, l)).astype(F)
        c = (dot3(l, l) - (s[:, 3] * s[:, 3]).astype(F)).astype(F)
        D = ((b * b).astype(F) - (F(4) * c).astype(F)).astype(F)
        some = ~(D < 0)
        q = np.sqrt(D).astype(F)
        t0 = (F(-0.5) * (b + q).astype(F)).astype(F)
        t1 = (F(-0.5) * (b - q).astype(F)).astype(F)
        return t0, t1, some & (tmin <= t0) & (t0 <= tmax), some & (tmin <= t1) & (t1 <= tmax)


def planar(r, rec, tri):
    """r (m, 8), rec (m, 3, 3) -> t, u, v, ok, facing: triangle_test (tri) or quad_test on the record (origin, edge1, edge2)"""
    with np.errstate(all="ignore"):
        o, d, tmin, tmax = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
        a, e1, e2 = rec[:, 0], rec[:, 1], rec[:, 2]
        n = cross3(e1, e2)
        ro = (o - a).astype(F)
        q = cross3(ro, d)
        dn = dot3(d, n)
        k = (F(1) / dn).astype(F)
        u = (k * (-dot3(q, e2)).astype(F)).astype(F)
        v = (k * dot3(q, e1)).astype(F)
        out = (u < 0) | (v < 0) | ((u + v).astype(F) > 1) if tri else (u < 0) | (u > 1) | (v < 0) | (v > 1)
        t = (k * (-dot3(n, ro)).astype(F)).astype(F)
        ok = ~out & (tmin <= t) & (t <= tmax)
        return t, u, v, ok, np.where(dn > 0, 1, np.where(dn < 0, -1, 0)).astype(np.int32)


def candidates(sh, rays, ri, si):
    """the candidates of the (ray, shape) pairs -> ray, shape, root, t, u, v, facing, one row per candidate"""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    ns, nq = len(sh["spheres"]), len(sh["quads"])
    rows = []

    def add(r, s, root, t, u, v, face, ok):
        rows.append((r[ok], s[ok], np.full(int(ok.sum()), root, np.int64), t[ok], u[ok], v[ok], face[ok]))

    m = si < ns
    if m.any():
        r, s = ri[m], si[m]
        t0, t1, ok0, ok1 = sphere_roots(rays[r], sh["spheres"][s])
        z, one = np.zeros(len(r), F), np.ones(len(r), F)
        add(r, s, 0, t0, z, z, np.full(len(r), -1, np.int32), ok0)
        add(r, s, 1, t1, one, z, np.full(len(r), 1, np.int32), ok1)
    for tri, m in ((False, (si >= ns) & (si < ns + nq)), (True, si >= ns + nq)):
        if m.any():
            r, s = ri[m], si[m]
            rec = sh["triangles"][s - ns - nq] if tri else sh["quads"][s - ns]
            t, u, v, ok, face = planar(rays[r], rec, tri)
            add(r, s, 0, t, u, v, face, ok)
    if not rows:
        e = np.zeros(0, np.int64)
        return e, e, e, np.zeros(0, F), np.zeros(0, F), np.zeros(0, F), np.zeros(0, np.int32)
    return tuple(np.concatenate([x[k] for x in rows]) for k in range(7))


def all_hits(sh, nodes, rays, K=MAX_HITS, brute=False):
    """-> counts (n,) uint32, crossings (n,) int32, hits (n, K, 4) float32: the contract.  brute: every shape is a candidate's shape."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n = len(rays)
    counts, cross = np.zeros(n, np.int64), np.zeros(n, np.int64)
    hits = np.tile(MISS, (n, K, 1))
    if brute:
        ri, si = every_pair(sh, rays)
    else:
        ri, si, _ = reached(nodes, rays)
    r, s, root, t, u, v, face = candidates(sh, rays, ri, si)
    np.add.at(counts, r, 1)
    np.add.at(cross, r, face)
    order = np.lexsort((root, s, t, r))                                    # by ray, then the key (t as a float, shape index, root)
    r, s, t, u, v = r[order], s[order], t[order], u[order], v[order]
    first = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))[:-1]]) if n else np.zeros(0, np.int64)
    rank = np.arange(len(r)) - first[r]
    keep = rank < K
    rec = np.stack([s.astype(np.int32).view(F), t, u, v], 1).astype(F) if len(r) else np.zeros((0, 4), F)
    hits[r[keep], rank[keep]] = rec[keep]
    return counts.astype(U), cross.astype(np.int32), hits


def point_rays(points):
    """points (n, 4) -> (3 n, 8) rays: point i's three rays at 3 i .. 3 i + 2, tMin = 0, tMax = +inf"""
    p = np.ascontiguousarray(points, F).reshape(-1, 4)
    rays = np.zeros((len(p), 3, 8), F)
    rays[:, :, 0:3] = p[:, None, 0:3]
    rays[:, :, 3:6] = DIRECTIONS[None]
    rays[:, :, 7] = np.inf
    return rays.reshape(-1, 8)


def vote(counts, cross, parity=False):
    """per point's three rays -> inside (n,) uint32, votes (n,) uint32"""
    yes = (counts.reshape(-1, 3) & 1) != 0 if parity else cross.reshape(-1, 3) > 0
    votes = yes.sum(1).astype(U)
    return (votes >= 2).astype(U), votes


def points_inside(sh, nodes, points, parity=False, brute=False):
    counts, cross, _ = all_hits(sh, nodes, point_rays(points), 0, brute)
    return vote(counts, cross, parity)


def nodes_of_device(tree):
    """Renderer.scene_tree()'s second copy of the uploaded tree in the uploaded layout: what the device's walk reads"""
    rec = np.array(tree["records"][tree["root2"]:], U)
    N = len(rec)
    inner = (rec[:, 3] & 0x80000000) != 0
    rec[inner, 3] = abi.BVH_INNER
    e = rec[:, 7].astype(np.int64)
    rec[:, 7] = np.where(e == END_OF_WALK, N, e - tree["root2"]).astype(U)
    return rec


def same_walk(a, b):
    """two node arrays give the same walk: boxes, leaves, inner marks, exits (every exit >= N is the end)"""
    a, b = (np.ascontiguousarray(x, U).reshape(-1, 8).copy() for x in (a, b))
    if a.shape != b.shape:
        return False
    for x in (a, b):
        x[:, 7] = np.minimum(x[:, 7], len(x))
    return bool((a == b).all())
