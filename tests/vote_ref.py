"""The device ray vote (kernels/hj_vote.h) restated in plain numpy, for tests/test_vote_host.py and tests/test_vote_gpu.py (DESIGN.md 4,
"The vote's two halves, pinned").  Nothing here reads the code under test: records are (N, 8) uint32 arrays in the reference's layout
(box minimum, shape word, box maximum, exit), rays (n, 8) float32 (origin, direction, tMin, tMax), gains Python integers.

  exchange_ref   the exchange: children change places where gain_r > gain_l, a subtree keeps its size, the last child inherits its
                 parent's exit
  cast_counts    per ray and ancestor of its leaf: the nodes of the other child the ray enters (ci), those it enters in front of its
                 hit (ct) - the slab test in float32, operation for operation
  cast_ref       ... summed into the gains as a closest-hit or a shadow ray votes
  closest_f64    the nearest and second-nearest hit of every ray by brute force over all shapes in float64"""
import numpy as np

INNER = 0xFFFFFFFF
MISS = 0xFFFFFFFF
EPS = np.float32(1e-4)                                   # M_EPS (kernels/hj_num.h kEps)
F32_INF = np.float32(np.inf)


# ---------------------------------------------------------------------------------------------------------------- the exchange
def exchange_ref(nodes, gain_l, gain_r):
    """-> (records, exchanged nodes, levels that held an inner node).  Explicit stack; the root keeps its exit whatever it is."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    N = len(nodes)
    out = np.zeros_like(nodes)
    shape, exits = nodes[:, 3].tolist(), nodes[:, 7].tolist()
    gl, gr = [int(x) for x in gain_l], [int(x) for x in gain_r]
    new_pos, new_exit = [0] * N, [0] * N
    exchanged = levels = 0
    stack = [(0, N, 0, exits[0], 0)] if N else []         # record, end of its subtree, new position, new exit, depth
    while stack:
        i, end, pos, ex, depth = stack.pop()
        new_pos[i], new_exit[i] = pos, ex
        if shape[i] != INNER:
            continue
        levels = max(levels, depth + 1)
        l = i + 1
        r = exits[l]
        assert l < r < end, f"exchange_ref: record {i} is no inner node of a pre-order skip-link tree"
        size_l, size_r = r - l, end - r
        if gr[i] > gl[i]:                                 # strictly: ties, and nodes no ray voted on, keep their order
            exchanged += 1
            stack.append((r, end, pos + 1, pos + 1 + size_r, depth + 1))
            stack.append((l, r, pos + 1 + size_r, ex, depth + 1))
        else:
            stack.append((l, r, pos + 1, pos + 1 + size_l, depth + 1))
            stack.append((r, end, pos + 1 + size_l, ex, depth + 1))
    if N:
        out[new_pos] = nodes
        out[new_pos, 7] = np.array(new_exit, np.uint64).astype(np.uint32)
    return out, exchanged, levels


def moved_gains(nodes, gain_l, gain_r):
    """the gains carried along with their records by exchange_ref(nodes, gain_l, gain_r), an exchanged node's two gains changing sides
    with its children: what a second exchange of the result would be handed"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    tagged = nodes.copy()
    inner = np.nonzero(nodes[:, 3] == INNER)[0]
    tagged[:, 0] = np.arange(len(nodes), dtype=np.uint32)                  # (word 0 is carried, not read: the record's old place)
    out, _, _ = exchange_ref(tagged, gain_l, gain_r)
    old = out[:, 0].astype(np.int64)
    gl, gr = [int(gain_l[k]) for k in old], [int(gain_r[k]) for k in old]
    swapped = {int(k) for k in inner if int(gain_r[k]) > int(gain_l[k])}
    for p, k in enumerate(old.tolist()):
        if k in swapped:
            gl[p], gr[p] = gr[p], gl[p]
    return gl, gr


# ---------------------------------------------------------------------------------------------------------------- the counting
def entry_f32(nodes, rays):
    """hj::vote::entry for every (ray, record): (entered (n, N) bool, entry distance t0 (n, N) float32).  float32 throughout, every
    product rounded before its sum (contraction is off in that file), minNum / maxNum as np.fmin / np.fmax, 1 / d correctly rounded."""
    f = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8).view(np.float32)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    lo, hi = f[:, 0:3], f[:, 4:7]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.float32(1.0) / rays[:, 3:6]
        off = -(rays[:, 0:3] * inv)
        t0 = t1 = None
        for k in range(3):
            tn = lo[None, :, k] * inv[:, None, k] + off[:, None, k]
            tp = hi[None, :, k] * inv[:, None, k] + off[:, None, k]
            assert tn.dtype == np.float32 and tp.dtype == np.float32
            near, far = np.fmin(tn, tp), np.fmax(tn, tp)
            t0 = near if t0 is None else np.fmax(t0, near)
            t1 = far if t1 is None else np.fmin(t1, far)
        entered = (t0 < t1 + EPS) & (t0 < rays[:, 7:8]) & (t1 > rays[:, 6:7])
    return entered, t0


def cast_counts(nodes, rays, hits, chunk=512):
    """hits = (leaf position per ray or MISS, t per ray as float32).  -> a list of (ray, node, side, ci, ct, depth) int tuples, one per
    ray and ancestor of its leaf, side 0: the leaf is under the left child (the vote goes to gain_l).  The walk of the other child is
    stated bottom-up: F[j] = nodes of j's subtree the walk enters when it comes to j = entered[j] * (1 + F[left] + F[right]), and the
    same with "enters in front of the hit" counted, for every ray at once."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    pos_all = np.asarray(hits[0], np.int64)
    t_all = np.ascontiguousarray(hits[1], np.float32)
    N = len(nodes)
    shape, exits = nodes[:, 3].tolist(), nodes[:, 7].tolist()
    out = []
    for c0 in range(0, len(rays), chunk):
        sel = slice(c0, min(len(rays), c0 + chunk))
        entered, t0 = entry_f32(nodes, rays[sel])
        front = entered & (t0 < t_all[sel, None])
        F = np.zeros((N, entered.shape[0]), np.int64)
        T = np.zeros((N, entered.shape[0]), np.int64)
        e_t, f_t = entered.T.astype(np.int64), front.T.astype(np.int64)
        for j in range(N - 1, -1, -1):
            if shape[j] != INNER:
                F[j], T[j] = e_t[j], f_t[j]
            else:
                r = exits[j + 1]
                F[j] = e_t[j] * (1 + F[j + 1] + F[r])
                T[j] = e_t[j] * (f_t[j] + T[j + 1] + T[r])
        for k in range(entered.shape[0]):
            pos = int(pos_all[c0 + k])
            if pos == MISS:
                continue
            assert 0 <= pos < N and shape[pos] != INNER
            i, end, depth = 0, N, 0
            while i != pos:
                l = i + 1
                r = exits[l]
                if pos < r:
                    out.append((c0 + k, i, 0, int(F[r, k]), int(T[r, k]), depth))
                    i, end = l, r
                else:
                    out.append((c0 + k, i, 1, int(F[l, k]), int(T[l, k]), depth))
                    i = r
                depth += 1
    return out


def gains_of(counts, N, any_hit, w_shadow):
    """a closest-hit ray is spared ci - ct nodes (4 quarters each), a shadow ray all ci (w_shadow quarters each)"""
    gl, gr = [0] * N, [0] * N
    for _, i, side, ci, ct, _ in counts:
        g = ci * int(w_shadow) if any_hit else (ci - ct) * 4
        if side == 0:
            gl[i] += g
        else:
            gr[i] += g
    return gl, gr


def cast_ref(nodes, rays, hits, any_hit, w_shadow):
    return gains_of(cast_counts(nodes, rays, hits), len(np.asarray(nodes).reshape(-1, 8)), any_hit, w_shadow)


# ---------------------------------------------------------------------------------------------------------------- the closest hit
def closest_f64(cs, rays, chunk=256):
    """closest_chunk_f64 over all rays, `chunk` at a time (the intermediate arrays are rays x shapes x 3 doubles)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    parts = [closest_chunk_f64(cs, rays[k:k + chunk]) for k in range(0, len(rays), chunk)]
    return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}


def closest_chunk_f64(cs, rays):
    """Brute force over all shapes of `cs` (spheres (S, 4), quads (Q, 12), triangles (T, 3) over vertices (V, 8)) in float64, the
    float32 inputs taken as they are.  -> dict of per-ray arrays: shape (-1: none) and t of the nearest accepted hit, t2 of the
    second-nearest accepted candidate (inf: none; a sphere's other root counts as one, so a grazing ray has t2 close to t), edge = the smallest
    distance of a barycentric coordinate from an edge over the plane hits at t <= (1 + 1e-4) * t whether inside or not (inf: none),
    window = the smallest relative distance of any candidate's t from tMin or tMax, graze = the smallest |r^2 - d^2| over the spheres
    the ray passes at distance d no further along than that hit (a choice of rays may keep away from it; `ambiguous` does not read it)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8).astype(np.float64)
    o, d, tmin, tmax = rays[:, None, 0:3], rays[:, None, 3:6], rays[:, 6:7], rays[:, 7:8]
    n = len(rays)
    cand_t, cand_id, cand_edge = [], [], []              # (n, k) blocks: t (inf: no candidate), shape id, barycentric margin
    graze_t, graze_d = np.full((n, 1), np.inf), np.full((n, 1), np.inf)
    ns, nq = len(cs.spheres), len(cs.quads)
    if ns:
        sp = np.asarray(cs.spheres, np.float64)
        oc = o - sp[None, :, 0:3]
        a = (d * d).sum(-1)
        b = (oc * d).sum(-1)
        c = (oc * oc).sum(-1) - sp[None, :, 3] ** 2
        disc = b * b - a * c
        sq = np.sqrt(np.maximum(disc, 0.0))
        graze_t, graze_d = -b / a, np.abs(disc / a)      # closest approach: where along the ray, and |r^2 - distance^2| there
        for root in ((-b - sq) / a, (-b + sq) / a):
            cand_t.append(np.where(disc >= 0.0, root, np.inf))
            cand_id.append(np.broadcast_to(np.arange(ns), (n, ns)))
            cand_edge.append(np.full((n, ns), np.inf))

    def planar(a0, ab, ac, first, quad):
        nrm = np.cross(ab, ac)
        ro = o - a0[None]
        q = np.cross(ro, np.broadcast_to(d, ro.shape))
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / (d * nrm[None]).sum(-1)
            u, v, t = inv * -(q * ac[None]).sum(-1), inv * (q * ab[None]).sum(-1), inv * -(nrm[None] * ro).sum(-1)
            margin = np.minimum(np.minimum(u, v), np.minimum(1.0 - u, 1.0 - v) if quad else 1.0 - u - v)
        ok = np.isfinite(t)
        cand_t.append(np.where(ok, t, np.inf))
        cand_id.append(np.broadcast_to(first + np.arange(len(a0)), t.shape))
        cand_edge.append(np.where(ok, margin, -np.inf))
    if nq:
        qd = np.asarray(cs.quads, np.float64)
        planar(qd[:, 0:3], qd[:, 4:7], qd[:, 8:11], ns, True)
    if len(cs.triangles):
        p = np.asarray(cs.vertices, np.float64)[:, 0:3][np.asarray(cs.triangles, np.int64)]
        planar(p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], ns + nq, False)
    t, ids, edge = np.concatenate(cand_t, 1), np.concatenate(cand_id, 1), np.concatenate(cand_edge, 1)
    in_window = (t >= tmin) & (t <= tmax)
    accepted = in_window & (edge >= 0.0)
    ta = np.where(accepted, t, np.inf)
    best = np.argmin(ta, axis=1)
    rows = np.arange(n)
    t_best = ta[rows, best]
    hit = np.isfinite(t_best)
    others = ta.copy()
    others[rows, best] = np.inf
    t2 = others.min(axis=1)
    scale = np.maximum(1.0, np.abs(np.where(np.isfinite(t), t, 0.0)))
    with np.errstate(invalid="ignore"):
        near_end = np.minimum(np.abs(t - tmin), np.where(np.isfinite(tmax), np.abs(t - tmax), np.inf)) / scale
    near_end = np.where(np.isfinite(t) & (edge > -1e-4), near_end, np.inf)
    limit = np.where(hit, t_best * (1.0 + 1e-4), np.inf)[:, None]
    relevant = np.isfinite(t) & (t <= limit) & (t >= tmin * (1.0 - 1e-4)) & np.isfinite(edge)
    edge_margin = np.where(relevant, np.abs(edge), np.inf).min(axis=1)
    grazes = (graze_t >= tmin) & (graze_t <= np.minimum(limit, tmax))
    return {"shape": np.where(hit, ids[rows, best], -1).astype(np.int64), "t": t_best, "t2": t2, "edge": edge_margin,
            "window": near_end.min(axis=1), "graze": np.where(grazes, graze_d, np.inf).min(axis=1)}


def ambiguous(ref):
    """the rays whose closest hit the float64 reference alone calls too close to decide in float32: a second candidate within 1e-4
    relative of the nearest, a candidate's t within 1e-4 of a window end, a barycentric within 1e-4 of an edge"""
    t, t2 = ref["t"], ref["t2"]
    with np.errstate(invalid="ignore"):
        second = np.isfinite(t) & (np.abs(t2 - t) <= 1e-4 * np.maximum(1.0, np.abs(t)))
    return second | (ref["window"] <= 1e-4) | (ref["edge"] <= 1e-4)
