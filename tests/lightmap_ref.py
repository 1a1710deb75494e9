"""The reference of hj_lightmap_texels and of hj_bake_lightmap's image steps: include/hijiki_hip.h's contract restated in numpy
float32 - vectorised over texels, one triangle at a time in ascending index, every operation on np.float32 arrays in the written
order.  normalize is the oracle's (oracle.num_batch, the numeric contract's: test_num_gpu.py pins the device's to it).  Shares no
text with the kernels: the closed box of the predicate is evaluated first, on the texel centres themselves, so no integer bounding
box exists here.  coverage_owner_batched is the same predicate for meshes of 10^5 to 10^6 triangles: the centres are strictly
increasing, so np.searchsorted finds the centres inside a closed interval exactly, by the same comparisons; the (triangle, texel)
pairs of all small triangles are evaluated in one batch, and the owner is the minimum index (np.minimum.at).
test_lightmap_scale_host.py pins it to coverage_owner word for word."""
import numpy as np

U, F = np.uint32, np.float32
NONE = 0xFFFFFFFF
PI = F(3.14159274)


def centres(n):
    return (np.arange(n, dtype=F) + F(0.5)) / F(n)


def edge(su, sv, tu, tv, pu, pv):
    return (tu - su) * (pv - sv) - (tv - sv) * (pu - su)


def edges(a, b, c, pu, pv):
    """a, b, c: (u, v) pairs (scalars or arrays), pu, pv arrays -> e0, e1, e2, s in float32"""
    e0 = edge(b[0], b[1], c[0], c[1], pu, pv)
    e1 = edge(c[0], c[1], a[0], a[1], pu, pv)
    e2 = edge(a[0], a[1], b[0], b[1], pu, pv)
    return e0, e1, e2, (e0 + e1) + e2


def covers(uv, W, H):
    """uv: (3, 2) float32 -> (ys, xs, mask (len(ys), len(xs))): the texels whose centre lies in the closed box, and which of them
    the triangle covers"""
    uv = np.asarray(uv, F)
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 0), bool))
    if not np.isfinite(uv).all():
        return none
    pu, pv = centres(W), centres(H)
    xs = np.flatnonzero((uv[:, 0].min() <= pu) & (pu <= uv[:, 0].max()))
    ys = np.flatnonzero((uv[:, 1].min() <= pv) & (pv <= uv[:, 1].max()))
    if not len(xs) or not len(ys):
        return none
    with np.errstate(all="ignore"):
        e0, e1, e2, s = edges(uv[0], uv[1], uv[2], pu[xs][None, :], pv[ys][:, None])
        mask = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (s != 0)
    return ys, xs, mask


def coverage_owner(triangles, vertices, W, H, first=0, num=0):
    """-> owner (H, W) uint32 by coverage alone (before the normals are looked at)"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    vt = np.asarray(vertices, F).reshape(-1, 8)
    last = len(tri) if num == 0 else first + num
    owner = np.full((H, W), NONE, U)
    for i in range(first, last):
        ys, xs, mask = covers(vt[tri[i]][:, [3, 7]], W, H)
        if mask.any():
            sub = owner[np.ix_(ys, xs)]
            sub[mask & (sub == NONE)] = i                               # ascending i: the first to arrive is the lowest
            owner[np.ix_(ys, xs)] = sub
    return owner


def coverage_owner_batched(triangles, vertices, W, H, first=0, num=0, small=64, chunk=1 << 16):
    """coverage_owner vectorised over triangles.  A triangle's candidates are the centres pu[x0:x1] x pv[y0:y1] inside its closed
    box (searchsorted: 'left' is the first centre >= min, 'right' one past the last centre <= max).  Triangles with at most `small`
    candidates: every (triangle, texel) pair at once, `chunk` triangles at a time, in edges' expressions; the others one by one
    through covers.  The minimum commutes, so the order of the two parts does not show."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    vt = np.asarray(vertices, F).reshape(-1, 8)
    last = len(tri) if num == 0 else first + num
    uv = vt[tri[first:last]][:, :, [3, 7]]                               # (m, 3, 2)
    finite = np.isfinite(uv).all(axis=(1, 2))
    uv = np.where(finite[:, None, None], uv, F(0))
    pu, pv = centres(W), centres(H)
    x0, x1 = np.searchsorted(pu, uv[:, :, 0].min(axis=1), "left"), np.searchsorted(pu, uv[:, :, 0].max(axis=1), "right")
    y0, y1 = np.searchsorted(pv, uv[:, :, 1].min(axis=1), "left"), np.searchsorted(pv, uv[:, :, 1].max(axis=1), "right")
    nx, ny = np.where(finite, x1 - x0, 0), np.where(finite, y1 - y0, 0)
    cand = nx * ny
    owner = np.full(H * W, NONE, U)
    few = np.flatnonzero((cand > 0) & (cand <= small))
    for c0 in range(0, len(few), chunk):
        j = few[c0:c0 + chunk]
        rep = np.repeat(j, cand[j])                                      # the triangle of each pair
        k = np.arange(len(rep)) - np.repeat(np.cumsum(cand[j]) - cand[j], cand[j])
        ry = k // nx[rep]
        xs, ys = x0[rep] + (k - ry * nx[rep]), y0[rep] + ry
        a, b, c = ((uv[rep, v, 0], uv[rep, v, 1]) for v in range(3))
        with np.errstate(all="ignore"):
            e0, e1, e2, s = edges(a, b, c, pu[xs], pv[ys])
            mask = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (s != 0)
        np.minimum.at(owner, (ys * W + xs)[mask], (first + rep[mask]).astype(U))
    owner = owner.reshape(H, W)
    for j in np.flatnonzero(cand > small):
        ys, xs, mask = covers(uv[j], W, H)
        sub = owner[np.ix_(ys, xs)]
        owner[np.ix_(ys, xs)] = np.where(mask, np.minimum(sub, U(first + j)), sub)
    return owner


def normalize3(v):
    from oracle import hj_oracle as oracle
    if not len(v):
        return np.zeros((0, 3), F)
    return oracle.num_batch("normalize3", np.ascontiguousarray(v, F).view(U))[:, 0:3].copy().view(F)


def texels(triangles, vertices, W, H, first=0, num=0, seed=0, seed_stride=1, offset=0.0, batched=False):
    """-> (points (count, 8) float32 in ascending texel index, owner (H, W) uint32); batched: coverage by coverage_owner_batched"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    vt = np.asarray(vertices, F).reshape(-1, 8)
    owner = (coverage_owner_batched if batched else coverage_owner)(tri, vt, W, H, first, num)
    t = np.flatnonzero(owner.ravel() != NONE)
    o = owner.ravel()[t].astype(np.int64)
    A, B, C = (vt[tri[o, k]] if len(o) else np.zeros((0, 8), F) for k in range(3))
    pu, pv = centres(W)[t % W], centres(H)[t // W]
    with np.errstate(all="ignore"):
        _, e1, e2, s = edges((A[:, 3], A[:, 7]), (B[:, 3], B[:, 7]), (C[:, 3], C[:, 7]), pu, pv)
        hu, hv = e1 / s, e2 / s
        l0 = (F(1.0) - hu) - hv
        l0, hu, hv = l0[:, None], hu[:, None], hv[:, None]
        P = (A[:, 0:3] * l0 + B[:, 0:3] * hu) + C[:, 0:3] * hv
        n = normalize3((A[:, 4:7] * l0 + B[:, 4:7] * hu) + C[:, 4:7] * hv)
        keep = np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
        pos = P + n * F(offset)
    owner.reshape(-1)[t[~keep]] = NONE
    t, pos, n = t[keep], pos[keep], n[keep]
    pts = np.zeros((len(t), 8), F)
    pts[:, 0:3], pts[:, 3:6] = pos, n
    w = pts.view(U)
    w[:, 6] = ((int(seed) + t.astype(np.uint64) * int(seed_stride)) & 0xFFFFFFFF).astype(U)
    w[:, 7] = t.astype(U)
    return pts, owner


def scatter(points, records, W, H, spp):
    """points (n, 8), records (n, 8: hj_trace_irradiance's) -> (H, W, 4) float32"""
    img = np.zeros((H * W, 4), F)
    t = np.ascontiguousarray(points, F).view(U)[:, 7]
    scale = PI / F(spp)
    img[t, 0:3] = np.asarray(records, F)[:, 0:3] * scale
    img[t, 3] = 1.0
    return img.reshape(H, W, 4)


def dilate(img):
    """one gutter pass"""
    H, W, _ = img.shape
    pad = np.zeros((H + 2, W + 2, 4), F)
    pad[1:-1, 1:-1] = img
    total, k = np.zeros((H, W, 3), F), np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                v = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                on = v[:, :, 3] > 0
                total = np.where(on[:, :, None], total + v[:, :, 0:3], total)
                k += on
        fill = (img[:, :, 3] == 0) & (k > 0)
        out = img.copy()
        mean = total / np.maximum(k, 1).astype(F)[:, :, None]
    out[fill, 0:3] = mean[fill]
    out[fill, 3] = 0.5
    return out


def image(points, records, W, H, spp, gutter):
    img = scatter(points, records, W, H, spp)
    for _ in range(gutter):
        img = dilate(img)
    return img
