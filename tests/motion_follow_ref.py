"""The reference of hj_render_motion_followed: include/hijiki_hip.h's contract restated in numpy float32, in the written operation
order, over whole-image arrays.  The chains are made as follow_ref makes the followed AOVs': follow_ref.continue_rays alternated with
a trace the caller brings - on the GPU hj_trace_rays itself (test_follow_gpu.gpu_trace), without one the oracle's intersect
(follow_ref.oracle_trace).  The first-hit record, the projection and the hit point's fma are motion_ref's.  Shares no text with the
kernels: no list, no tiles, no walk."""
import numpy as np

import follow_ref as R
import motion_ref as M
import temporal_ref as T
from closest_ref import dot3
from hijiki_amd import abi

U, F = np.uint32, np.float32
LEFT, NONE = abi.MOTION_LEFT, abi.MOTION_NONE
REFLECTS = (R.MIRROR, R.REFLECT_FR, R.REFLECT_TIR)


def householder(Mat, n):
    """M -> M - 2 (M n) n^T for k matrices (k, 3, 3: [row, column]) and normals (k, 3): w_i = (M_i0 n.x + M_i1 n.y) + M_i2 n.z,
    w2_i = 2 w_i, M_ij = M_ij - w2_i n_j"""
    Mat, n = np.asarray(Mat, F), np.asarray(n, F)
    w = ((Mat[:, :, 0] * n[:, 0:1]).astype(F) + (Mat[:, :, 1] * n[:, 1:2]).astype(F)).astype(F) + (Mat[:, :, 2] * n[:, 2:3]).astype(F)
    w2 = (F(2) * w.astype(F)).astype(F)
    return (Mat - (w2[:, :, None] * n[:, None, :]).astype(F)).astype(F)


def segment_point(t, d, o):
    """fma(t, d, o) per channel with an origin per record: dot3((o, 0, t), (1, 0, d)), as motion_ref.hit_point"""
    out = np.zeros(d.shape, F)
    one, zero = np.ones_like(t), np.zeros_like(t)
    for k in range(3):
        out[:, k] = dot3(np.stack([o[:, k], zero, t], -1), np.stack([one, zero, d[:, k]], -1))
    return out


def shape_points(cs, spheres, quads, vertices, ids, n, u, v):
    """X of shapes ids (all inside the scene) on the arrays given: a sphere's at the normal n, a quad's and a triangle's at (u, v)"""
    ns, nq = len(cs.spheres), len(cs.quads)
    X = np.zeros((len(ids), 3), F)
    m = ids < ns
    if m.any():
        s = np.asarray(spheres, F)[ids[m]]
        X[m] = s[:, 0:3] + (n[m] * s[:, 3:4]).astype(F)
    m = (ids >= ns) & (ids < ns + nq)
    if m.any():
        q = np.asarray(quads, F)[ids[m] - ns]
        uu, vv = u[m][:, None], v[m][:, None]
        X[m] = (q[:, 0:3] + (q[:, 4:7] * uu).astype(F)).astype(F) + (q[:, 8:11] * vv).astype(F)
    m = ids >= ns + nq
    if m.any():
        tri = np.asarray(cs.triangles).astype(np.int64)[ids[m] - ns - nq]
        vert = np.asarray(vertices, F)[:, 0:3]
        a, b, c = vert[tri[:, 0]], vert[tri[:, 1]], vert[tri[:, 2]]
        uu, vv = u[m][:, None], v[m][:, None]
        l0 = ((F(1) - uu).astype(F) - vv).astype(F)
        X[m] = ((a * l0).astype(F) + (b * uu).astype(F)).astype(F) + (c * vv).astype(F)
    return X.astype(F)


def chains(cs, W, H, max_follow, trace):
    """The chains of the centre rays -> dict: first (n, 4) the first raw hits; last (n, 4) each chain's last raw hit; o, d (n, 3) its
    last segment; depth (n,) the float32 sum of the t values BEFORE the last hit; count (n,) continuations taken; left (n,) the last
    continuation hit nothing; Mat (n, 3, 3) the product of the reflect events' Householder matrices; length (n,) continuations that
    hit"""
    rays = M.centre_rays(cs.desc.camera, W, H)
    n = len(rays)
    hits, surf = trace(rays)
    c = dict(first=np.array(hits, F), last=np.array(hits, F), o=rays[:, 0:3].copy(), d=rays[:, 3:6].copy(), depth=np.zeros(n, F), count=np.zeros(n, np.int32),
             left=np.zeros(n, bool), Mat=np.tile(np.eye(3, dtype=F), (n, 1, 1)), length=np.zeros(n, np.int32), d0=rays[:, 3:6].copy())
    live, cur = np.arange(n), rays
    for _ in range(int(max_follow)):
        if not len(live):
            break
        nxt, cls = R.continue_rays(cs, cur, hits, surf)
        go = cls != R.END
        if not go.any():
            break
        idx = live[go]
        c["depth"][idx] = (c["depth"][idx] + hits[go, 1]).astype(F)
        c["o"][idx], c["d"][idx] = nxt[go, 0:3], nxt[go, 3:6]
        c["count"][idx] += 1
        refl = np.isin(cls[go], REFLECTS)
        if refl.any():
            c["Mat"][idx[refl]] = householder(c["Mat"][idx[refl]], np.asarray(surf, F)[go][refl, 3:6])
        live, cur = idx, nxt[go]
        hits, surf = trace(cur)
        hit = hits[:, 0].copy().view(np.int32) >= 0
        c["last"][live[hit]] = hits[hit]
        c["left"][live[~hit]] = True
        c["length"][live[hit]] += 1
        live, cur, hits, surf = live[hit], cur[hit], hits[hit], surf[hit]
    return c


def render_motion_followed(cs, prev, W, H, max_follow, trace, detail=False):
    """hj_render_motion_followed's (H, W, 4) for the uploaded scene cs and the previous state prev (a motion_ref.Prev) [, detail: the
    chains and D (H, W): the followed depth]"""
    cam = cs.desc.camera
    c = chains(cs, W, H, max_follow, trace)
    f = c["first"]
    base = M.render_motion(cs, prev, W, H, (f[:, 0].copy().view(np.int32), f[:, 1], f[:, 2], f[:, 3]))
    n = W * H
    went, left = c["count"] > 0, c["left"]
    last = c["last"]
    ids = last[:, 0].copy().view(np.int32).astype(np.int64)
    with np.errstate(all="ignore"):
        D = np.where(left, c["depth"], (c["depth"] + last[:, 1]).astype(F)).astype(F)
        Pv = (np.array(list(cam.position)[0:3], F) + (D[:, None] * c["d0"]).astype(F)).astype(F)
        m = went & ~left
        if m.any():
            i = ids[m]
            nrm = np.zeros((len(i), 3), F)
            sph = i < len(cs.spheres)
            if sph.any():
                P = segment_point(last[m][sph, 1], c["d"][m][sph], c["o"][m][sph])
                cur = np.asarray(cs.spheres, F)[i[sph]]
                nrm[sph] = ((P - cur[:, 0:3]).astype(F) * (F(1) / cur[:, 3])[:, None]).astype(F)
            u, v = last[m][:, 2], last[m][:, 3]
            arrays = [np.asarray(getattr(cs, k), F) if getattr(prev, k) is None else getattr(prev, k) for k in ("spheres", "quads", "vertices")]
            Xn = shape_points(cs, cs.spheres, cs.quads, cs.vertices, i, nrm, u, v)
            Xp = shape_points(cs, *arrays, i, nrm, u, v)
            dl = (Xp - Xn).astype(F)
            Mt = c["Mat"][m]
            Md = ((Mt[:, :, 0] * dl[:, 0:1]).astype(F) + (Mt[:, :, 1] * dl[:, 1:2]).astype(F)).astype(F) + (Mt[:, :, 2] * dl[:, 2:3]).astype(F)
            Pv[m] = (Pv[m] + Md.astype(F)).astype(F)
    word = np.where(left, np.int64(LEFT), ids)
    rec = M.project_points(prev.camera, Pv.reshape(H, W, 3), went.reshape(H, W), W, H, word.reshape(H, W))
    out = np.where(went.reshape(H, W, 1), rec.view(U), base.view(U)).view(F)
    assert n == len(went)
    if detail:
        return out, dict(c, D=D.reshape(H, W), went=went.reshape(H, W))
    return out


def ids_of(m):
    return np.ascontiguousarray(m, F).view(U)[..., 3]
