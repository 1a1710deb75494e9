"""The reference of hj_render_motion and hj_denoise_frame_temporal_motion: include/hijiki_hip.h's two contracts restated in numpy
float32, in the written operation order, over whole-image arrays.  The camera direction, rotate, tan and the accumulate stage are
temporal_ref's; dot3 and cross3 - inside rotate - are oracle.num_batch's through closest_ref, and so is the hit point's fmaf (a dot3
with a zero term).  The taps of REPROJECT are written once more here, from the header, because temporal_ref.reproject computes
its own (sx, sy, zp): test_motion_host.py holds the two texts to each other word for word.  Shares no text with the kernels: no
walk, no tiles - the raw hits (id, t, u, v) come in as an array, from hj_trace_rays where a test is about the resolve, from the
oracle's first hit where it is about the whole call."""
import ctypes as C

import numpy as np

import denoise_ref as D
import temporal_ref as T
from closest_ref import dot3
from hijiki_amd import abi
from lightmap_filter_ref import inv_sq

U, F = np.uint32, np.float32
NONE = abi.MOTION_NONE
KEPS = F(1e-4)


class Prev:
    """How a scene stood in the previous frame, in the form Renderer.render_motion takes: .desc with the camera, the three shape
    arrays (None: that kind did not move) and the counts of `cs`"""

    def __init__(self, cs, camera, spheres=None, quads=None, vertices=None):
        self.camera = camera
        self.spheres = None if spheres is None else np.ascontiguousarray(spheres, F).reshape(-1, 4)
        self.quads = None if quads is None else np.ascontiguousarray(quads, F).reshape(-1, 12)
        self.vertices = None if vertices is None else np.ascontiguousarray(vertices, F).reshape(-1, 8)
        d = abi.SceneDesc()
        d.camera = camera
        d.num_spheres, d.num_quads, d.num_vertices = len(cs.spheres), len(cs.quads), len(cs.vertices)
        for name, a, rec in (("spheres", self.spheres, abi.Sphere), ("quads", self.quads, abi.Quad), ("vertices", self.vertices, abi.Vertex)):
            if a is not None and len(a):
                assert len(a) == getattr(d, "num_" + name)
                setattr(d, name, C.cast(C.c_void_p(a.ctypes.data), C.POINTER(rec)))
        self.desc = d


def centre_rays(camera, W, H):
    """(H * W, 8): origin, d of the pixel centres (x + 0.5, y + 0.5), tMin = eps, tMax = +inf - the rays of hj_render_motion"""
    rays = np.zeros((H * W, 8), F)
    rays[:, 0:3] = np.array(list(camera.position)[0:3], F)
    rays[:, 3:6] = T.directions(camera, W, H).reshape(-1, 3)
    rays[:, 6], rays[:, 7] = KEPS, np.inf
    return rays


def hit_point(t, d, o):
    """fma(t, d, o) per channel: dot3((o, 0, t), (1, 0, d)) = fma(t, d, fma(0, 0, o * 1))"""
    out = np.zeros(d.shape, F)
    one, zero = np.ones_like(t), np.zeros_like(t)
    for k in range(3):
        ok = np.broadcast_to(F(o[k]), t.shape)
        out[..., k] = dot3(np.stack([ok, zero, t], -1), np.stack([one, zero, d[..., k]], -1))
    return out


def previous_points(cs, camera, prev, W, H, ids, t, u, v):
    """PREVIOUS POINT: Pp (H, W, 3) and which pixels hit a shape; ids, t, u, v (H, W) raw hits; cs holds the CURRENT arrays"""
    ns, nq, nt = len(cs.spheres), len(cs.quads), len(cs.triangles)
    ids = ids.astype(np.int64)
    hit = (ids >= 0) & (ids < ns + nq + nt)
    Pp = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        m = hit & (ids < ns)
        if m.any():
            d = T.directions(camera, W, H)[m]
            P = hit_point(t[m], d, np.array(list(camera.position)[0:3], F))
            cur = np.asarray(cs.spheres, F)[ids[m]]
            was = (np.asarray(cs.spheres, F) if prev.spheres is None else prev.spheres)[ids[m]]
            r = F(1) / cur[:, 3]
            n = ((P - cur[:, 0:3]).astype(F) * r[:, None]).astype(F)
            Pp[m] = was[:, 0:3] + (n * was[:, 3:4]).astype(F)
        m = hit & (ids >= ns) & (ids < ns + nq)
        if m.any():
            q = (np.asarray(cs.quads, F) if prev.quads is None else prev.quads)[ids[m] - ns]
            uu, vv = u[m][:, None], v[m][:, None]
            Pp[m] = (q[:, 0:3] + (q[:, 4:7] * uu).astype(F)).astype(F) + (q[:, 8:11] * vv).astype(F)
        m = hit & (ids >= ns + nq)
        if m.any():
            tri = np.asarray(cs.triangles).astype(np.int64)[ids[m] - ns - nq]
            vert = (np.asarray(cs.vertices, F) if prev.vertices is None else prev.vertices)[:, 0:3]
            a, b, c = vert[tri[:, 0]], vert[tri[:, 1]], vert[tri[:, 2]]
            uu, vv = u[m][:, None], v[m][:, None]
            l0 = ((F(1) - uu).astype(F) - vv).astype(F)
            Pp[m] = ((a * l0).astype(F) + (b * uu).astype(F)).astype(F) + (c * vv).astype(F)
    return Pp.astype(F), hit


def project_points(prev_camera, Pp, hit, W, H, ids):
    """PROJECTION -> (H, W, 4) records"""
    Wf, Hf = F(W), F(H)
    vv = (Pp - np.array(list(prev_camera.position)[0:3], F)).astype(F)
    q = list(prev_camera.rotation)
    c = T.rotate(vv, [-F(q[0]), -F(q[1]), -F(q[2]), q[3]])
    out = np.zeros((H, W, 4), F)
    with np.errstate(all="ignore"):
        k = (F(0.5) * Wf) / T.tan_half(prev_camera)
        out[..., 0] = (c[..., 0] / -c[..., 2]) * k + F(0.5) * Wf
        out[..., 1] = (-c[..., 1] / -c[..., 2]) * k + F(0.5) * Hf
        out[..., 2] = np.sqrt(D.sq(vv))
    out.view(U)[..., 3] = ids.astype(np.int64) & 0xFFFFFFFF
    none = ~(hit & (c[..., 2] < 0))
    out[none] = 0
    out.view(U)[none, 3] = NONE
    return out


def render_motion(cs, prev, W, H, hits):
    """hj_render_motion's (H, W, 4) for the uploaded scene cs (its camera and CURRENT arrays) and the previous state `prev` (a Prev);
    hits = (ids, t, u, v) of the centre rays, (H * W,) each"""
    ids, t, u, v = (np.asarray(a).reshape(H, W) for a in hits)
    cam = cs.desc.camera
    Pp, hit = previous_points(cs, cam, prev, W, H, ids.astype(np.int32), t.astype(F), u.astype(F), v.astype(F))
    return project_points(prev.camera, Pp, hit, W, H, ids.astype(np.int32))


def static_motion(cam, prev, z, W, H, ids=0):
    """the static projection's own (sx, sy, zp) as a motion image: what hj_denoise_frame_temporal computes for the depths z"""
    Wf, Hf = F(W), F(H)
    d = T.directions(cam, W, H)
    P = (np.array(list(cam.position)[0:3], F) + z[..., None] * d).astype(F)
    v = (P - np.array(list(prev.position)[0:3], F)).astype(F)
    q = list(prev.rotation)
    c = T.rotate(v, [-F(q[0]), -F(q[1]), -F(q[2]), q[3]])
    out = np.zeros((H, W, 4), F)
    with np.errstate(all="ignore"):
        k = (F(0.5) * Wf) / T.tan_half(prev)
        out[..., 0] = (c[..., 0] / -c[..., 2]) * k + F(0.5) * Wf
        out[..., 1] = (-c[..., 1] / -c[..., 2]) * k + F(0.5) * Hf
        out[..., 2] = np.sqrt(D.sq(v))
    out.view(U)[..., 3] = ids
    none = ~(c[..., 2] < 0)
    out[none] = 0
    out.view(U)[none, 3] = NONE
    return out


def reproject(G, n, motion, history, depth_tolerance, normal_cos):
    """REPROJECT through a motion image -> has, I_prev, m1_prev, m2_prev, N_prev as temporal_ref.reproject gives them"""
    H, W = G.shape
    zero = np.zeros((H, W), F)
    if history is None:
        return np.zeros((H, W), bool), np.zeros((H, W, 3), F), zero, zero.copy(), zero.copy()
    history, motion = np.asarray(history, F), np.asarray(motion, F)
    valid = history.view(U)[..., 7] != 0
    front = motion.view(U)[..., 3] != NONE
    sx, sy, zp = motion[..., 0], motion[..., 1], motion[..., 2]
    tol, ncos = F(depth_tolerance), F(normal_cos)
    with np.errstate(all="ignore"):
        fx, fy = (sx - F(0.5)).astype(F), (sy - F(0.5)).astype(F)
        ix, iy = np.floor(fx), np.floor(fy)
        tx, ty = fx - ix, fy - iy
        wx, wy = (F(1) - tx, tx), (F(1) - ty, ty)
        sums = [np.zeros((H, W), F) for _ in range(6)]                  # I.r, I.g, I.b, m1, m2, N
        ws = np.zeros((H, W), F)
        for b in (0, 1):
            for a in (0, 1):
                xx, yy = ix + F(a), iy + F(b)
                inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                on = G & front & inside
                xi, yi = np.where(on, xx, 0).astype(np.int64), np.where(on, yy, 0).astype(np.int64)
                h = history[yi, xi]
                on &= valid[yi, xi]
                on &= np.abs(h[..., 6] - zp) <= tol * zp
                hn = h[..., 8:11]
                on &= (hn[..., 0] * n[..., 0] + hn[..., 1] * n[..., 1]) + hn[..., 2] * n[..., 2] >= ncos
                w = wx[a] * wy[b]
                for s, word in zip(sums, (0, 1, 2, 4, 5, 3)):
                    s[on] = (s + h[..., word] * w)[on]
                ws[on] = (ws + w)[on]
        has = ws > 0
        out = [np.where(has, s / ws, F(0)).astype(F) for s in sums]
    return has, np.stack(out[0:3], -1), out[3], out[4], out[5]


def run(beauty, aov, motion, history=None, iterations=5, sigma_normal=0.5, sigma_depth=1.0, sigma_luminance=4.0, sigma_albedo=0.1, alpha=0.2,
        alpha_moments=0.2, depth_tolerance=0.1, normal_cos=0.9, max_history=64, feedback=True, keep=False):
    """-> (out (H, W, 4), history_out (H, W, 12)) of hj_denoise_frame_temporal_motion: temporal_ref.run with the motion form of step 2"""
    G, c, A, I_cur, n, z = D.prepare(beauty, aov)
    has, I_prev, m1_prev, m2_prev, N_prev = reproject(G, n, motion, history, depth_tolerance, normal_cos)
    I, m1, m2, N = T.accumulate(G, I_cur, has, I_prev, m1_prev, m2_prev, N_prev, alpha, alpha_moments, max_history)
    V = np.where(N < T.VARIANCE_FRAMES, D.variance(I, G), np.fmax(m2 - m1 * m1, F(0))).astype(F)
    V[~G] = 0
    gzx, gzy = D.slope(z, G, 1), D.slope(z, G, 0)
    img = np.concatenate([np.where(G[..., None], I, c), V[..., None]], 2).astype(F)
    inn, ia, sz, sl = inv_sq(sigma_normal), inv_sq(sigma_albedo), F(sigma_depth), F(sigma_luminance)
    I_hist = I
    for i in range(int(iterations)):
        img = D.iteration(img, G, n, z, A, gzx, gzy, 1 << i, inn, sz, sl, ia)
        if i == 0 and feedback:
            I_hist = img[..., 0:3]
    out = img.copy()
    out[G, 0:3] = (img[..., 0:3] * A)[G]
    hist = np.zeros(G.shape + (T.WORDS,), F)
    hist[G, 0:3], hist[G, 3], hist[G, 4], hist[G, 5], hist[G, 6], hist[G, 8:11] = I_hist[G], N[G], m1[G], m2[G], z[G], n[G]
    hist.view(U)[G, 7] = 1
    if keep:
        return out, hist, dict(G=G, has=has, N=N, z=z, n=n)
    return out, hist
