"""The reference of hj_denoise_frame_temporal: include/hijiki_hip.h's contract restated in numpy float32, in the written operation
order, over whole-image arrays.  The shared stages - prepare, slope, the spatial variance, the iteration - are denoise_ref's.  The
camera direction is the oracle's camera_rays (what test_aov_gpu.py holds the device's camera_ray to); dot3 and cross3 inside the
quaternion rotation - the only places where fmaf matters - are oracle.num_batch's, through closest_ref.  Shares no text with the
kernels: no tiles, no records - gathers of (H, W) arrays at the four tap positions."""
import math

import numpy as np

import denoise_ref as D
from closest_ref import cross3, dot3
from hijiki_amd import abi
from lightmap_filter_ref import inv_sq

U, F = np.uint32, np.float32
WORDS = abi.TEMPORAL_WORDS
VARIANCE_FRAMES = F(abi.TEMPORAL_VARIANCE_FRAMES)
DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, depth_tolerance=0.1, normal_cos=0.9, max_history=64, feedback=True)


def camera(position=(0, 0, 0), rotation=(0, 0, 0, 1), fov=60.0):
    c = abi.Camera()
    c.position[:], c.rotation[:], c.fov = [*position, 0.0], list(rotation), fov
    return c


def axis_angle(axis, degrees):
    """the unit quaternion (x, y, z, w) of a rotation about `axis`, rounded to float32"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2
    return [float(F(v)) for v in (*(a * math.sin(h)), math.cos(h))]


def tan_half(cam):
    return F(math.tan(float(F(0.5) * F(cam.fov)) * (3.14159265358979323846 / 180.0)))


def rotate(v, q):
    """quaternionRotate(v, q) in camera_ray's operation order; v (..., 3) float32, q four floats"""
    v = np.asarray(v, F)
    qv, qw = np.broadcast_to(np.array(q[0:3], F), v.shape), F(q[3])
    tw = qw * F(0) - dot3(qv, v)
    c1 = cross3(qv, v)
    t = (c1 + qv * F(0)) + v * qw
    cq = -qv
    c2 = cross3(t, cq)
    return ((c2 + t * qw) + cq * tw[..., None]).astype(F)


def directions(cam, W, H):
    """d of every pixel centre (H, W, 3): the oracle's camera ray through (x + 0.5, y + 0.5)"""
    from oracle import hj_oracle as oracle
    y, x = np.mgrid[0:H, 0:W]
    pix = np.stack([x.astype(F) + F(0.5), y.astype(F) + F(0.5)], -1).reshape(-1, 2)
    return oracle.camera_rays(cam, W, H, pix)[:, 3:6].reshape(H, W, 3).copy()


def project(cam, prev, z, W, H):
    """REPROJECT up to the tap positions -> front (c.z < 0), fx, fy, zp - (H, W) each - for the depths z"""
    Wf, Hf = F(W), F(H)
    d = directions(cam, W, H)
    P = (np.array(list(cam.position)[0:3], F) + z[..., None] * d).astype(F)
    v = (P - np.array(list(prev.position)[0:3], F)).astype(F)
    q = list(prev.rotation)
    c = rotate(v, [-F(q[0]), -F(q[1]), -F(q[2]), q[3]])
    with np.errstate(all="ignore"):
        k = (F(0.5) * Wf) / tan_half(prev)
        sx = (c[..., 0] / -c[..., 2]) * k + F(0.5) * Wf
        sy = (-c[..., 1] / -c[..., 2]) * k + F(0.5) * Hf
        zp = np.sqrt(D.sq(v))
    return c[..., 2] < 0, (sx - F(0.5)).astype(F), (sy - F(0.5)).astype(F), zp.astype(F)


def reproject(G, n, z, cam, prev, history, depth_tolerance, normal_cos):
    """-> has (H, W) bool, I_prev (H, W, 3), m1_prev, m2_prev, N_prev (H, W); zero where there is no history"""
    H, W = G.shape
    zero = np.zeros((H, W), F)
    if history is None:
        return np.zeros((H, W), bool), np.zeros((H, W, 3), F), zero, zero.copy(), zero.copy()
    history = np.asarray(history, F)
    valid = history.view(U)[..., 7] != 0
    front, fx, fy, zp = project(cam, prev, z, W, H)
    tol, ncos = F(depth_tolerance), F(normal_cos)
    with np.errstate(all="ignore"):
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


def accumulate(G, I_cur, has, I_prev, m1_prev, m2_prev, N_prev, alpha, alpha_moments, max_history):
    """-> I (H, W, 3), m1, m2, N (H, W) of the guided pixels (zero elsewhere)"""
    y1 = D.lum(I_cur)
    y2 = y1 * y1
    with np.errstate(all="ignore"):
        N = np.fmin(N_prev + F(1), F(max_history))
        a = np.fmax(F(alpha), F(1) / N)
        am = np.fmax(F(alpha_moments), F(1) / N)
        I = I_prev * (F(1) - a)[..., None] + I_cur * a[..., None]
        m1 = m1_prev * (F(1) - am) + y1 * am
        m2 = m2_prev * (F(1) - am) + y2 * am
    I, m1, m2, N = np.where(has[..., None], I, I_cur), np.where(has, m1, y1), np.where(has, m2, y2), np.where(has, N, F(1))
    off = ~G
    I[off], m1[off], m2[off], N[off] = 0, 0, 0, 0
    return I.astype(F), m1.astype(F), m2.astype(F), N.astype(F)


def run(beauty, aov, cam, prev, history=None, iterations=5, sigma_normal=0.5, sigma_depth=1.0, sigma_luminance=4.0, sigma_albedo=0.1, alpha=0.2,
        alpha_moments=0.2, depth_tolerance=0.1, normal_cos=0.9, max_history=64, feedback=True, keep=False):
    """-> (out (H, W, 4), history_out (H, W, 12)) of hj_denoise_frame_temporal; keep=True: a dict of the stages beside them"""
    G, c, A, I_cur, n, z = D.prepare(beauty, aov)
    has, I_prev, m1_prev, m2_prev, N_prev = reproject(G, n, z, cam, prev, history, depth_tolerance, normal_cos)
    I, m1, m2, N = accumulate(G, I_cur, has, I_prev, m1_prev, m2_prev, N_prev, alpha, alpha_moments, max_history)
    V = np.where(N < VARIANCE_FRAMES, D.variance(I, G), np.fmax(m2 - m1 * m1, F(0))).astype(F)
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
    hist = np.zeros(G.shape + (WORDS,), F)
    hist[G, 0:3], hist[G, 3], hist[G, 4], hist[G, 5], hist[G, 6], hist[G, 8:11] = I_hist[G], N[G], m1[G], m2[G], z[G], n[G]
    hist.view(U)[G, 7] = 1
    if keep:
        return out, hist, dict(G=G, has=has, I=I, m1=m1, m2=m2, N=N, V=V, I_cur=I_cur, A=A, n=n, z=z)
    return out, hist
