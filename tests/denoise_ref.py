"""The reference of hj_denoise_frame: include/hijiki_hip.h's contract restated in numpy float32, in the written operation order -
whole-image arrays shifted against each other, one tap at a time in (dy, dx) order, every operation on np.float32 arrays (numpy has
no fused multiply-add).  exp is lightmap_filter_ref's (the oracle's, to which test_num_gpu.py pins the device's hj_exp).  Shares no
text with the kernels: no tiles, no lattice, no guide records - a boolean map and a handful of (H, W[, 3]) arrays."""
import numpy as np

from lightmap_filter_ref import hj_exp, inv_sq

U, F = np.uint32, np.float32
K = (F(0.375), F(0.25), F(0.0625))
G3 = (F(0.25), F(0.125), F(0.0625))
FLOOR, EPS = F(0.015625), F(1e-6)


def sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _window(H, W, oy, ox):
    """the pixels p (slices d) whose neighbour q = p + (ox, oy) (slices q) lies in the image; None when there is none"""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def prepare(beauty, aov):
    """-> guided (H, W) bool, c, A, I, n (H, W, 3), z (H, W); what a pixel that is not guided never uses is zero"""
    beauty, aov = np.asarray(beauty, F), np.asarray(aov, F)
    S, Hc, bw = aov[..., 3], aov[..., 11], beauty[..., 3]
    H, W = S.shape
    lit = (aov[..., 8] > 0) | (aov[..., 9] > 0) | (aov[..., 10] > 0)
    near = np.zeros((H, W), bool)                                       # a lit pixel in the 5 x 5 window, the pixel itself included
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            w = _window(H, W, dy, dx)
            if w:
                near[w[0]] |= lit[w[1]]
    G = (Hc > 0) & (bw > 0) & ~near
    with np.errstate(all="ignore"):
        c = np.where((bw > 0)[..., None], beauty[..., 0:3] / bw[..., None], F(0))
        A = np.fmax(aov[..., 0:3] / S[..., None], FLOOR)
        I = c / A
        n = aov[..., 4:7] / Hc[..., None]
        z = aov[..., 7] / Hc
    off = ~G
    A[off], I[off], n[off], z[off] = 0, 0, 0, 0
    return G, c.astype(F), A.astype(F), I.astype(F), n.astype(F), z.astype(F)


def slope(z, G, axis):
    """the smaller of the forward and the backward difference along `axis`, among those whose neighbour is guided; a tie: forward"""
    H, W = G.shape
    f, b = np.zeros((H, W), F), np.zeros((H, W), F)
    has_f, has_b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    oy, ox = (1, 0) if axis == 0 else (0, 1)
    w = _window(H, W, oy, ox)
    if w:
        d, q = w
        f[d], has_f[d] = z[q] - z[d], G[q]
    w = _window(H, W, -oy, -ox)
    if w:
        d, q = w
        b[d], has_b[d] = z[d] - z[q], G[q]
    both = np.where(np.abs(b) < np.abs(f), b, f)
    return np.where(has_f & has_b, both, np.where(has_f, f, np.where(has_b, b, F(0)))).astype(F)


def variance(I, G):
    """the initial variance of the luminance of I over the guided pixels of the 5 x 5 window"""
    H, W = G.shape
    l = lum(I)
    m1, m2, cnt = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            w = _window(H, W, dy, dx)
            if not w:
                continue
            d, q = w
            on = G[d] & G[q]
            a, b, c = m1[d], m2[d], cnt[d]                              # (views)
            a[on] = a[on] + l[q][on]
            b[on] = b[on] + l[q][on] * l[q][on]
            c[on] = c[on] + F(1)
    with np.errstate(all="ignore"):
        mu = m1 / cnt
        V = np.fmax(m2 / cnt - mu * mu, F(0))
    V[~G] = 0
    return V.astype(F)


def iteration(img, G, n, z, A, gzx, gzy, s, inn, sz, sl, ia):
    """one iteration at the step s: (I, V) as (H, W, 4) -> (I', V')"""
    H, W = G.shape
    I, V = img[..., 0:3], img[..., 3]
    vsum, gsum = np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            w = _window(H, W, dy, dx)
            if not w:
                continue
            d, q = w
            on = G[d] & G[q]
            g = G3[abs(dx) + abs(dy)]
            a, b = vsum[d], gsum[d]
            a[on] = a[on] + V[q][on] * g
            b[on] = b[on] + g
    l = lum(I)
    total, vs, ws = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        sd = np.sqrt(vsum / gsum)
        dl = sl * sd + EPS
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                w = _window(H, W, dy * s, dx * s)
                if not w:
                    continue                                            # every tap of this offset lies outside the image
                d, q = w
                on = G[d] & G[q]
                if not on.any():
                    continue
                h = K[abs(dx)] * K[abs(dy)]
                en = sq(n[q][on] - n[d][on]) * inn
                ez = el = F(0)
                if sz != 0:
                    ez = np.abs(z[q][on] - z[d][on]) / (sz * np.abs(gzx[d][on] * F(dx * s) + gzy[d][on] * F(dy * s)) + EPS)
                if sl != 0:
                    el = np.abs(l[q][on] - l[d][on]) / dl[d][on]
                ea = sq(A[q][on] - A[d][on]) * ia
                wt = h * hj_exp(-(((en + ez) + el) + ea))
                t, a, b = total[d], vs[d], ws[d]
                t[on] = t[on] + I[q][on] * wt[:, None]
                a[on] = a[on] + V[q][on] * (wt * wt)
                b[on] = b[on] + wt
        out = img.copy()
        out[G, 0:3] = (total / ws[..., None])[G]
        out[G, 3] = (vs / (ws * ws))[G]
    return out


def run(beauty, aov, iterations=5, sigma_normal=0.5, sigma_depth=1.0, sigma_luminance=4.0, sigma_albedo=0.1, keep=False):
    """-> the (H, W, 4) float32 output of hj_denoise_frame; keep=True: the list of the outputs for 0, 1, ..., iterations iterations"""
    G, c, A, I, n, z = prepare(beauty, aov)
    gzx, gzy = slope(z, G, 1), slope(z, G, 0)
    img = np.concatenate([np.where(G[..., None], I, c), variance(I, G)[..., None]], 2).astype(F)
    inn, ia, sz, sl = inv_sq(sigma_normal), inv_sq(sigma_albedo), F(sigma_depth), F(sigma_luminance)

    def finish(x):
        out = x.copy()
        out[G, 0:3] = (x[..., 0:3] * A)[G]
        return out

    steps = [finish(img)]
    for i in range(int(iterations)):
        img = iteration(img, G, n, z, A, gzx, gzy, 1 << i, inn, sz, sl, ia)
        steps.append(finish(img))
    return steps if keep else steps[-1]
