"""The reference of hj_filter_lightmap: include/hijiki_hip.h's contract restated in numpy float32, in the written operation order -
whole-image arrays shifted against each other, one tap at a time in (dy, dx) order, every operation on np.float32 arrays (numpy has
no fused multiply-add).  exp is the oracle's (oracle.num_batch("exp"): test_num_gpu.py pins the device's hj_exp to it).  Shares no
text with the kernels: no tiles, no lattice, no guide records - a boolean map and two (H, W, 3) arrays."""
import numpy as np

U, F = np.uint32, np.float32
K = (F(0.375), F(0.25), F(0.0625))


def hj_exp(x):
    """the numeric contract's exp over a float32 array of any shape"""
    from oracle import hj_oracle as oracle
    flat = np.ascontiguousarray(x, F).ravel()
    out = np.zeros(flat.shape, F)
    for i in range(0, len(flat), 1 << 20):
        out[i:i + (1 << 20)] = oracle.num_batch("exp", flat[i:i + (1 << 20)].view(U))[:, 0].copy().view(F)
    return out.reshape(np.shape(x))


def inv_sq(sigma):
    sigma = F(sigma)
    return F(1.0) / (sigma * sigma) if sigma > 0 else F(0.0)


def sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def guides(points, W, H):
    """points (count, 8) -> guided (H, W) bool, P (H, W, 3), N (H, W, 3); a point whose word 7 names no texel is skipped"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 8)
    t = pts.view(U)[:, 7].astype(np.int64)
    ok = t < W * H
    G, P, N = np.zeros(W * H, bool), np.zeros((W * H, 3), F), np.zeros((W * H, 3), F)
    G[t[ok]], P[t[ok]], N[t[ok]] = True, pts[ok, 0:3], pts[ok, 3:6]
    return G.reshape(H, W), P.reshape(H, W, 3), N.reshape(H, W, 3)


def iteration(img, G, P, N, s, ip, in_, ic):
    """one iteration at the step s: (H, W, 4) -> (H, W, 4)"""
    H, W = G.shape
    c = img[:, :, 0:3]
    total, wsum = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                oy, ox = dy * s, dx * s
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue                                            # every tap of this offset lies outside the atlas
                d, q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                on = G[d] & G[q]
                h = K[abs(dx)] * K[abs(dy)]
                sub_t, sub_w = total[d], wsum[d]                        # (views)
                if on.all():                                            # (the same operations on the slices themselves: no copies)
                    a = (sq(P[q] - P[d]) * ip + sq(N[q] - N[d]) * in_) + sq(c[q] - c[d]) * ic
                    w = h * hj_exp(-a)
                    sub_t[...] = sub_t + c[q] * w[:, :, None]
                    sub_w[...] = sub_w + w
                    continue
                a = (sq(P[q][on] - P[d][on]) * ip + sq(N[q][on] - N[d][on]) * in_) + sq(c[q][on] - c[d][on]) * ic
                w = h * hj_exp(-a)
                sub_t[on] = sub_t[on] + c[q][on] * w[:, None]
                sub_w[on] = sub_w[on] + w
        out = img.copy()
        out[G, 0:3] = (total / wsum[:, :, None])[G]
    return out


def run(image, points, iterations, sigma_position, sigma_normal, sigma_color=0.0, keep=False):
    """-> the filtered (H, W, 4) float32 image; keep=True: the list of the images after every iteration"""
    img = np.array(image, F)
    H, W, _ = img.shape
    G, P, N = guides(points, W, H)
    ip, in_, ic = inv_sq(sigma_position), inv_sq(sigma_normal), inv_sq(sigma_color)
    steps = []
    for i in range(int(iterations)):
        img = iteration(img, G, P, N, 1 << i, ip, in_, ic)
        ic = ic * F(4.0)
        steps.append(img)
    return steps if keep else img
