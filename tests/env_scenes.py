"""Environment lighting (DESIGN.md "Environment lighting") restated in numpy: the sampling distribution's cell weights, the
probabilities an alias table gives its cells, the lookup Le(d) from the oracle's hjo_atan2 / hjo_texture_lookup in float32, the
next-event sample from hjo_sincos2pi and numpy float32; and the environment-lit scenes the oracle and GPU tests share."""
import numpy as np

import scenes
from hijiki_amd import abi, host

F = np.float32
TWO_PI_INV = F(1.0) / F(6.28318530717958647692)      # (1.0f / kTwoPi) in float32
INV_PI = F(1.0) / F(3.14159265358979323846)          # kInvPi


def solid_angles(H, W):
    """(H, W) exact solid angle of every texel cell: (2 pi / W) (sin lat1 - sin lat0), row 0 at the top (+y)."""
    y = np.arange(H, dtype=np.float64)
    s1, s0 = np.sin(np.pi * (0.5 - y / H)), np.sin(np.pi * (0.5 - (y + 1) / H))
    return np.repeat(((2 * np.pi / W) * (s1 - s0))[:, None], W, axis=1)


def weights(texels, scale, filt):
    """(H, W) cell weights: max(r, g, b) of scale * texel (at least 0; bilinear: max over the 3 x 3 wrapped neighbours) x solid angle."""
    t = np.asarray(texels, np.float64)[..., :3] * np.asarray(scale, np.float64)
    m = np.maximum(t.max(axis=-1), 0.0)
    if filt == abi.TEX_BILINEAR:
        m = np.max([np.roll(np.roll(m, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    H, W = m.shape
    return m * solid_angles(H, W)


def alias_probabilities(alias_prob, alias):
    """The probability an alias table (threshold, alias cell per column) gives every cell, in float64."""
    q = np.asarray(alias_prob, np.float64).ravel()
    a = np.asarray(alias).ravel()
    p = q.copy()
    np.add.at(p, a, 1.0 - q)
    p -= np.where(a == np.arange(len(a)), 1.0 - q, 0.0)      # (a column that keeps itself gives nothing away)
    return (p / len(q)).reshape(np.shape(alias_prob))


def env_uv(oracle, dirs):
    """(n, 2) float32 (u, v) of directions, as the device computes them (no contraction)."""
    d = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    at = oracle.lib().hjo_atan2
    a1 = np.array([at(float(z), float(x)) for x, z in zip(d[:, 0], d[:, 2])], F)
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2])
    a2 = np.array([at(float(y), float(rr)) for y, rr in zip(d[:, 1], r)], F)
    with np.errstate(invalid="ignore"):
        u = F(0.5) + a1 * TWO_PI_INV
        v = F(0.5) + a2 * INV_PI
    u = np.where(np.isnan(u), F(0.0), u)
    return np.stack([u, v], 1).astype(F)


def lookup(oracle, texture_set, texture, scale, dirs):
    """Le(d) = scale * texture_rgb(env, u, v) in float32."""
    rgb = oracle.texture_lookup(texture_set, texture, env_uv(oracle, dirs))
    return (np.asarray(scale, F)[None, :] * rgb).astype(F)


def sky_texels(H=32, W=64, sun=None, sun_rgb=(400.0, 380.0, 300.0)):
    """A sky gradient (bright at the zenith, dim at the horizon, dark ground) with one bright sun texel (default: row H / 6, column
    W / 3)."""
    sun = (H // 6, W // 3) if sun is None else sun
    y = (np.arange(H) + 0.5) / H
    t = np.zeros((H, W, 4), F)
    up = y < 0.5
    t[up, :, 0] = (0.2 + 0.8 * (0.5 - y[up]))[:, None]
    t[up, :, 1] = (0.3 + 0.9 * (0.5 - y[up]))[:, None]
    t[up, :, 2] = (0.6 + 1.0 * (0.5 - y[up]))[:, None]
    t[~up, :, :3] = 0.05
    t[sun[0], sun[1], :3] = sun_rgb
    return t


def random_env(rng, H, W, zeros=0.3):
    """Random texels in [0, 4), a share of them zero, one channel negative, the middle one surely bright."""
    t = rng.uniform(0.0, 4.0, (H, W, 4)).astype(F)
    t[rng.uniform(size=(H, W)) < zeros, :3] = 0.0
    t[0, 0, 0] = -1.0
    t[H // 2, W // 2, 1] = 2.0
    return t


def env_only_scene(texels, filt=abi.TEX_NEAREST, scale=(1.0, 1.0, 1.0)):
    """Two small diffuse spheres BEHIND the camera (a tree needs two shapes): every camera ray misses.  No emitters, so select_prob
    is 1."""
    s = host.Scene()
    s.set_camera((0.0, 1.0, 3.0), (0.0, 0.0, 0.0, 1.0), 60.0)
    m = s.add_diffuse((0.5, 0.5, 0.5))
    s.add_sphere((0.0, 1.0, 5.0), 0.25, m)
    s.add_sphere((0.5, 1.0, 5.5), 0.25, m)
    t = s.add_texture(texels, filt)
    s.set_environment(t, scale)
    return s


# ------------------------------------------------------------------ the next-event sample, restated

def rng_next(s):
    """xorshift32 on a uint32 array -> the new states (= the draws)."""
    s = s ^ (s << np.uint32(13))
    s = s ^ (s >> np.uint32(17))
    return s ^ (s << np.uint32(5))


def sincos2pi(oracle, v):
    """(sin, cos)(2 pi v) by hjo_sincos2pi for a float32 array (evaluated once per distinct value)."""
    import ctypes as C
    f = oracle.lib().hjo_sincos2pi
    uniq, inv = np.unique(np.ascontiguousarray(v, F).view(np.uint32), return_inverse=True)
    out = np.zeros((len(uniq), 2), F)
    buf = (C.c_float * 2)()
    for k, x in enumerate(uniq.view(F)):
        f(float(x), buf)
        out[k] = buf[0], buf[1]
    return out[inv, 0], out[inv, 1]


def sample(oracle, cs, table, states, env=None):
    """DESIGN.md's environment sample for the uint32 RNG `states`, as hj_debug_env_sample / hjo_env_sample lay it out: (n, 8) =
    direction, pdf, cell, Le / pdf.  coin = float(draw 1) * 2^-32 (selection probability 1), a = draw 2, b = draw 3; the three
    sincos by hjo_sincos2pi, the lookup by `lookup`, everything else numpy float32."""
    env = cs.environment if env is None else env
    rec = cs.texture_set.textures[env.texture]
    W, H = int(rec.width), int(rec.height)
    table = np.ascontiguousarray(table, F).reshape(-1, 4)
    s1 = rng_next(np.ascontiguousarray(states, np.uint32))
    a = rng_next(s1)
    b = rng_next(a)
    coin = s1.astype(F) * F(1.0 / 4294967296.0)
    col = ((a.astype(np.uint64) * np.uint64(W * H)) >> np.uint64(32)).astype(np.int64)
    take = coin >= table[col, 0]
    cell = np.where(take, table[col, 1].copy().view(np.uint32).astype(np.int64), col)
    pdf = np.where(take, table[col, 3], table[col, 2]).astype(F)
    x, y = (cell % W).astype(F), (cell // W)
    fu = ((b >> np.uint32(16)).astype(F) + F(0.5)) * F(1.0 / 65536.0)
    fv = ((b & np.uint32(0xFFFF)).astype(F) + F(0.5)) * F(1.0 / 65536.0)
    sp, cp = sincos2pi(oracle, (x + fu) / F(W) - F(0.5))
    _, y0 = sincos2pi(oracle, y.astype(F) / F(2 * H))
    _, y1 = sincos2pi(oracle, (y + 1).astype(F) / F(2 * H))
    ys = y1 + fv * (y0 - y1)
    rr = np.sqrt(np.maximum(F(0.0), F(1.0) - ys * ys))
    d = np.stack([rr * cp, ys, rr * sp], 1).astype(F)
    le = lookup(oracle, cs.texture_set, env.texture, [env.scale[k] for k in range(3)], d)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = le * (F(1.0) / pdf)[:, None]
    return np.concatenate([d, pdf[:, None], cell.astype(F)[:, None], w], 1).astype(F)


def threshold_states(table, W, H, count=64):
    """RNG states whose coin equals their column's threshold EXACTLY (where `>=` and `>` part), found by running xorshift32
    backwards from the wanted first draw: thresholds t = k * 2^-32-representable floats with 0 < t < 1, column from draw 2."""
    def unshift_l(x, k):
        r = x
        for _ in range(32 // k + 1):
            r = x ^ ((r << k) & 0xFFFFFFFF)
        return r

    def unshift_r(x, k):
        r = x
        for _ in range(32 // k + 1):
            r = x ^ (r >> k)
        return r

    table = np.ascontiguousarray(table, F).reshape(-1, 4)
    out = []
    for col in np.nonzero((table[:, 0] > 0) & (table[:, 0] < 1))[0]:
        first = int(np.float64(table[col, 0]) * 4294967296.0)        # a uint32 whose float conversion may be the threshold
        for draw in range(max(first - 300, 1), first + 300):          # (float32 keeps 24 bits: many draws convert to it)
            if np.uint32(draw).astype(F) * F(1.0 / 4294967296.0) != table[col, 0]:
                continue
            a = int(rng_next(np.array([draw], np.uint32))[0])
            if (a * W * H) >> 32 == col:
                out.append(unshift_l(unshift_r(unshift_l(draw, 5), 17), 13))
                break
        if len(out) >= count:
            break
    return np.array(out, np.uint32)


def states_with_draws(first=None, second=None, third=None):
    """An RNG state whose draw 1 / 2 / 3 is the given uint32 (one of them)."""
    def unshift_l(x, k):
        r = x
        for _ in range(32 // k + 1):
            r = x ^ ((r << k) & 0xFFFFFFFF)
        return r

    def unshift_r(x, k):
        r = x
        for _ in range(32 // k + 1):
            r = x ^ (r >> k)
        return r

    def back(x):
        return unshift_l(unshift_r(unshift_l(x, 5), 17), 13)
    if first is not None:
        return back(first)
    if second is not None:
        return back(back(second))
    return back(back(back(third)))


# ------------------------------------------------------------------ scenes under an environment

def mixed_scene(tinted=False, select_prob=None):
    """cbox with its mirror and glass spheres, diffuse walls and area light, a textured quad, under a bilinear sky (select_prob 0.5).
    tinted: an OPEN scene instead - floor, one side wall, the area light, a mirror sphere and a sphere of tinted glass whose
    extinction has a zero channel - so that paths leave the scene straight from the glass."""
    rng = np.random.default_rng(2)
    tex = rng.uniform(0.1, 0.9, (5, 7, 4)).astype(F)
    if not tinted:
        s = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES)
        m = s.add_diffuse_textured(s.add_texture(tex, abi.TEX_BILINEAR))
        s.add_quad((-0.6, 0.2, 0.4), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0), m)
        s.set_environment(s.add_texture(sky_texels(16, 32), abi.TEX_BILINEAR), 2.0, select_prob)
        return s.compile()
    s = host.Scene()
    s.set_camera_cbox()
    m = s.add_diffuse_textured(s.add_texture(tex, abi.TEX_BILINEAR))
    s.add_quad((-1.2, 0, 1.2), (2.4, 0, 0), (0, 0, -2.4), s.add_diffuse((0.7, 0.7, 0.7)))
    s.add_quad((-1.2, 0, 1.2), (0, 0, -2.4), (0, 2.0, 0), s.add_diffuse((0.6, 0.1, 0.1)))
    s.add_quad((-0.4, 1.99, -0.4), (0.8, 0, 0), (0, 0, 0.8), s.add_emissive((15.0, 14.0, 12.0)))
    s.add_quad((0.3, 0.0, -0.9), (0.6, 0.0, 0.0), (0.0, 0.6, 0.0), m)
    s.add_sphere((-0.45, 0.4, -0.2), 0.4, s.add_mirror())
    s.add_sphere((0.45, 0.45, 0.3), 0.45, s.add_dielectric(1.5, extinction=(0.5, 0.0, 3.0)))
    s.set_environment(s.add_texture(sky_texels(16, 32), abi.TEX_BILINEAR), 2.0, select_prob)
    return s.compile()


def analytic_sky_scene(tex, rho=(0.5, 0.6, 0.7)):
    """An upward diffuse quad of albedo rho filling a downward camera's frame (and a small sphere far below: a tree needs two
    shapes) under the nearest sky `tex`; no emitters, so select_prob is 1."""
    s = host.Scene()
    s.set_camera((0.0, 1.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)     # looking down -y
    s.add_quad((-5.0, 0.0, -5.0), (0.0, 0.0, 10.0), (10.0, 0.0, 0.0), s.add_diffuse(tuple(rho)))   # edge1 x edge2 = +y
    s.add_sphere((0.0, -50.0, 0.0), 0.1, s.add_diffuse((0.5, 0.5, 0.5)))
    s.set_environment(s.add_texture(tex, abi.TEX_NEAREST))
    return s.compile()


def analytic_sky_expectation(tex, rho=(0.5, 0.6, 0.7)):
    """rho / pi * sum over the upper cells of L * dphi * (y1^2 - y0^2) / 2: what every pixel of analytic_sky_scene expects."""
    H, W = tex.shape[:2]
    y = np.sin(np.pi * (0.5 - np.arange(H + 1) / H))                               # sin(latitude) of the row edges
    cosw = (2 * np.pi / W) * (y[:-1] ** 2 - y[1:] ** 2) / 2                          # integral of cos over a cell, per row
    up = np.arange(H) < H // 2
    return np.asarray(rho) / np.pi * (tex[up, :, :3].astype(np.float64) * cosw[up, None, None]).sum((0, 1))


def cluster_scene(texels=None, filt=abi.TEX_BILINEAR, scale=(1.0, 1.0, 1.0), select_prob=None, light=False):
    """A cluster of spheres (diffuse, checkerboard, mirror, clear glass) on a ground quad under the open sky; no emitters unless
    `light` (a quad light above the cluster)."""
    s = host.Scene()
    s.set_camera((0.0, 0.9, 3.2), (-0.1, 0.0, 0.0, 0.995), 38.0)
    s.add_quad((-4.0, 0.0, 4.0), (8.0, 0.0, 0.0), (0.0, 0.0, -8.0), s.add_diffuse((0.6, 0.6, 0.55)))
    mats = [s.add_diffuse((0.7, 0.3, 0.2)), s.add_diffuse_cboard((0.9, 0.9, 0.2), 0.13, (0.1, 0.2, 0.8), 0.21), s.add_mirror(),
            s.add_dielectric(1.5), s.add_diffuse((0.2, 0.5, 0.7))]
    rng = np.random.default_rng(4)
    for k in range(9):
        rad = float(rng.uniform(0.15, 0.35))
        s.add_sphere((float(rng.uniform(-1.0, 1.0)), rad, float(rng.uniform(-1.0, 1.0))), rad, mats[k % len(mats)])
    if light:
        s.add_quad((-0.4, 1.8, -0.4), (0.8, 0, 0), (0, 0, 0.8), s.add_emissive((10.0, 9.0, 8.0)))
    texels = sky_texels(16, 32) if texels is None else texels
    s.set_environment(s.add_texture(np.asarray(texels, F), filt), scale, select_prob)
    return s.compile()


def random_scene_with_env(seed, select_prob, filt=abi.TEX_BILINEAR):
    """scenes.random_scene plus a sphere light and a triangle light (so that all three shape kinds emit) and a random sky."""
    s = scenes.random_scene_builder(seed)
    rng = np.random.default_rng(300 + seed)
    s.add_sphere((0.5, 1.5, 0.4), 0.1, s.add_emissive((9.0, 12.0, 14.0)))
    pos = np.array([[-0.9, 1.6, -0.8], [-0.5, 1.6, -0.8], [-0.7, 1.9, -0.5]], F)
    b = s.add_vertices(pos, np.tile(np.array([[0, -0.6, 0.8]], F), (3, 1)), np.zeros((3, 2), F))
    s.add_triangle(b, b + 1, b + 2, s.add_emissive((14.0, 6.0, 6.0)))
    s.set_environment(s.add_texture(random_env(rng, 9, 13), filt), (1.5, 1.0, 0.75), select_prob)
    return s.compile()


def uniform_sky_sphere_scene(L=1.5, rho=0.6):
    """A convex diffuse sphere of albedo rho under a uniform sky of radiance L, nothing else to see (a second tiny sphere far
    behind the camera: a tree needs two shapes): the sphere is rho * L, the background L."""
    s = host.Scene()
    s.set_camera((0.0, 0.0, 2.5), (0.0, 0.0, 0.0, 1.0), 40.0)
    s.add_sphere((0.0, 0.0, 0.0), 0.6, s.add_diffuse((rho,) * 3))
    s.add_sphere((0.0, 0.0, 500.0), 0.01, s.add_diffuse((0.5, 0.5, 0.5)))
    s.set_environment(s.add_texture(np.full((4, 8, 4), L, F), abi.TEX_NEAREST))
    return s.compile()


def ray_log_premises(cs, log):
    """What a frame's ray log (oracle.logged_rays) says about the environment code it exercised: counts of environment shadow rays
    and of the unoccluded ones, of camera rays that miss, of misses straight after a mirror or glass bounce, of those after a glass
    bounce of non-zero extinction (the ray leaves a convex glass body with its extinction set), and of
    misses after a diffuse bounce (which add nothing)."""
    mats = np.asarray(cs.materials)
    kind, hit, em = log[:, 8], log[:, 9].astype(np.int64), log[:, 10]
    env_sh = (kind == 1) & (em == 8)
    c = np.nonzero(kind == 0)[0]                              # the closest-hit rays, in path order
    chit, camera = hit[c], log[c, 6] == F(1e-4)
    prev_tag = np.full(len(c), -1, np.int64)
    prev_tag[1:] = np.where(chit[:-1] >= 0, mats[np.maximum(chit[:-1], 0)] >> 24, -1)
    prev_mat = np.zeros(len(c), np.int64)
    prev_mat[1:] = np.where(chit[:-1] >= 0, mats[np.maximum(chit[:-1], 0)] & 0xFFFFFF, 0)
    miss = (chit < 0) & ~camera
    tinted = np.zeros(len(c), bool)
    d = cs.desc
    for k in np.nonzero(miss & (prev_tag == abi.MAT_DIELECTRIC))[0]:
        tinted[k] = any(d.dielectric[int(prev_mat[k])].extinction[j] != 0.0 for j in range(3))
    return {"env_shadow": int(env_sh.sum()), "env_shadow_free": int((env_sh & (log[:, 9] < 0)).sum()),
            "area_shadow": int(((kind == 1) & (em != 8)).sum()), "camera_misses": int(((chit < 0) & camera).sum()),
            "discrete_misses": int((miss & ((prev_tag == abi.MAT_MIRROR) | (prev_tag == abi.MAT_DIELECTRIC))).sum()),
            "tinted_misses": int(tinted.sum()),
            "diffuse_misses": int((miss & np.isin(prev_tag, (abi.MAT_DIFFUSE, abi.MAT_DIFFUSECBOARD, abi.MAT_DIFFUSE_TEXTURED))).sum())}
