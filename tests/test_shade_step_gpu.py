"""Step level: ONE pass of the shade stage (stage_shade through the split path's own kernel, hj_debug_shade_step) over fabricated
path states and raw hits against the step function the oracle's integrate_ray itself calls (hjo_shade_step), 0 differing bits over
every word of every output record, counters included.  One exception: a NaN float word equals any NaN.  No record is masked out.

Families (inputs(...) below): TRACED - random rays and the oracle's logged rays through oracle.intersect for real hits, crossed with
stratified throughput, extinction, bounce index and wasDiscrete; GEOMETRY - hits no walk was asked for but the stage defines (sphere
poles and meridian, a normal beyond +-1, triangle corners and edges, cancelling vertex normals, |n.x| == |n.y|, skewed quads,
direction lengths 1e-12 .. 1e12, zero components, t == 0); BRANCHES - records that sit on a comparison of the stage (cosI == 0, the
k == 0 transition, the Fresnel and roulette draws on their thresholds, the selection draw on every cdf step, a reference point equal
to or in the plane of the sampled point, the importance at kEps, the environment coin on select_prob, checkerboard arguments);
STRUCTURE - per-tag bin sizes around the wave size, several workgroups, both parities, one tag only, misses only; and the
light-shaft grid against the same scene without it.

The tests without the gpu mark assert, from the oracle alone, that the inputs are what they claim - every branch is taken - and that
hjo_shade_step chained with oracle.intersect reproduces hjo_integrate_block bit for bit: the step is the integrator's text and the
record layouts carry everything."""
import ctypes as C
import functools

import numpy as np
import pytest

import env_scenes
import fuzz_cases
from hijiki_amd import abi, device, host
from test_num_gpu import unxorshift, words

U, F = np.uint32, np.float32
IN, OUT = abi.STEP_IN_WORDS, abi.STEP_OUT_WORDS
INT_OUT = (0, 10, 11, 15)                                   # alive, flags, RNG state, shadow record present; the rest are floats
FLOAT_OUT = np.array([k not in INT_OUT for k in range(OUT)])
MAX_BOUNCES, RR_START = 12, 4
BOUNCES = (0, 1, RR_START - 1, RR_START, RR_START + 1, MAX_BOUNCES - 2, MAX_BOUNCES - 1)
TINT = (0.5, 1.5, 3.0)
KEPS = F(1e-4)


def opts(grid=False):
    o = abi.RenderOpts.default()
    o.max_bounces, o.rr_start = MAX_BOUNCES, RR_START
    if not grid:
        o.flags |= abi.RENDER_NO_LIGHT_GRID
    return o


def differing(a, b):
    """Words of (n, OUT) record arrays that differ; a NaN float word equals any NaN."""
    a, b = np.asarray(a, U), np.asarray(b, U)
    ne = a != b
    with np.errstate(invalid="ignore"):
        both_nan = np.isnan(a.view(F)) & np.isnan(b.view(F)) & FLOAT_OUT[None, :]
    return ne & ~both_nan


def report(name, rec, got, want):
    d = differing(got, want)
    if not d.any():
        return ""
    i = int(np.argmax(d.any(1)))
    return (f"{name}: {int(d.sum())} words of {int(d.any(1).sum())} records differ; first: record {i}, words {np.flatnonzero(d[i]).tolist()}\n"
            f"  in   {[hex(int(x)) for x in rec[i]]}\n  gpu  {[hex(int(x)) for x in got[i]]}\n  want {[hex(int(x)) for x in want[i]]}")


# ------------------------------------------------------------------------------------------------------------------- scenes

VARIANTS = ("rich", "env0", "env1", "many", "dark")


@functools.lru_cache(maxsize=None)
def scene(variant):
    """A few dozen shapes: quads, spheres and triangles of all six material tags (nearest and bilinear textures), clear glass of
    eta 1.5, 1 / 1.5 and 1 on power-of-two quads (their normal is exactly +y), a skewed quad, triangles whose vertex normals cancel
    or have |n.x| == |n.y|, a checkerboard with scale 0.
      rich: emissive sphere, quad and triangle, a tinted dielectric, an environment picked with probability 0.5
      env0 / env1: the same under select_prob 0 / 1
      many: eleven quad lights (more than the light-shaft grid's eight), the first one facing -x exactly; no environment
      dark: no emitter, no environment, no tinted glass (the stage then carries no extinction)"""
    rng = np.random.default_rng(17)
    s = host.Scene()
    s.set_camera((0.05, 0.9, 3.3), (-0.02, 0.01, 0.0, 0.9997), 38.0)
    white, red = s.add_diffuse((0.7, 0.7, 0.7)), s.add_diffuse((0.6, 0.1, 0.1))
    cb = s.add_diffuse_cboard((0.9, 0.9, 0.2), 0.13, (0.1, 0.2, 0.8), 0.21)
    cb0 = s.add_diffuse_cboard((0.3, 0.9, 0.2), 0.0, (0.8, 0.2, 0.1), 0.25)
    tn = s.add_diffuse_textured(s.add_texture(rng.uniform(0.1, 0.9, (5, 7, 4)).astype(F), abi.TEX_NEAREST))
    tb = s.add_diffuse_textured(s.add_texture(rng.uniform(0.1, 0.9, (6, 3, 4)).astype(F), abi.TEX_BILINEAR))
    mirror = s.add_mirror()
    glass = [s.add_dielectric(1.5), s.add_dielectric(float(F(1.0) / F(1.5))), s.add_dielectric(1.0)]
    tinted = s.add_dielectric(1.33, extinction=(0.0, 0.0, 0.0) if variant == "dark" else TINT)
    lit = variant != "dark"
    lq, ls, lt = (s.add_emissive((20, 18, 15)), s.add_emissive((9, 12, 14)), s.add_emissive((14, 6, 6))) if lit else (white, red, cb)
    if variant == "many":
        ls = lt = white
    if variant == "many":                                                                  # emitter 0: a light that faces -x exactly
        s.add_quad((1.0, 1.0, 0.0), (0, 0, 0.25), (0, 0.25, 0), s.add_emissive((30, 28, 26)))
    s.add_quad((-1.2, 0, 1.2), (2.4, 0, 0), (0, 0, -2.4), white)
    s.add_quad((-1.2, 0, -1.2), (2.4, 0, 0), (0, 2.0, 0), cb)
    s.add_quad((-1.2, 0, 1.2), (0, 0, -2.4), (0, 2.0, 0), tn)                              # (faces +x)
    s.add_quad((1.2, 0, -1.2), (0, 0, 2.4), (0, 2.0, 0), tb)
    s.add_quad((-0.5, 1.99, -0.5), (1.0, 0, 0), (0, 0, 1.0), lq)
    s.add_quad((-0.9, 0.3, 0.2), (0.7, 0.1, 0.2), (0.3, 0.9, 0.1), red)                    # neither unit nor orthogonal edges
    s.add_quad((-1.0, 0.25, 0.5), (0.5, 0, 0), (0, 0, -0.5), cb0)
    for k, g in enumerate(glass):                                                          # normal = (0, 0, -1) x ... exactly +y
        s.add_quad((-1.0 + 0.75 * k, 0.5, 1.0), (0.5, 0, 0), (0, 0, -0.5), g)
    s.add_quad((0.25, 1.25, 0.75), (0.5, 0, 0), (0, 0, -0.5), mirror)
    if variant == "many":
        for k in range(9):
            s.add_quad((-1.0 + 0.22 * k, 1.9 - 0.05 * k, -1.0), (0.2, 0, 0), (0, 0, 0.2 + 0.1 * k), s.add_emissive((5 + k, 9, 14 - k)))
    s.add_sphere((0.55, 1.45, 0.3), 0.12, ls)
    s.add_sphere((-0.55, 0.35, 0.1), 0.35, mirror)
    s.add_sphere((0.45, 0.3, 0.45), 0.3, glass[0])
    s.add_sphere((0.0, 0.95, -0.3), 0.25, tinted)
    s.add_sphere((0.6, 0.25, -0.5), 0.25, cb)
    s.add_sphere((-0.6, 1.2, -0.6), 0.3, tn)
    s.add_sphere((0.0, 0.3, 0.9), 0.25, white)
    nv = 24
    pos = rng.uniform([-0.9, 0.05, -0.9], [0.9, 1.5, 0.9], (nv, 3)).astype(F)
    nrm = rng.normal(size=(nv, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    base = s.add_vertices(pos, nrm, rng.uniform(-3, 3, (nv, 2)).astype(F))
    mats = [white, tb, cb, mirror, glass[0], tinted, lt, tn]
    for i in range(16):
        a, b, c = (int(x) for x in rng.choice(nv, 3, replace=False))
        s.add_triangle(base + a, base + b, base + c, mats[i % len(mats)])
    r = F(np.sqrt(0.5))
    cancel = np.array([[0, 1, 0], [0, -1, 0], [0, 1, 0]], F)                               # l0 = l1: the interpolated normal is 0
    equal = np.array([[r, r, 0], [r, -r, 0], [-r, r, 0]], F)                               # |n.x| == |n.y| at the corners and beyond
    for n3, m in ((cancel, white), (cancel, glass[0]), (equal, cb), (equal, mirror)):
        b = s.add_vertices(rng.uniform([-0.9, 0.05, -0.9], [0.9, 1.5, 0.9], (3, 3)).astype(F), n3, rng.uniform(-3, 3, (3, 2)).astype(F))
        s.add_triangle(b, b + 1, b + 2, m)
    if variant in ("rich", "env0", "env1"):
        p = {"rich": 0.5, "env0": 0.0, "env1": 1.0}[variant]
        s.set_environment(s.add_texture(env_scenes.sky_texels(8, 16), abi.TEX_BILINEAR), (1.5, 1.0, 0.75), p)
    return s.compile()


def arrays(cs):
    d = cs.desc
    ns, nq, nt = int(d.num_spheres), int(d.num_quads), int(d.num_triangles)
    mats = np.ctypeslib.as_array(d.materials, (ns + nq + nt,)).copy()
    return ns, nq, nt, mats >> abi.MATERIAL_TAG_SHIFT


# ------------------------------------------------------------------------------------------------------------------ records

def records(o, d, t, ids, u, v, T=None, ext=None, rng=None, bounce=0, discrete=1):
    n = len(ids)
    rec = np.zeros((n, IN), U)
    rec[:, 0:3] = words(np.broadcast_to(np.asarray(o, F), (n, 3)))
    rec[:, 3:6] = words(np.broadcast_to(np.asarray(d, F), (n, 3)))
    rec[:, 6] = words(np.broadcast_to(np.asarray(t, F), (n,)))
    rec[:, 7] = np.asarray(ids, np.int32).view(U)
    rec[:, 8] = words(np.broadcast_to(np.asarray(u, F), (n,)))
    rec[:, 9] = words(np.broadcast_to(np.asarray(v, F), (n,)))
    rec[:, 10:13] = words(np.broadcast_to(np.asarray((1, 1, 1) if T is None else T, F), (n, 3)))
    rec[:, 13:16] = words(np.broadcast_to(np.asarray((0, 0, 0) if ext is None else ext, F), (n, 3)))
    rec[:, 16] = np.broadcast_to(np.asarray(0x9E3779B9 if rng is None else rng, U), (n,))
    rec[:, 17] = (np.broadcast_to(np.asarray(bounce, U), (n,)) << U(1)) | np.broadcast_to(np.asarray(discrete, U), (n,))
    return rec


def after(f32, k):
    """The float32 k ulps from f32 (positive values)."""
    return (np.asarray(f32, F).view(U).astype(np.int64) + np.asarray(k)).astype(U).view(F)


T_VALUES = np.concatenate([[0.0, 1e-45, 1e-39, 1e-3, 0.03, 0.3, 0.7, 1.0, 1.5, 40.0, 1e30], after(0.99, np.arange(-2, 3))]).astype(F)


def state_strata(rng, n):
    T = rng.choice(T_VALUES, (n, 3))
    same = rng.random(n) < 0.3
    T[same] = T[same][:, :1]
    ext = np.where((rng.random(n) < 0.5)[:, None], np.asarray(TINT, F)[None, :] * rng.choice([1.0, 0.0, 7.0], (n, 3)).astype(F), F(0))
    return T, ext.astype(F), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U), rng.choice(BOUNCES, n).astype(U), rng.integers(0, 2, n).astype(U)


@functools.lru_cache(maxsize=None)
def traced(variant, n=24000):
    """(records, the hits' shading normals) of the traced family on scene(variant)."""
    from oracle import hj_oracle as oracle
    cs = scene(variant)
    rng = np.random.default_rng([fuzz_cases.source_seed(), VARIANTS.index(variant)])
    ns = int(cs.desc.num_spheres)
    sph = np.ctypeslib.as_array(C.cast(cs.desc.spheres, C.POINTER(C.c_float)), (ns, 4)).copy()
    k = n // 3
    o_box = rng.uniform([-1.1, 0.05, -1.1], [1.1, 1.9, 1.1], (k, 3))
    pick = rng.integers(0, ns, k)                                                         # origins inside the spheres: total internal reflection
    inside = sph[pick, :3] + rng.normal(size=(k, 3)) * 0.3 * sph[pick, 3:4]
    d = rng.normal(size=(2 * k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.exp(rng.uniform(-3, 3, (2 * k, 1)))
    rays = np.zeros((2 * k, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = np.concatenate([o_box, inside]), d, 1e-4, np.inf
    block = abi.ImageBlock()
    block.dimension[:] = (32, 32)
    block.original_dimension[:] = (32, 32)
    block.origin[:] = (0, 0)
    block.sample_offset[:] = (0.5, 0.5)
    block.seed = 77
    with_log = oracle.logged_rays(cs, [block], opts())
    log = with_log[with_log[:, 8] == 0][:, :8]
    log = log[rng.choice(len(log), n - 2 * k, replace=len(log) < n - 2 * k)]
    rays = np.concatenate([rays, log.astype(F)])
    ids, t, u, v, full = oracle.intersect(cs, rays, full=True)
    T, ext, states, bounce, disc = state_strata(rng, n)
    return records(rays[:, 0:3], rays[:, 3:6], t, ids, u, v, T, ext, states, bounce, disc), full[:, 3:6].copy()


def shapes_of(cs, tag=None, kind=None):
    ns, nq, nt, tags = arrays(cs)
    ids = np.arange(ns + nq + nt)
    kinds = np.where(ids < ns, 0, np.where(ids < ns + nq, 1, 2))
    keep = np.ones(len(ids), bool)
    if tag is not None:
        keep &= tags == tag
    if kind is not None:
        keep &= kinds == kind
    return ids[keep]


@functools.lru_cache(maxsize=None)
def geometry(variant):
    """Crafted hits.  t == 0 puts the hit point exactly where the origin is."""
    cs = scene(variant)
    rng = np.random.default_rng([fuzz_cases.source_seed(), 100 + VARIANTS.index(variant)])
    ns, nq, nt, tags = arrays(cs)
    sph = np.ctypeslib.as_array(C.cast(cs.desc.spheres, C.POINTER(C.c_float)), (ns, 4)).copy()
    dirs = np.array([[0.3, -0.8, 0.52], [1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0.6, -0.8], [-0.6, 0, 0.8], [0.6, 0.8, 0], [-0.0, -1, 0.0],
                     [1e-12, 0, 0], [0, -1e-12, 1e-12], [1e12, -1e12, 3e11], [0, 0, -1e12], [0, 0, 0]], F)
    out = []
    for i in range(ns):                                                                   # poles, the n.x == 0 meridian, n.y beyond +-1
        c, r = sph[i, :3], sph[i, 3]
        th = np.linspace(0, 2 * np.pi, 17)
        pts = [c + F(r) * np.array([0, 1, 0], F), c - F(r) * np.array([0, 1, 0], F), c + np.array([0, r * F(1.0001), 0], F),
               c - np.array([0, after(r, 3)[()], 0], F), c + np.array([0, after(r, -3)[()], 0], F)]
        pts += [c + np.array([0, r * np.sin(a), r * np.cos(a)], F) for a in th] + [c + np.array([r * np.cos(a), 0, r * np.sin(a)], F) for a in th]
        pts = np.array(pts, F)
        for d in dirs:
            out.append(records(pts, d, 0.0, np.full(len(pts), i), 0.0, 0.0, rng=rng.integers(1, 1 << 32, len(pts), dtype=np.uint64)))
            out.append(records(pts - F(0.75) * d, d, 0.75, np.full(len(pts), i), 0.0, 0.0, bounce=RR_START, T=(0.7, 0.3, 0.03)))
    uv = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.5, 0], [0, 0.5], [0.25, 0.75], [0.3, 0.3], [-0.0, 1.0], [1.0, 1.0], [-0.25, 0.5]], F)
    flat = np.arange(ns, ns + nq + nt)
    for d in dirs:                                                                        # corners and edges of every quad and triangle
        g = np.repeat(flat, len(uv))
        p = rng.uniform([-1, 0.1, -1], [1, 1.8, 1], (len(g), 3)).astype(F)
        for t in (0.0, 1.5):
            out.append(records(p, d, t, g, np.tile(uv[:, 0], len(flat)), np.tile(uv[:, 1], len(flat)),
                               rng=rng.integers(1, 1 << 32, len(g), dtype=np.uint64), bounce=rng.choice(BOUNCES, len(g)),
                               discrete=rng.integers(0, 2, len(g))))
    return np.concatenate(out)


def draw_states(u32):
    """States whose next draw is u32."""
    return unxorshift(np.asarray(u32, np.int64).astype(U))


def float_draws(f32, spread=2):
    """The uint32 draws whose rng_float is f32 and the floats `spread` ulps each side (f32 in [2^-8, 1): a float is 256+ draws wide)."""
    fs = after(f32, np.arange(-spread, spread + 1))
    lo = np.floor(fs.astype(np.float64) * 2.0 ** 32).astype(np.int64)
    return np.unique(np.clip(np.concatenate([lo, lo - 1, lo + 1, lo + 255, lo - 255]), 0, 0xFFFFFFFF))


def bisect_draw(cs, rec, flips):
    """Per record, the smallest first draw at which `flips(out)` (monotone in the draw) holds, found with the oracle's own step."""
    from oracle import hj_oracle as oracle
    lo, hi = np.zeros(len(rec), np.int64), np.full(len(rec), 0xFFFFFFFF, np.int64)     # flips is false at lo, true at hi
    for _ in range(32):
        mid = (lo + hi) // 2
        r = rec.copy()
        r[:, 16] = draw_states(mid)
        f = flips(oracle.shade_step(cs, r, opts()))
        hi, lo = np.where(f, mid, hi), np.where(f, lo, mid)
    return hi


@functools.lru_cache(maxsize=None)
def branches(variant):
    """Records on the stage's comparisons; returns (records, {name: slice}) so that the CPU test can check each claim."""
    from oracle import hj_oracle as oracle
    cs = scene(variant)
    ns, nq, nt, tags = arrays(cs)
    d = cs.desc
    out, parts, at = [], {}, 0

    def add(name, rec):
        nonlocal at
        out.append(rec)
        parts[name] = slice(at, at + len(rec))
        at += len(rec)

    glass_quads = shapes_of(cs, abi.MAT_DIELECTRIC, 1)                                     # normal exactly +y: cosI = -d.y
    p = np.array([0.1, 0.5, 0.9], F)
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-45, -3e-45, 1e-30, -1e-30], F)
    for q in glass_quads:
        dd = np.stack([np.full(len(tiny), 0.8, F), tiny, np.full(len(tiny), 0.6, F)], 1)
        add(f"cosI0_{q}", records(p, dd, 0.0, np.full(len(tiny), q), 0.3, 0.3, ext=TINT))
        # the k == 0 transition: cosI swept 64 ulps each side of where 1 - etaInv^2 (1 - cosI^2) changes sign, both faces
        eta = float(np.ctypeslib.as_array(C.cast(d.dielectric, C.POINTER(C.c_float)), (int(d.num_dielectric), 4))[int(np.ctypeslib.as_array(d.materials, (ns + nq + nt,))[q] & abi.MATERIAL_INDEX_MASK), 3])
        for sign, e in ((1.0, eta), (-1.0, 1.0 / eta)):                                    # e: the eta the face sees; k <= 0 needs e < 1
            if e >= 1.0:
                continue
            c = after(np.sqrt(1.0 - e * e), np.arange(-64, 65))
            dd = np.stack([np.sqrt(np.maximum(0, 1 - c.astype(np.float64) ** 2)).astype(F), F(-sign) * c, np.zeros(len(c), F)], 1)
            add(f"k0_{q}_{int(sign)}", records(p, dd, 0.0, np.full(len(c), q), 0.3, 0.3, ext=TINT, bounce=1))
        # the Fresnel draw on fr: the threshold draw found by bisection with the oracle, then its neighbours
        dd = np.array([[0.6, -0.8, 0.0], [0.6, 0.8, 0.0], [0.96, -0.28, 0.0], [0.0, -1.0, 0.0]], F)
        base = records(p, dd, 0.0, np.full(len(dd), q), 0.3, 0.3, bounce=1)
        refl = oracle.shade_step(cs, base, opts())[:, 5].view(F) * dd[:, 1] < 0             # (reflection turns wo.y round)
        thr = bisect_draw(cs, base, lambda o: ~((o[:, 5].view(F) * dd[:, 1] < 0) | ((o[:, 5] << U(1)) == 0)))
        near = (thr[:, None] + np.array([-513, -257, -256, -255, -17, -16, -1, 0, 1, 15, 16, 255, 256, 257, 513])[None, :]).clip(0, 0xFFFFFFFF)
        rec = np.repeat(base, near.shape[1], axis=0)
        rec[:, 16] = draw_states(near.ravel())
        add(f"fresnel_{q}", rec)
        del refl
    # roulette: the draw on q, q at the 0.99 cap (T = 1 through a mirror) and below it
    mq = shapes_of(cs, abi.MAT_MIRROR, 1)[0]
    for name, T, q in (("rr_cap", (1, 1, 1), F(0.99)), ("rr_half", (0.5, 0.25, 0.125), F(0.5)), ("rr_cap_above", (1.5, 0.2, 0.99), F(0.99))):
        dr = float_draws(q)
        add(name, records(p, (0.6, -0.8, 0.0), 0.0, np.full(len(dr), mq), 0.3, 0.3, T=T, rng=draw_states(dr), bounce=RR_START))
    add("rr_cap_last", records(p, (0.6, -0.8, 0.0), 0.0, np.full(8, mq), 0.3, 0.3, T=(1e-3, 0, 0), rng=draw_states(np.arange(8) << 29), bounce=MAX_BOUNCES - 1))
    # next-event estimation from a diffuse floor point
    floor = shapes_of(cs, abi.MAT_DIFFUSE, 1)[0]
    ne = int(d.num_emitters)
    env = getattr(cs, "environment", None)
    pe = F(env.select_prob) if env is not None else None
    if ne:
        pdf = np.array([d.emitters[e].pdf for e in range(ne)], F)
        cdf = np.zeros(ne, F)
        acc = F(0)
        for e in range(ne):
            acc = F(acc + pdf[e])
            cdf[e] = acc
        steps = cdf if pe is None else (pe + cdf * (F(1) - pe)).astype(F)
        dr = np.concatenate([float_draws(min(float(c), 0.99999994), 4) for c in steps])
        add("cdf", records((0.1, 0.0, 0.2), (0.0, -1.0, 0.0), 0.0, np.full(len(dr), floor), 0.3, 0.3, rng=draw_states(dr)))
    if pe is not None and 0 < pe < 1:
        dr = float_draws(pe)
        add("coin", records((0.1, 0.0, 0.2), (0.0, -1.0, 0.0), 0.0, np.full(len(dr), floor), 0.3, 0.3, rng=draw_states(dr)))
    if variant == "many":
        # state 0 draws 0 for ever: emitter 0 (a quad that faces -x), sampled at its origin; the hit is on the wall that faces +x
        floor = shapes_of(cs, abi.MAT_DIFFUSE_TEXTURED, 1)[0]
        q0 = np.ctypeslib.as_array(C.cast(d.quads, C.POINTER(C.c_float)), (nq, 12))[int(d.emitters[0].shape) - ns]
        org, e1, e2 = q0[0:3].copy(), q0[4:7].copy(), q0[8:11].copy()
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm)
        below = (org + nrm.astype(F)).astype(F)
        pts = np.array([org, below, org + F(0.5) * e1, org - F(0.25) * e2, org + F(0.5) * e1 + F(2.0) * e2, org - nrm.astype(F)], F)
        names = ("dist0", "below", "cosT0_a", "cosT0_b", "cosT0_c", "behind")
        for nm, pt in zip(names, pts):
            add(nm, records(pt, -nrm.astype(F), 0.0, np.full(3, floor), 0.3, 0.3, rng=0, T=[(1, 1, 1), (0.5, 2, 0), (1e30, 1, 1)]))
        # dot(shadow direction, n) == 0 under a light that is seen face on: the hit's normal is exactly +y (the power-of-two
        # checkerboard quad), the reference point level with the sampled point, and one ulp above and below
        level = shapes_of(cs, abi.MAT_DIFFUSECBOARD, 1)[-1]
        ys = after(org[1], [0, 1, -1, 2, -2])
        for x in (0.5, 0.75, -1.0):
            pts = np.stack([np.full(5, x, F), ys, np.full(5, org[2], F)], 1)
            add(f"dot0_{x}", records(pts, (0.0, -1.0, 0.0), 0.0, np.full(5, level), 0.3, 0.3, rng=0))
        # the importance at kEps: straight in front of the light the importance falls with the distance; the distance where the oracle
        # stops wanting a shadow ray, found by bisection over the float's bits, and 8 ulps each side
        lo, hi = int(F(1.0).view(U)), int(F(1e6).view(U))
        for _ in range(32):
            mid = (lo + hi) // 2
            r = records((org + nrm.astype(F) * U(mid).view(F)).astype(F)[None, :], -nrm.astype(F), 0.0, [floor], 0.3, 0.3, rng=0)
            if oracle.shade_step(cs, r, opts())[0, 15]:
                lo = mid
            else:
                hi = mid
        dist = (np.int64(hi) + np.arange(-8, 9)).astype(U).view(F)
        add("imp_eps", records((org[None, :] + nrm.astype(F)[None, :] * dist[:, None]).astype(F), -nrm.astype(F), 0.0, np.full(len(dist), floor), 0.3, 0.3, rng=0))
    # checkerboard arguments on quads (a quad's u, v are the raw hit's): negative, huge, cell boundaries, scale 0
    vals = np.concatenate([np.array([0.0, -0.0, 0.13, 0.26, 0.21, 0.42, -0.13, 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan, 1e-45, 0.25, 0.5], F),
                           after(0.13, [-1, 1]), after(0.26, [-1, 1]), after(0.42, [-1, 1])])
    for q in shapes_of(cs, abi.MAT_DIFFUSECBOARD, 1):
        uu, vv = np.repeat(vals, len(vals)), np.tile(vals, len(vals))
        add(f"cboard_{q}", records((0.1, 0.3, 0.2), (0.3, -0.8, 0.52), 0.0, np.full(len(uu), q), uu, vv))
    return np.concatenate(out), parts


@functools.lru_cache(maxsize=None)
def expected(family, variant):
    from oracle import hj_oracle as oracle
    return oracle.shade_step(scene(variant), inputs(family, variant), opts())


def inputs(family, variant):
    if family == "traced":
        return traced(variant)[0]
    if family == "geometry":
        return geometry(variant)
    return branches(variant)[0]


# -------------------------------------------------------------------------------------------------- premises (no GPU needed)

def has_nan(out):
    with np.errstate(invalid="ignore"):
        return (np.isnan(out.view(F)) & FLOAT_OUT[None, :]).any(1)


def test_traced_records_reach_every_outcome():
    """From the oracle alone: per material tag at least 100 continuing and 100 ending records (an emissive hit always ends), 100 each
    of reflection, refraction and total internal reflection, of roulette kill and survival and of the bounce cap, of shadow rays
    wanted and rejected; at most 1 record in 1000 with a NaN output word, so that "a NaN equals any NaN" cannot carry the comparison."""
    seen = set()
    for variant in VARIANTS:
        cs = scene(variant)
        rec, nrm = traced(variant)
        out = expected("traced", variant)
        ns, nq, nt, tags = arrays(cs)
        ids = rec[:, 7].view(np.int32)
        hit = ids >= 0
        tag = np.where(hit, tags[np.maximum(ids, 0)], 99)
        alive, bounce = out[:, 0] == 1, rec[:, 17] >> 1
        assert has_nan(out).sum() * 1000 <= len(out), (variant, int(has_nan(out).sum()), len(out))
        assert hit.sum() >= 0.8 * len(rec)
        for tg in (abi.MAT_DIFFUSE, abi.MAT_DIFFUSECBOARD, abi.MAT_DIFFUSE_TEXTURED, abi.MAT_MIRROR, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE):
            if tg == abi.MAT_EMISSIVE and variant in ("dark",):
                continue
            assert ((tag == tg) & ~alive).sum() >= 100, (variant, tg)
            if tg != abi.MAT_EMISSIVE:
                assert ((tag == tg) & alive).sum() >= 100, (variant, tg)
            else:
                assert not ((tag == tg) & alive).any()
                assert ((tag == tg) & (out[:, 26:29] != 0).any(1)).sum() >= 100 and ((tag == tg) & (out[:, 26:29] == 0).all(1)).sum() >= 100
        gl = (tag == abi.MAT_DIELECTRIC) & (bounce < RR_START)                            # (always alive; no roulette draw)
        assert alive[gl].all()
        drew = out[:, 11] != rec[:, 16]
        with np.errstate(invalid="ignore", over="ignore"):
            din = (rec[:, 3:6].view(F).astype(np.float64) * nrm).sum(1)
            dout = (out[:, 4:7].view(F).astype(np.float64) * nrm).sum(1)
        assert (gl & ~drew).sum() >= 100, variant                                        # total internal reflection: no Fresnel draw
        assert (gl & drew & (din * dout < 0)).sum() >= 100, variant                      # reflected: wo on the side the ray came from
        assert (gl & drew & (din * dout > 0)).sum() >= 100, variant                      # refracted
        rr = hit & (tag != abi.MAT_EMISSIVE) & (bounce >= RR_START) & (bounce + 1 < MAX_BOUNCES)
        assert (rr & alive).sum() >= 100 and (rr & ~alive).sum() >= 100, variant
        assert (hit & (tag != abi.MAT_EMISSIVE) & (bounce + 1 == MAX_BOUNCES) & ~alive).sum() >= 100, variant
        assert not (alive & (bounce + 1 == MAX_BOUNCES)).any()
        diffuse = (tag == abi.MAT_DIFFUSE) | (tag == abi.MAT_DIFFUSECBOARD) | (tag == abi.MAT_DIFFUSE_TEXTURED)
        if variant != "dark":
            assert (diffuse & (out[:, 15] == 1)).sum() >= 100, variant
        assert (diffuse & (out[:, 15] == 0)).sum() >= 100, variant
        assert not (~diffuse & (out[:, 15] == 1)).any()
        miss = ~hit
        lit = (out[miss, 26:29] != 0).any(1)
        assert miss.sum() >= 100
        assert lit.any() == (variant in ("rich", "env0", "env1")) and not out[miss][:, :26].any()
        if lit.any():                                                                     # the miss rule per channel: a tinted channel adds nothing
            e = rec[miss, 13:16].view(F)
            assert ((out[miss, 26:29] == 0) >= (e != 0))[rec[miss, 17] & 1 == 1].all() and (lit & (e != 0).any(1)).sum() >= 20
        assert (out[:, 29:33].any(1) == (hit & (bounce == 0))).all() or has_nan(out).any()
        seen.add(variant)
    assert seen == set(VARIANTS)


def test_crafted_records_sit_on_their_branches():
    """From the oracle alone: the crafted records do what their names say."""
    from oracle import hj_oracle as oracle
    for variant in ("rich", "many"):
        cs = scene(variant)
        rec, parts = branches(variant)
        out = expected("branches", variant)
        fresnel_rows = 0
        for name, sl in parts.items():
            r, o = rec[sl], out[sl]
            drew = o[:, 11] != r[:, 16]
            if name.startswith("cosI0"):
                assert (o[:, 0] == 1).all() and len({tuple(x) for x in o[:, 12:15]}) >= (2 if variant == "rich" else 1)
            elif name.startswith("k0_"):
                assert drew.any() and (~drew).any(), name                                 # both sides of k <= 0 inside the sweep
                assert (np.diff(drew.astype(int)) != 0).sum() == 1, name
            elif name.startswith("fresnel"):
                side = o[:, 5].view(F) * r[:, 4].view(F) < 0
                per = side.reshape(-1, 15)
                ok = (r[:, 3].view(F) != 0).reshape(-1, 15)[:, 0] & drew.reshape(-1, 15).any(1)   # (not head-on, not totally reflected)
                both = per[ok].any(1) & (~per[ok]).any(1)                                  # reflected below the threshold, refracted from it on
                fresnel_rows += int(both.sum())                                            # (eta = 1: fr is 0 or a rounding error)
            elif name in ("rr_cap", "rr_half", "rr_cap_above"):
                assert (o[:, 0] == 1).any() and (o[:, 0] == 0).any(), name
            elif name == "rr_cap_last":
                assert (o[:, 0] == 0).all()
            elif name == "cdf":
                assert len({tuple(x) for x in o[:, 19:22]}) + (o[:, 15] == 0).any() >= 2, name
            elif name == "coin":
                assert len({int(x) for x in o[:, 22]}) + (o[:, 15] == 0).any() >= 2, name   # tMax = inf for the environment only
            elif name == "below":
                assert (o[:, 15] == 1).all() and (o[0, 22].view(F) == F(1.0) - KEPS)     # the sampled point IS the quad's origin ...
            elif name in ("dist0", "cosT0_a", "cosT0_b", "cosT0_c", "behind"):
                assert (o[:, 15] == 0).all(), name                                        # ... so these are rejected
            elif name.startswith("dot0"):
                assert o[:, 15].tolist() == [0, 0, 1, 0, 1], name                          # wanted only from below the light's level
            elif name == "imp_eps":
                w = o[:, 15]
                assert w[0] == 1 and w[-1] == 0 and (np.diff(w.astype(int)) != 0).sum() == 1
            elif name.startswith("cboard"):
                assert len({tuple(x) for x in o[:, 7:10]}) == 2, name                     # both colours
        assert any(n.startswith("k0_") for n in parts) and fresnel_rows >= 4


def chain(cs, block, o):
    """hjo_integrate_block's samples from hjo_shade_step, oracle.intersect for the rays between the steps and for the shadow rays."""
    from oracle import hj_oracle as oracle
    W, H = int(block.dimension[0]), int(block.dimension[1])
    ly, lx = np.mgrid[0:H, 0:W]
    px = np.stack([lx.ravel() + block.origin[0] + block.sample_offset[0], ly.ravel() + block.origin[1] + block.sample_offset[1]], 1).astype(F)
    cam = oracle.camera_rays(cs.desc.camera, int(block.original_dimension[0]), int(block.original_dimension[1]), px)
    n = W * H
    L = oracle.lib()
    seeds = np.array([L.hjo_rng_seed(int(block.seed + x + y * W) & 0xFFFFFFFF) for y, x in zip(ly.ravel(), lx.ravel())], U)
    rec = records(cam[:, 0:3], cam[:, 3:6], 0.0, np.zeros(n, np.int32), 0.0, 0.0, rng=seeds, bounce=0, discrete=1)
    tmin = np.full(n, KEPS, F)
    total = np.zeros((n, 3), F)
    nd = np.zeros((n, 4), F)
    live = np.arange(n)
    while len(live):
        rays = np.concatenate([rec[:, 0:6].view(F), tmin[:, None], np.full((len(rec), 1), np.inf, F)], 1)
        ids, t, u, v = oracle.intersect(cs, rays, use_bvh=bool(o.use_bvh))
        rec[:, 6], rec[:, 7], rec[:, 8], rec[:, 9] = words(t), ids.view(U), words(u), words(v)
        out = oracle.shade_step(cs, rec, o)
        total[live] = total[live] + out[:, 26:29].view(F)                                 # (+0 where the step added nothing)
        first = (rec[:, 17] >> 1) == 0
        nd[live[first]] = out[first, 29:33].view(F)
        sh = out[:, 15] == 1
        if sh.any():
            srays = np.concatenate([out[sh, 16:22].view(F), np.full((int(sh.sum()), 1), F(2) * KEPS, F), out[sh, 22:23].view(F)], 1)
            occ = oracle.intersect(cs, srays, use_bvh=bool(o.use_bvh))[0] >= 0
            idx = live[sh][~occ]
            total[idx] = total[idx] + out[sh][~occ][:, 23:26].view(F)
        go = out[:, 0] == 1
        nxt = np.zeros((int(go.sum()), IN), U)
        nxt[:, 0:3], nxt[:, 3:6], nxt[:, 10:13], nxt[:, 13:16] = out[go, 1:4], out[go, 4:7], out[go, 7:10], out[go, 12:15]
        nxt[:, 16], nxt[:, 17] = out[go, 11], out[go, 10]
        rec, live, tmin = nxt, live[go], np.full(int(go.sum()), F(2) * KEPS, F)
    return np.concatenate([total, np.ones((n, 1), F), nd], 1).reshape(H, W, 8)


@pytest.mark.parametrize("which", ["spheres", "environment"])
def test_chained_steps_are_the_integrator(which):
    """hjo_shade_step is integrate_ray's own loop body: chained by the test it gives hjo_integrate_block's samples bit for bit."""
    from oracle import hj_oracle as oracle
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile() if which == "spheres" else env_scenes.mixed_scene(tinted=True)
    block = abi.ImageBlock()
    block.dimension[:] = (32, 32)
    block.original_dimension[:] = (32, 32)
    block.origin[:] = (0, 0)
    block.sample_offset[:] = (0.25, 0.75)
    block.seed = 4242
    o = abi.RenderOpts.default()
    o.max_bounces = 40
    want, _ = oracle.integrate_block(cs, block, o)
    got = chain(cs, block, o)
    assert np.array_equal(got.view(U), want.view(U)), int((got.view(U) != want.view(U)).sum())


# ----------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.fixture(scope="module")
def renderer():
    with device.Renderer(0) as r:
        yield r


def run(r, rec, o, num_wg, parity):
    got, ctr = [], []
    for a in range(0, len(rec), abi.STEP_MAX_RECORDS):
        g, c = r.shade_step(rec[a:a + abi.STEP_MAX_RECORDS], o, num_wg, parity)
        got.append(g)
        ctr.append(c)
    return np.concatenate(got), ctr


def counters_of(want, n0, num_wg):
    """What the stage's per-workgroup counters must be for records n0 .. of `want` dealt i % num_wg."""
    g = np.arange(len(want)) % num_wg
    return np.stack([np.bincount(g, want[:, 0] == 1, num_wg), np.bincount(g, want[:, 15] == 1, num_wg), np.zeros(num_wg)], 1).astype(U)


def check(r, name, rec, want, num_wg=3, parity=0):
    got, ctr = run(r, rec, opts(), num_wg, parity)
    msg = report(name, rec, got, want)
    assert not msg, msg
    for k, c in enumerate(ctr):
        a = k * abi.STEP_MAX_RECORDS
        assert np.array_equal(c, counters_of(want[a:a + abi.STEP_MAX_RECORDS], a, num_wg)), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_traced_records_bit_exact(renderer, variant):
    renderer.upload_scene(scene(variant))
    rec = inputs("traced", variant)
    check(renderer, f"traced/{variant}", rec, expected("traced", variant), num_wg=5, parity=VARIANTS.index(variant) & 1)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rich", "many", "dark"])
def test_crafted_geometry_bit_exact(renderer, variant):
    renderer.upload_scene(scene(variant))
    check(renderer, f"geometry/{variant}", inputs("geometry", variant), expected("geometry", variant), num_wg=2, parity=1)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rich", "env0", "env1", "many"])
def test_crafted_branches_bit_exact(renderer, variant):
    renderer.upload_scene(scene(variant))
    check(renderer, f"branches/{variant}", inputs("branches", variant), expected("branches", variant), num_wg=1, parity=0)


def by_tag_counts(cs, rec, counts, rng):
    """Records of `rec` picked so that bin k of workgroup 0 (num_wg = 1) holds counts[k] hits; the miss bin last."""
    ns, nq, nt, tags = arrays(cs)
    ids = rec[:, 7].view(np.int32)
    bins = np.where(ids < 0, 5, np.where(tags[np.maximum(ids, 0)] == abi.MAT_DIFFUSE_TEXTURED, abi.MAT_DIFFUSECBOARD, tags[np.maximum(ids, 0)]))
    pick = np.concatenate([rng.choice(np.flatnonzero(bins == k), c, replace=False) for k, c in enumerate(counts)])
    return rng.permutation(pick)


@pytest.mark.gpu
def test_wave_and_queue_structure(renderer):
    """Bin sizes around the wave (64) and the workgroup (64 x waves), 1, 2 and 5 workgroups with n no multiple of them, both
    parities, one tag only, misses only - the records and the expected outputs are the traced family's."""
    cs = scene("rich")
    renderer.upload_scene(cs)
    rec, want = inputs("traced", "rich"), expected("traced", "rich")
    rng = np.random.default_rng(5)
    W = 64 * 4                                                                            # the shade kernel's workgroup: 4 waves (HJ_BLOCK_THREADS)
    sizes = (0, 1, 63, 64, 65, W - 1, W, W + 1)
    for j in range(len(sizes)):
        counts = [sizes[(j + k) % len(sizes)] for k in range(6)]
        sel = by_tag_counts(cs, rec, counts, rng)
        check(renderer, f"bins {counts}", rec[sel], want[sel], num_wg=1, parity=j & 1)
    for num_wg, n in ((1, 1), (2, 1001), (5, 4099), (2, 3), (5, 7)):
        for parity in (0, 1):
            sel = rng.choice(len(rec), n, replace=False)
            check(renderer, f"num_wg {num_wg} n {n} parity {parity}", rec[sel], want[sel], num_wg=num_wg, parity=parity)
    for k in range(6):
        counts = [0] * 6
        counts[k] = 777
        sel = by_tag_counts(cs, rec, counts, rng)
        check(renderer, f"only bin {k}", rec[sel], want[sel], num_wg=2, parity=k & 1)
    dark = scene("dark")                                                                  # no environment: misses leave nothing at all
    renderer.upload_scene(dark)
    rec, want = inputs("traced", "dark"), expected("traced", "dark")
    sel = np.flatnonzero(rec[:, 7].view(np.int32) < 0)
    assert len(sel) >= 100 and not want[sel].any()
    check(renderer, "misses only, no environment", rec[sel], want[sel], num_wg=2, parity=0)


def nee(out):
    """A record's next-event contribution: the shadow record's colour when there is one, else what the sample received (+ 0, as
    the sample buffer adds it to its zero)."""
    sh = out[:, 15] == 1
    return np.where(sh[:, None], out[:, 23:26].view(F) + F(0), out[:, 26:29].view(F))


@pytest.mark.gpu
def test_light_grid_answers_what_the_shadow_ray_would(renderer, monkeypatch):
    """A cbox where the light-shaft grid proves cells: uploaded with the grid and with HJ_LIGHT_GRID=0, the next-event contributions
    are equal bit for bit between the two and the oracle, every other word too; the grid answers some samples, and answers plus
    shadow records are as many as the shadow records without it."""
    from oracle import hj_oracle as oracle
    cs = host.Scene.synthetic(host.SYNTH_CBOX).compile()
    ns, nq, nt, tags = arrays(cs)
    rng = np.random.default_rng(9)
    n = 20000
    o3 = rng.uniform([-0.9, 0.1, -0.9], [0.9, 1.8, 0.9], (n, 3))
    d3 = rng.normal(size=(n, 3))
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o3, d3 / np.linalg.norm(d3, axis=1, keepdims=True), 1e-4, np.inf
    ids, t, u, v = oracle.intersect(cs, rays)
    T, ext, states, bounce, disc = state_strata(rng, n)
    rec = records(rays[:, 0:3], rays[:, 3:6], t, ids, u, v, T, ext, states, bounce, disc)
    want = oracle.shade_step(cs, rec, opts())
    diffuse = (ids >= 0) & (tags[np.maximum(ids, 0)] == abi.MAT_DIFFUSE)
    res = {}
    monkeypatch.delenv("HJ_LIGHT_GRID", raising=False)
    for grid in ("default", "0"):
        if grid == "0":
            monkeypatch.setenv("HJ_LIGHT_GRID", "0")
        renderer.upload_scene(cs)
        res[grid] = renderer.shade_step(rec, opts(grid=True), 3, 1)
    monkeypatch.delenv("HJ_LIGHT_GRID")
    (g1, c1), (g0, c0) = res["default"], res["0"]
    msg = report("HJ_LIGHT_GRID=0", rec, g0, want)
    assert not msg, msg
    assert c0[:, 2].sum() == 0 and c1[:, 2].sum() > 0
    assert np.array_equal(c1[:, 1] + c1[:, 2], c0[:, 1]) and np.array_equal(c1[:, 0], c0[:, 0])
    answered = (g1[:, 15] == 0) & (g0[:, 15] == 1)
    assert answered.sum() == c1[:, 2].sum() and not (answered & ~diffuse).any()
    for side in (g1, g0):
        assert np.array_equal(nee(side)[diffuse].view(U), nee(want)[diffuse].view(U))
    rest = np.r_[0:15, 29:33]
    assert not differing(g1, want)[:, rest].any()
    assert not differing(g1[~answered], want[~answered]).any()
    assert not g1[answered][:, 16:26].any()


@pytest.mark.gpu
def test_refusals(renderer):
    rec = inputs("traced", "rich")[:10]
    with device.Renderer(0) as fresh:
        with pytest.raises(abi.HijikiError) as e:
            fresh.shade_step(rec)
        assert e.value.status == abi.HJ_ERR_STATE
    renderer.upload_scene(scene("rich"))
    ns, nq, nt, _ = arrays(scene("rich"))
    bad = rec.copy()
    bad[3, 7] = ns + nq + nt
    for args in ((rec, None, 0, 0), (rec, None, 11, 0), (rec, None, 1, 2), (bad, None, 1, 0), (rec[:0], None, 1, 0),
                 (np.zeros((abi.STEP_MAX_RECORDS + 1, IN), U), None, 1, 0)):
        with pytest.raises(abi.HijikiError) as e:
            renderer.shade_step(*args)
        assert e.value.status == abi.HJ_ERR_INVALID
    L = device.lib()
    assert L.hj_debug_shade_step(None, None, None, 1, 1, 0, None, None) == abi.HJ_ERR_INVALID
