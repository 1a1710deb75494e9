"""hj_follow_specular and hj_render_aovs_followed restated in numpy, float32 throughout: the specular continuation of a ray at its
hit - a mirror's reflection, a dielectric's deterministic branch - operation for operation (the dot products are the oracle's own
fused form, as the kernels'), and the chain of a frame's samples made by alternating it with a trace the caller brings: on the GPU
hj_trace_rays itself, without one the oracle's intersect."""
import numpy as np

import aov_ref as A
import path_query_ref as P
from hijiki_amd import abi

U, F = np.uint32, np.float32
KEPS = P.KEPS
END, MIRROR, REFRACT_IN, REFRACT_OUT, REFLECT_FR, REFLECT_TIR = range(6)
CLASS_NAMES = ("end", "mirror", "refract entering", "refract leaving", "reflect: fr >= 0.5", "reflect: k <= 0")


def dot3(p, q):
    """fma(p.z, q.z, fma(p.y, q.y, p.x * q.x)): the oracle's dot3, the kernels' dot3"""
    from oracle import hj_oracle as oracle
    p, q = np.ascontiguousarray(p, F).reshape(-1, 3), np.ascontiguousarray(q, F).reshape(-1, 3)
    if not len(p):
        return np.zeros(0, F)
    return oracle.num_batch("dot3", np.concatenate([p.view(U), q.view(U)], 1))[:, 0].copy().view(F)


def reflect(d, n):
    """d - n * (2 * dot(n, d))"""
    s = (F(2) * dot3(n, d)).astype(F)
    return (d - (n * s[:, None]).astype(F)).astype(F)


def empty_rays(n):
    out = np.zeros((n, 8), F)
    out[:, 6], out[:, 7] = np.inf, -np.inf
    return out


def dielectric(eta, d, n):
    """hj_stages.h:560-583 without the draw, every operation float32 -> dict(k, fr (NaN where k <= 0), flipped, reflect, refract)"""
    eta, d, n = np.asarray(eta, F), np.asarray(d, F).reshape(-1, 3), np.asarray(n, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        eta_inv = (F(1) / eta).astype(F)
        cos_i = (-dot3(n, d)).astype(F)
        flip = cos_i < 0
        eta2 = np.where(flip, eta_inv, eta).astype(F)
        eta_inv2 = np.where(flip, (F(1) / eta_inv).astype(F), eta_inv).astype(F)
        normal = np.where(flip[:, None], -n, n).astype(F)
        cos_i = np.where(flip, -cos_i, cos_i).astype(F)
        k = (F(1) - ((eta_inv2 * eta_inv2).astype(F) * (F(1) - (cos_i * cos_i).astype(F)).astype(F)).astype(F)).astype(F)
        cos_o = np.sqrt(np.maximum(k, F(0))).astype(F)
        a, b = (eta2 * cos_i).astype(F), (eta2 * cos_o).astype(F)
        rpar = ((a - cos_o).astype(F) / (a + cos_o).astype(F)).astype(F)
        rorth = ((cos_i - b).astype(F) / (cos_i + b).astype(F)).astype(F)
        fr = (F(0.5) * ((rpar * rpar).astype(F) + (rorth * rorth).astype(F)).astype(F)).astype(F)
        fr = np.where(k <= 0, F(np.nan), fr).astype(F)
        par = (d - (normal * dot3(d, normal)[:, None]).astype(F)).astype(F)
        refract = ((par * eta_inv2[:, None]).astype(F) - (normal * cos_o[:, None]).astype(F)).astype(F)
    return dict(k=k, fr=fr, flipped=flip, reflect=reflect(d, normal), refract=refract)


def continue_rays(cs, rays, hits, surface, detail=False):
    """The continuation of rays (n, 8) at hits (n, 4: shape id bits, t, u, v) whose populated records are surface (n, 16: hit point
    0..2, shading normal 3..5) -> (out (n, 8): the continued ray (p, wo, eps, +inf) or the empty ray, classes (n,) of END ...
    REFLECT_TIR) [, detail: dict(reflect, refract (n, 3): a dielectric's two candidates, zeros elsewhere; k, fr)].
    Records no walk gives (t, d, u, v not finite) can make words of out NaN: the contract fixes which words, not a NaN's sign or
    payload - this processor's differ from the GPU's for a NaN an operation generates (nan_equal compares by that rule)."""
    rays, hits, surface = (np.asarray(a, F).reshape(-1, w) for a, w in ((rays, 8), (hits, 4), (surface, 16)))
    n = len(rays)
    ids = hits[:, 0].copy().view(np.int32).astype(np.int64)
    mats = np.asarray(cs.materials, U)
    valid = (ids >= 0) & (ids < len(mats))
    word = np.zeros(n, U)
    word[valid] = mats[ids[valid]]
    tag, midx = word >> abi.MATERIAL_TAG_SHIFT, (word & U(abi.MATERIAL_INDEX_MASK)).astype(np.int64)
    d, p, nrm = rays[:, 3:6], surface[:, 0:3], surface[:, 3:6]
    out, cls = empty_rays(n), np.full(n, END, np.int8)
    wo = np.zeros((n, 3), F)
    cand = dict(reflect=np.zeros((n, 3), F), refract=np.zeros((n, 3), F), k=np.full(n, np.nan, F), fr=np.full(n, np.nan, F))
    m = valid & (tag == abi.MAT_MIRROR)
    if m.any():
        wo[m], cls[m] = reflect(d[m], nrm[m]), MIRROR
    m = valid & (tag == abi.MAT_DIELECTRIC)
    if m.any():
        eta = np.array([cs.desc.dielectric[int(i)].eta for i in midx[m]], F)
        r = dielectric(eta, d[m], nrm[m])
        tir = r["k"] <= 0
        with np.errstate(invalid="ignore"):
            refl = tir | (r["fr"] >= F(0.5))
        wo[m] = np.where(refl[:, None], r["reflect"], r["refract"])
        cls[m] = np.where(tir, REFLECT_TIR, np.where(refl, REFLECT_FR, np.where(r["flipped"], REFRACT_OUT, REFRACT_IN)))
        for key in cand:
            cand[key][m] = r[key]
    go = cls != END
    out[go, 0:3], out[go, 3:6], out[go, 6], out[go, 7] = p[go], wo[go], KEPS, np.inf
    return (out, cls, cand) if detail else (out, cls)


def nan_equal(got, want):
    """(n, w) float32 arrays by the contract's rule for fabricated records -> the words that differ: a NaN word of `want` must be a
    NaN in `got`, of any sign and payload; every other word must have want's bits"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return np.where(nan, ~np.isnan(got), got.view(U) != want.view(U))


def records(cs, hits, surface):
    """aov_ref.sample_records' record of each (hit, surface) pair, for any set of records"""
    hits, surface = np.asarray(hits, F).reshape(-1, 4), np.asarray(surface, F).reshape(-1, 16)
    mat = A.materials(cs, cs.textures, hits[:, 0].copy().view(np.int32), surface[:, 6], surface[:, 7])
    hit = mat.view(U)[:, 3] != A.MISS
    rec = np.zeros((len(hits), 12), F)
    rec[:, 0:3], rec[:, 3] = mat[:, 0:3], F(1)
    rec[hit, 4:7], rec[hit, 7] = surface[hit, 3:6], hits[hit, 1]
    rec[hit, 8:11], rec[hit, 11] = mat[hit, 4:7], F(1)
    return rec


def oracle_trace(cs):
    """a trace for followed_records that needs no GPU: the oracle's closest hit and populated record"""
    from oracle import hj_oracle as oracle

    def trace(rays):
        ids, t, u, v, full = oracle.intersect(cs, rays, full=True)
        return np.stack([ids.view(F), t, u, v], 1), full
    return trace


def followed_records(cs, rays, max_follow, trace):
    """The chains of `rays` (n, 8: camera rays, tMin = eps, tMax = +inf): trace(rays) -> (hits (n, 4), surface (n, 16)) alternated
    with continue_rays, at most max_follow continuations a chain -> (records (n, 12): the record of each chain's last hit, its word 7
    the float32 sum of the chain's t in chain order - a chain that left a specular surface and hit nothing keeps that surface's
    record -; length (n,): continuations that hit; classes: per round the class of every ray, END where its chain had ended)."""
    n = len(rays)
    hits, surf = trace(rays)
    rec = records(cs, hits, surf)
    length = np.zeros(n, np.int32)
    live = np.arange(n)
    cur = np.asarray(rays, F)
    classes = []
    for _ in range(max_follow):
        nxt, cls = continue_rays(cs, cur, hits, surf)
        full = np.full(n, END, np.int8)
        full[live] = cls
        classes.append(full)
        go = cls != END
        if not go.any():
            break
        live, cur = live[go], nxt[go]
        hits, surf = trace(cur)
        hit = hits[:, 0].copy().view(np.int32) >= 0
        new = records(cs, hits, surf)
        new[:, 7] = (rec[live, 7] + hits[:, 1]).astype(F)
        rec[live[hit]] = new[hit]
        length[live[hit]] += 1
        live, cur, hits, surf = live[hit], cur[hit], hits[hit], surf[hit]
    return rec, length, classes


def aimed_rays(cs, count=96, seed=5):
    """Rays at the scene's first dielectric sphere that take the branches a random ray seldom takes: `count` from inside it towards
    its rim (impact parameter 0.75 ... 0.97 of the radius: total internal reflection for eta >= 1.34), `count` grazing its outside
    (0.995 ... 0.9995: fr >= 0.5) and `count` from inside it outwards (0 ... 0.5: refraction, leaving).  (3 * count, 8), tMin = eps,
    tMax = +inf."""
    tags = np.asarray(cs.materials, U) >> abi.MATERIAL_TAG_SHIFT
    sph = [i for i in range(len(cs.spheres)) if tags[i] == abi.MAT_DIELECTRIC]
    assert sph, "no glass sphere"
    c, r = cs.spheres[sph[0], 0:3].astype(np.float64), float(cs.spheres[sph[0], 3])
    rng = np.random.default_rng(seed)
    e1 = rng.normal(size=(3 * count, 3))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(e1, rng.normal(size=(3 * count, 3)))
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    b = np.concatenate([rng.uniform(0.75, 0.97, count), rng.uniform(0.995, 0.9995, count), rng.uniform(0.0, 0.5, count)]) * r
    back = np.concatenate([np.zeros(count), np.full(count, 1.2 * r), np.zeros(count)])
    rays = np.zeros((3 * count, 8), F)
    rays[:, 0:3], rays[:, 3:6] = c + b[:, None] * e1 - back[:, None] * e2, e2
    rays[:, 6], rays[:, 7] = KEPS, np.inf
    return rays


def query_rays(name="cbox"):
    """path_query_ref's ray set of the scene, as closest-hit rays, and the aimed rays behind it"""
    rays = np.array(P.ray_set(name))
    rays[:, 6], rays[:, 7] = KEPS, np.inf
    return np.concatenate([rays, aimed_rays(P.scene(name))])
