"""hj_render_probe_lit restated in numpy, float32 throughout, from three things that exist already: follow_ref's chain of a sample
(continue_rays alternated with a trace the caller brings - on the GPU hj_trace_rays itself, without one the oracle's intersect), the
look-up restatements (probe_ref.sample, probe_vis_ref.sample, probe_place_ref.sample) and the compose and block-order sum of
include/hijiki_hip.h: L = Le + (albedo * E) * (1 / pi), summed per pixel block by block."""
import numpy as np

import aov_ref as A
import follow_ref as R
import path_query_ref as P
import probe_place_ref as PP
import probe_ref as PR
import probe_vis_ref as PV
from hijiki_amd import abi

U, F = np.uint32, np.float32
INV_PI = F(0.318309886)                               # the shade stage's 1.0f / 3.14159274f: the same bits
DIFFUSE, SPECULAR, MISS = 0, 1, 2
assert F(1) / F(3.14159274) == INV_PI


def camera_rays(cs, blocks):
    """the camera rays of every sample of `blocks`, block after block, row by row: tMin = eps, tMax = +inf"""
    rays = np.concatenate([P.camera_rays(cs, b) for b in blocks]) if len(blocks) else np.zeros((0, 8), F)
    rays[:, 6], rays[:, 7] = P.KEPS, np.inf
    return rays


def chains(cs, rays, max_follow, trace):
    """follow_ref.followed_records' loop, keeping what the compose needs of each chain's end -> dict(kind (n,): DIFFUSE, SPECULAR (the
    cap cut the chain on a mirror or a dielectric) or MISS (nothing hit, from the camera or after leaving a specular surface);
    points (n, 8): (p, n, 0, 0) at the last hit; albedo, emission (n, 3): the material record's at the last hit; direction (n, 3):
    the last segment's; length (n,): continuations taken; left (n,): MISS behind a specular surface)"""
    n = len(rays)
    hits, surf = trace(rays)
    last_hits, last_surf = np.array(hits, F), np.array(surf, F)
    direction = np.array(rays[:, 3:6], F)
    length, left = np.zeros(n, np.int32), np.zeros(n, bool)
    live, cur = np.arange(n), np.asarray(rays, F)
    for _ in range(max_follow):
        nxt, cls = R.continue_rays(cs, cur, hits, surf)
        go = cls != R.END
        if not go.any():
            break
        live, cur = live[go], nxt[go]
        hits, surf = trace(cur)
        last_hits[live], last_surf[live], direction[live] = hits, surf, cur[:, 3:6]
        length[live] += 1
        hit = hits[:, 0].copy().view(np.int32) >= 0
        left[live[~hit]] = True
        live, cur, hits, surf = live[hit], cur[hit], hits[hit], surf[hit]
    mat = A.materials(cs, cs.textures, last_hits[:, 0].copy().view(np.int32), last_surf[:, 6], last_surf[:, 7])
    word = mat.view(U)[:, 3]
    miss = word == A.MISS
    tag = word >> abi.MATERIAL_TAG_SHIFT
    kind = np.where(miss, MISS, np.where((tag == abi.MAT_MIRROR) | (tag == abi.MAT_DIELECTRIC), SPECULAR, DIFFUSE)).astype(np.int8)
    points = np.zeros((n, 8), F)
    points[:, 0:6] = last_surf[:, 0:6]
    return dict(kind=kind, points=points, albedo=mat[:, 0:3].copy(), emission=mat[:, 4:7].copy(), direction=direction, length=length, left=left)


def lookup(d, volume, v=None, atlas=None, placement=None):
    """the look-up hj_probe_lighting selects -> a function of (m, 8) points -> (m, 4)"""
    if v is None:
        assert atlas is None and placement is None
        return lambda pts: PR.sample(d, volume, pts)
    if placement is None:
        return lambda pts: PV.sample(d, v, volume, atlas, pts)
    return lambda pts: PP.sample(d, v, volume, atlas, pts, placement)


def compose(ch, look, env=None):
    """chains() -> L (n, 3) float32.  look: points -> the look-up's records; env: directions (m, 3) -> radiance (m, 3), None: no
    environment is uploaded"""
    n = len(ch["kind"])
    L = np.zeros((n, 3), F)
    dif = ch["kind"] == DIFFUSE
    if dif.any():
        E = np.asarray(look(ch["points"][dif]), F)[:, 0:3]
        with np.errstate(invalid="ignore", over="ignore"):
            L[dif] = (ch["emission"][dif] + ((ch["albedo"][dif] * E).astype(F) * INV_PI).astype(F)).astype(F)
    spec = ch["kind"] == SPECULAR
    L[spec] = ch["emission"][spec]
    miss = ch["kind"] == MISS
    if env is not None and miss.any():
        L[miss] = np.asarray(env(ch["direction"][miss]), F)
    return L


def accumulate(width, height, blocks, L):
    """-> (height, width, 4): words 0..2 the float32 sums of L over a pixel's samples, block by block in the order of the list from +0;
    word 3 the count of its samples (aov_ref.accumulate: one text of the block order and of the samples that are dropped)"""
    rec = np.zeros((len(L), 12), F)
    rec[:, 0:3], rec[:, 3] = L, F(1)
    return np.ascontiguousarray(A.accumulate(width, height, blocks, rec)[..., 0:4])


def render(cs, blocks, width, height, max_follow, trace, look, env=None, detail=False):
    """hj_render_probe_lit -> (height, width, 4) [, the chains, L]"""
    ch = chains(cs, camera_rays(cs, blocks), max_follow, trace)
    L = compose(ch, look, env)
    img = accumulate(width, height, blocks, L)
    return (img, ch, L) if detail else img
