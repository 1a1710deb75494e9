"""hj_eval_materials and hj_render_aovs restated in numpy, float32 throughout: the tag dispatch of a material record, the
checkerboard, the image-texture look-up (texture_scenes.lookup, the restatement test_textures_host.py pins), a sample's 12-word AOV
record from hj_trace_rays' hit and surface records, and the sums of the records per pixel in block order."""
import numpy as np

import texture_scenes
from hijiki_amd import abi

U, F = np.uint32, np.float32
MISS = U(0xFFFFFFFF)


def tables(cs):
    """the compiled scene's material tables as arrays: diffuse (n, 3), checkerboard (n, 8: color_a, scale_u, color_b, scale_v),
    emissive (n, 3)"""
    d = cs.desc
    diffuse = np.array([list(d.diffuse[i].color) for i in range(d.num_diffuse)], F).reshape(-1, 3)
    cb = np.array([list(d.diffusecb[i].color_a) + [d.diffusecb[i].scale_u] + list(d.diffusecb[i].color_b) + [d.diffusecb[i].scale_v]
                   for i in range(d.num_diffusecb)], F).reshape(-1, 8)
    emissive = np.array([list(d.emissive[i].power) for i in range(d.num_emissive)], F).reshape(-1, 3)
    return diffuse, cb, emissive


def checkerboard(cb, idx, u, v):
    """shader/materials/diffusecb.glsl:6-13, every operation float32: (0.5 * u) / scale, x - floor(x), < 0.5, !="""
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fu = (F(0.5) * u).astype(F) / cb[idx, 3]
        fv = (F(0.5) * v).astype(F) / cb[idx, 7]
        fu = (fu - np.floor(fu)).astype(F)
        fv = (fv - np.floor(fv)).astype(F)
        a, b = fu < F(0.5), fv < F(0.5)
    return np.where((a != b)[:, None], cb[idx, 4:7], cb[idx, 0:3]).astype(F)


def materials(cs, textures, ids, u, v):
    """-> (n, 8) float32 material records for shape ids (int32; outside [0, shapes): a miss) at texture coordinates (u, v).
    textures: cs.textures - ([(width, height, filter, first_texel)], (texels, 4)) - or None for a scene without any."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    u, v = np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    n = len(ids)
    out = np.zeros((n, 8), F)
    words = out.view(U)
    mats = np.asarray(cs.materials, U)
    hit = (ids >= 0) & (ids < len(mats))
    words[~hit, 3] = MISS
    if not hit.any():
        return out
    word = np.zeros(n, U)
    word[hit] = mats[ids[hit]]
    words[hit, 3] = word[hit]
    tag, idx = word >> abi.MATERIAL_TAG_SHIFT, (word & U(abi.MATERIAL_INDEX_MASK)).astype(np.int64)
    diffuse, cb, emissive = tables(cs)
    m = hit & (tag == abi.MAT_DIFFUSE)
    out[m, 0:3] = diffuse[idx[m]]
    m = hit & (tag == abi.MAT_DIFFUSECBOARD)
    if m.any():
        out[m, 0:3] = checkerboard(cb, idx[m], u[m], v[m])
    m = hit & (tag == abi.MAT_DIFFUSE_TEXTURED)
    if m.any():
        table, texels = textures
        for t in sorted(set(idx[m].tolist())):
            W, H, filt, first = table[t]
            sel = m & (idx == t)
            out[sel, 0:3] = texture_scenes.lookup(texels[first:first + W * H].reshape(H, W, 4), filt, np.stack([u[sel], v[sel]], 1))
    m = hit & ((tag == abi.MAT_MIRROR) | (tag == abi.MAT_DIELECTRIC))
    out[m, 0:3] = F(1)
    m = hit & (tag == abi.MAT_EMISSIVE)
    out[m, 4:7] = emissive[idx[m]]
    return out


def block_samples(block, width, height):
    """(w, h) of a block's samples: local pixels below the block's dimension and below the image's size (render.glsl:152)"""
    return min(int(block.dimension[0]), width), min(int(block.dimension[1]), height)


def sample_records(cs, blocks, hits, surface):
    """-> (n, 12) float32: the AOV record of every sample of `blocks`, block after block, row by row inside a block, from the hit
    records (n, 4: shape id bits, t, u, v) and surface records (n, 16) hj_trace_rays gives for the samples' camera rays:
    albedo.rgb, 1 | n.xyz, t | emission.rgb, 1 - a miss: 0, 0, 0, 1 and eight zeros."""
    hits, surface = np.asarray(hits, F).reshape(-1, 4), np.asarray(surface, F).reshape(-1, 16)
    W, H = int(blocks[0].original_dimension[0]), int(blocks[0].original_dimension[1])
    assert len(hits) == len(surface) == sum(w * h for w, h in (block_samples(b, W, H) for b in blocks))
    ids = hits[:, 0].copy().view(np.int32)
    mat = materials(cs, cs.textures, ids, surface[:, 6], surface[:, 7])
    hit = mat.view(U)[:, 3] != MISS
    rec = np.zeros((len(hits), 12), F)
    rec[:, 0:3], rec[:, 3] = mat[:, 0:3], F(1)
    rec[hit, 4:7], rec[hit, 7] = surface[hit, 3:6], hits[hit, 1]
    rec[hit, 8:11], rec[hit, 11] = mat[hit, 4:7], F(1)
    return rec


def accumulate(width, height, blocks, records):
    """-> (height, width, 12) float32: pixel (origin + l) is the float32 sum of its samples' records, block by block in the order of
    the list, starting from +0; a sample whose pixel lies outside the image is dropped."""
    out = np.zeros((height, width, 12), F)
    at = 0
    for b in blocks:
        w, h = block_samples(b, width, height)
        rec = np.asarray(records[at:at + w * h], F).reshape(h, w, 12)
        at += w * h
        ox, oy = int(b.origin[0]), int(b.origin[1])
        x1, y1 = min(ox + w, width), min(oy + h, height)
        if x1 > ox and y1 > oy:
            out[oy:y1, ox:x1] = out[oy:y1, ox:x1] + rec[:y1 - oy, :x1 - ox]
    assert at == len(records)
    return out
