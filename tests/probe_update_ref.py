"""The reference of hj_update_probes' and hj_update_probe_visibility's blend: include/hijiki_hip.h's text ("Probe updates") restated in
numpy float32, one rounding per operation, in the stated order.  The fresh values are arguments - the bakes' own results, which
probe_ref and probe_vis_ref (or the GPU's bakes) supply; nothing of a bake is restated here.  Every comparison is written the way the
header writes it, so that a NaN falls where the header says it falls: `a > b` is False with a NaN on either side.

upd is a dict: first, num (the probe window), hysteresis, soft, hard (float32)."""
import numpy as np

import probe_ref as P
import probe_vis_ref as V
from hijiki_amd import abi

U, F = np.uint32, np.float32
SOFT_STEP = F(0.15)                                  # Majercik et al. 2019
BRANCHES = ("none", "soft", "hard", "old_invalid", "fresh_invalid", "nan_validity")


def update(first, num, hysteresis, soft=np.inf, hard=np.inf):
    return dict(first=int(first), num=int(num), hysteresis=F(hysteresis), soft=F(soft), hard=F(hard))


def abi_update(first_probe=0, num_probes=8, frame=0, frame_stride=1, hysteresis=0.5, change_soft=0.25, change_hard=0.8, flags=0):
    """an abi.ProbeUpdate for the raw entry points"""
    return abi.ProbeUpdate(first_probe, num_probes, frame, frame_stride, hysteresis, change_soft, change_hard, flags)


def frame_seed(seed, frame, frame_stride):
    """seed' of an update: seed + frame * frame_stride in uint32"""
    return (int(seed) + int(frame) * int(frame_stride)) & 0xFFFFFFFF


def mix(o, f, hh):
    """o * hh + f * (1 - hh) with 1 - hh formed once, the fresh value's bits where hh == 0 (hh broadcasts against o and f)"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = (F(1) - hh).astype(F)
        blended = ((o * hh).astype(F) + (f * g).astype(F)).astype(F)
    return np.where(hh == 0, f, blended).astype(F)


def blend_probes(old, fresh, upd, detail=False):
    """old, fresh: the whole volume, (n, 28) or (nz, ny, nx, 28) -> the volume after hj_update_probes, old's shape; every record
    outside the window is old's, bit for bit.  detail: -> (new, hh (num,) float32, {branch: a mask over the window's rows})"""
    old = np.ascontiguousarray(old, F)
    out = old.reshape(-1, P.WORDS).copy()
    fr = np.ascontiguousarray(fresh, F).reshape(-1, P.WORDS)
    a, b = upd["first"], upd["first"] + upd["num"]
    assert 0 <= a <= b <= len(out) == len(fr)
    O, Fr = out[a:b].copy(), fr[a:b]
    h = F(upd["hysteresis"])
    with np.errstate(invalid="ignore", over="ignore"):
        old_ok, fresh_ok = O[:, 27] > F(0), Fr[:, 27] > F(0)             # (a NaN compares false)
        keep = old_ok & fresh_ok
        d = np.fmax(np.fmax(np.abs(Fr[:, 0] - O[:, 0]), np.abs(Fr[:, 1] - O[:, 1])), np.abs(Fr[:, 2] - O[:, 2])).astype(F)
        m = np.fmax(np.fmax(np.abs(O[:, 0]), np.abs(O[:, 1])), np.abs(O[:, 2])).astype(F)
        hard = keep & (d > (upd["hard"] * m).astype(F))
        soft = keep & ~hard & (d > (upd["soft"] * m).astype(F))
    hh = np.where(keep, h, F(0)).astype(F)
    hh = np.where(hard, F(0), hh).astype(F)
    hh = np.where(soft, np.fmax(h - SOFT_STEP, F(0)), hh).astype(F)
    new = Fr.copy()                                                      # word 27: the fresh validity
    new[:, 0:27] = mix(O[:, 0:27], Fr[:, 0:27], hh[:, None])
    out[a:b] = new
    out = out.reshape(old.shape)
    if not detail:
        return out
    nan_valid = np.isnan(O[:, 27]) | np.isnan(Fr[:, 27])
    masks = dict(none=keep & ~hard & ~soft, soft=soft, hard=hard, nan_validity=nan_valid, old_invalid=~old_ok & ~nan_valid,
                 fresh_invalid=old_ok & ~fresh_ok & ~nan_valid)
    return out, hh, masks


def blend_atlas(old, fresh, res, upd):
    """old, fresh: the whole atlas, (n, T, T, 2) or (nz, ny, nx, T, T, 2) -> the atlas after hj_update_probe_visibility, old's shape.
    Per probe of the window the interior is mixed, then every texel - border included - is the new value of the interior texel
    probe_vis_ref.border_source names; the old border is never read."""
    T = res + 2
    old = np.ascontiguousarray(old, F)
    out = old.reshape(-1, T, T, 2).copy()
    fr = np.ascontiguousarray(fresh, F).reshape(-1, T, T, 2)
    a, b = upd["first"], upd["first"] + upd["num"]
    assert 0 <= a <= b <= len(out) == len(fr)
    interior = mix(out[a:b, 1:-1, 1:-1, :], fr[a:b, 1:-1, 1:-1, :], F(upd["hysteresis"])).reshape(b - a, res * res, 2)
    out[a:b] = interior[:, V.border_source(res), :].reshape(b - a, T, T, 2)
    return out.reshape(old.shape)
