"""Reconstruction level: ONE pass of k_reconstruct (kernels/hj_reconstruct.h) with the per-tile block lists a render call builds for
it, through hj_debug_reconstruct, over fabricated samples - against oracle.reconstruct_block applied block by block in list order to
a copy of the initial framebuffer.  0 differing bits on every word; on touched pixels a NaN equals any NaN (x86 and the GPU
generate different default NaNs); untouched pixels - outside every block's rectangle extended by 2 and clipped to the image, a mask
this file computes itself - are compared as raw integers and against the initial framebuffer.

The initial framebuffer is a torch device tensor bound as the external framebuffer, filled with finite values, +-0, denormals,
+-inf and NaNs of distinct payloads (zeros where a family wants clean sums).  The case families (CASES) are geometry, filter
parameters, sample values, normals; then the round trip of a rendered block list and the refusals.  The tests without the gpu mark
assert the premises from the oracle alone, on the same case lists: every branch of the kernel is reached in a counted number of
taps, the NaN exception never does the comparing (at most one touched pixel in four of the oracle's result is a NaN where
non-finite values are injected, none is new elsewhere), and on the finite non-negative families the float64 restatement of the
shader (tests/golden/glsl_f64.py) agrees with the oracle within the tolerance tests/test_glsl_f64.py uses for this function."""
import collections
import ctypes as C
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import glsl_f64 as G  # noqa: E402
from hijiki_amd import abi, device, host  # noqa: E402

F, U = np.float32, np.uint32
FLT_MIN = float(np.finfo(F).tiny)
Case = collections.namedtuple("Case", "name family W H blocks samples stddev init inject f64")
CASES = {}
F64_NAMES = []              # the cases with finite non-negative samples and a filter float64 can follow


def bits(a):
    return np.ascontiguousarray(a, F).view(U)


def words(x):
    return np.ascontiguousarray(x, F).view(U)


def ulps(x, k):
    """The float32 k ulps above (k < 0: below) x."""
    return float((words([x]).astype(np.int64) + k).astype(U).view(F)[0])


def blk(W, H, ox, oy, dx, dy, off=(0.5, 0.5)):
    return abi.ImageBlock(id=0, seed=0, origin=(ox, oy), dimension=(dx, dy), original_dimension=(W, H), sample_offset=off)


def rand_samples(rng, b, scale=None):
    """Finite non-negative radiance, weight 1, unit normals, positive depth - what camera paths produce."""
    dy, dx = b.dimension[1], b.dimension[0]
    s = np.zeros((dy, dx, 8), F)
    s[..., 0:3] = rng.uniform(0.0, 4.0, (dy, dx, 3))
    s[..., 3] = 1.0
    if scale is not None:
        s[..., 0:4] *= scale
    n = rng.normal(size=(dy, dx, 3))
    s[..., 4:7] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    s[..., 7] = rng.uniform(0.5, 5.0, (dy, dx))
    return s


def case(name, family, W, H, blocks, stddev=0.5, init="mix", inject=False, f64=False, fill=None):
    """Registers a case; built on first use from a seed of its name alone.  fill(rng, i, block, samples): edits block i's samples."""
    def build():
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        bl = blocks(rng) if callable(blocks) else list(blocks)
        smp = []
        for i, b in enumerate(bl):
            s = rand_samples(rng, b)
            if fill is not None:
                s = fill(rng, i, b, s)
            smp.append(np.ascontiguousarray(s, F))
        return Case(name, family, W, H, bl, smp, stddev, init, inject, f64)
    assert name not in CASES
    CASES[name] = functools.lru_cache(maxsize=None)(build)
    if f64:
        F64_NAMES.append(name)


def get(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------------ geometry

SIZES = ((1, 1), (2, 2), (5, 5), (16, 16), (17, 19))
for _W, _H in ((1, 1), (15, 17), (16, 16), (17, 16), (33, 47), (200, 136)):
    # every size at the origin, then one that runs off the right and the bottom edge
    case(f"fb_{_W}x{_H}", "geometry", _W, _H,
         [blk(_W, _H, 0, 0, dx, dy, (0.3, 0.8)) for dx, dy in SIZES] + [blk(_W, _H, max(_W - 3, 0), max(_H - 3, 0), 5, 5, (0.6, 0.1))], f64=True)
for _o in (14, 15, 16, 17, 18):
    # around the tile boundary at 16: the body (14, 15), the apron only (16, 17) or nothing (18) reaches the tile before it, and
    # blocks that END at 12 .. 16 (origin _o - 6, 4 wide) do the same to the tile after it
    case(f"tile_boundary_{_o}", "geometry", 33, 47,
         [blk(33, 47, _o, 3, 2, 2), blk(33, 47, 3, _o, 2, 2, (0.2, 0.7)), blk(33, 47, _o, _o, 1, 1), blk(33, 47, _o - 6, _o - 6, 4, 4, (0.9, 0.4)),
          blk(33, 47, _o + 16 - 6, _o - 6, 4, 5)], f64=True)
case("four_tile_corner", "geometry", 33, 47,
     [blk(33, 47, 14, 14, 5, 5), blk(33, 47, 16, 16, 1, 1, (0.1, 0.1)), blk(33, 47, 15, 15, 1, 1), blk(33, 47, 15, 15, 2, 2, (0.7, 0.3)),
      blk(33, 47, 8, 8, 17, 19), blk(33, 47, 31, 31, 1, 1), blk(33, 47, 32, 32, 1, 1)], f64=True)
case("beyond_the_edge", "geometry", 33, 47,
     [blk(33, 47, 33 + k, 5 + 7 * k, 5, 5) for k in range(3)] + [blk(33, 47, 5 + 7 * k, 47 + k, 5, 5, (0.2, 0.9)) for k in range(3)]
     + [blk(33, 47, 33 + k, 47 + k, 1, 1) for k in range(3)] + [blk(33, 47, 28, 40, 17, 19)], f64=True)
case("nothing_in_image", "geometry", 33, 47, [blk(33, 47, 35, 5, 5, 5), blk(33, 47, 5, 49, 16, 16), blk(33, 47, 35, 49, 1, 1)], f64=True)
case("block_128", "geometry", 200, 136, [blk(200, 136, 40, 5, 128, 128, (0.3, 0.8)), blk(200, 136, 150, 100, 128, 128)], f64=True)
case("sparse_tiles", "geometry", 200, 136,
     [blk(200, 136, 3, 3, 5, 5), blk(200, 136, 100, 60, 17, 19, (0.8, 0.2)), blk(200, 136, 190, 130, 16, 16), blk(200, 136, 60, 120, 2, 2),
      blk(200, 136, 176, 0, 1, 1)], f64=True)


def _stack(rng):
    return [blk(33, 47, int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(rng.integers(3, 13)), int(rng.integers(3, 13)),
                (float(F(rng.uniform(0, 1))), float(F(rng.uniform(0, 1))))) for _ in range(40)]


def _spread(rng, i, b, s):
    s[..., 0:4] *= (10.0 ** rng.uniform(-6, 6, s.shape[:2]))[..., None].astype(F)
    return s


case("stack_40", "geometry", 33, 47, _stack, init="zeros", f64=True, fill=_spread)
case("stack_40_reversed", "geometry", 33, 47, lambda rng: get("stack_40").blocks[::-1], init="zeros", f64=True,
     fill=lambda rng, i, b, s: get("stack_40").samples[39 - i])

# ---------------------------------------------------------------------------------------- filter parameters

FILTER_BLOCKS = ((8, 8, 17, 19), (14, 14, 5, 5), (0, 0, 16, 16), (30, 44, 2, 2))


def filter_blocks(off):
    return [blk(33, 47, ox, oy, dx, dy, off) for ox, oy, dx, dy in FILTER_BLOCKS]


# (name, value, in float64's reach): 2 sigma^2 leaves float32's range for the last four - the float32 texts then see a gaussFac of
# -inf or -0, which the float64 restatement does not model
STDDEVS = (("0.25", 0.25, True), ("0.5", 0.5, True), ("1", 1.0, True), ("3", 3.0, True), ("1e-3", 1e-3, True), ("1e-20", 1e-20, False),
           ("1e20", 1e20, False), ("inf", float("inf"), False), ("min_normal", FLT_MIN, False))
for _n, _s, _ok in STDDEVS:
    case(f"stddev_{_n}", "filter", 33, 47, filter_blocks((0.3, 0.8)), stddev=_s, f64=_ok)
    case(f"stddev_{_n}_centred", "filter", 33, 47, filter_blocks((0.5, 0.5)), stddev=_s, f64=_ok)
OFFSETS = (0.0, 0.5, 0.99, 1.0, -0.5, 2.5, 3.0, float("nan"))
for _i, _a in enumerate(OFFSETS):
    for _b in (_a, OFFSETS[(3 * _i + 1) % 8]):
        case(f"offset_{_a}_{_b}", "filter", 33, 47, filter_blocks((_a, _b)), f64=_a == _a and _b == _b)
# stddev 0.5: a tap at distance exactly 2 has w == 0 and is kept; one and two ulps each side of the offsets that put one there
for _a, _b in ((0.5, 0.5), (2.5, 0.5), (0.5, 2.5), (-0.5, 0.5), (0.5, -1.5)):
    for _k in (-2, -1, 1, 2):
        case(f"w_zero_{_a}_{_b}_{_k:+d}x", "filter", 33, 47, filter_blocks((ulps(_a, _k), _b)), f64=True)
        case(f"w_zero_{_a}_{_b}_{_k:+d}y", "filter", 33, 47, filter_blocks((_a, ulps(_b, _k))), f64=True)
case("w_zero_0.5_-1.5", "filter", 33, 47, filter_blocks((0.5, -1.5)), f64=True)

# ------------------------------------------------------------------------------------------ sample values

VALUE_BLOCKS = [blk(33, 47, 8, 8, 17, 19), blk(33, 47, 20, 30, 16, 16, (0.3, 0.8)), blk(33, 47, 0, 40, 5, 5)]


def _binades(rng, i, b, s):
    e = rng.choice(np.arange(-149, 121, 5), s.shape[:2] + (4,))            # (sums of 25 taps stay finite below 2^121)
    s[..., 0:4] = (np.exp2(e.astype(np.float64)) * rng.choice([1.0, -1.0], e.shape)).astype(F)
    return s


def _sprinkle(values, density, channels=(0, 1, 2, 3)):
    def fill(rng, i, b, s):
        hit = rng.random(s.shape[:2]) < density
        ch = rng.choice(channels, s.shape[:2])
        val = rng.choice(np.asarray(values, F), s.shape[:2])
        yy, xx = np.nonzero(hit)
        s[yy, xx, ch[yy, xx]] = val[yy, xx]
        return s
    return fill


def _inf_pairs(rng, i, b, s):
    y, x, c = int(rng.integers(0, s.shape[0])), int(rng.integers(0, s.shape[1] - 1)), int(rng.integers(0, 4))
    s[y, x, c], s[y, x + 1, c] = np.inf, -np.inf
    return s


case("value_binades", "values", 33, 47, VALUE_BLOCKS, fill=_binades)
case("value_zeros", "values", 33, 47, VALUE_BLOCKS, fill=_sprinkle([0.0, -0.0], 0.3), f64=True)
case("value_negative", "values", 33, 47, VALUE_BLOCKS, fill=lambda rng, i, b, s: s * rng.choice([F(1), F(-1)], s.shape))
case("value_inf", "values", 33, 47, VALUE_BLOCKS, inject=True, fill=_sprinkle([np.inf, -np.inf], 0.03))
case("value_inf_off_centre", "values", 33, 47, [blk(33, 47, 8, 8, 17, 19, (0.3, 0.8))], inject=True, fill=_sprinkle([np.inf, -np.inf], 0.03))
case("value_nan_rgb", "values", 33, 47, VALUE_BLOCKS, inject=True, fill=_sprinkle([np.nan], 0.1, (0, 1, 2)))
case("value_nan_weight", "values", 33, 47, VALUE_BLOCKS, inject=True, fill=_sprinkle([np.nan], 0.1, (3,)))
case("value_inf_pairs", "values", 33, 47, VALUE_BLOCKS, inject=True, fill=_inf_pairs)

# ------------------------------------------------------------------------------------------------- normals

NORMAL_BLOCKS = [blk(33, 47, 2 + 6 * k, 3 + 8 * k, 9, 9, (0.4, 0.6)) for k in range(5)]
ULP_SCALES = (1.0, 2.0 ** -40, 2.0 ** -41, 2.0 ** -47, 2.0 ** -60)


def _normals(make):
    def fill(rng, i, b, s):
        s[..., 4:7] = make(rng, i, s.shape[:2])
        return s
    return fill


def _ulp_apart(rng, i, shape):
    """One base normal per block, scaled so that a step of 1 or 2 ulps in one component squares to 0 (2^-60), a denormal (2^-47,
    2^-41), the smallest normals (2^-40) or an ordinary number (1)."""
    base = words(np.asarray([0.6, 0.8, 1.0]) * ULP_SCALES[i]).astype(np.int64)
    w = np.broadcast_to(base, shape + (3,)).copy()
    comp = rng.integers(0, 3, shape)
    step = rng.integers(-2, 3, shape)
    yy, xx = np.indices(shape)
    w[yy, xx, comp] += step
    return w.astype(U).view(F)


def _signed_zeros(rng, i, shape):
    n = rng.choice(np.asarray([0.0, -0.0], F), shape + (3,))
    n[..., i % 3] = 1.0
    return n


def _lengths(rng, i, shape):
    n = rng.normal(size=shape + (3,))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return (n * 10.0 ** rng.uniform(-25, 20, shape)[..., None]).astype(F)


def _nan_taps(rng, i, shape):
    n = rng.normal(size=shape + (3,)).astype(F)
    hit = rng.random(shape) < 0.05
    yy, xx = np.nonzero(hit)
    n[yy, xx, rng.integers(0, 3, len(yy))] = np.nan
    return n


def _nan_centre(rng, i, shape):
    n = np.broadcast_to(np.asarray([0.0, 0.0, 1.0], F), shape + (3,)).copy()
    n[shape[0] // 2, shape[1] // 2, i % 3] = np.nan
    return n


case("normal_equal", "normals", 33, 47, NORMAL_BLOCKS, f64=True, fill=_normals(lambda rng, i, shape: np.broadcast_to(np.asarray([0.0, 0.6, 0.8], F), shape + (3,))))
case("normal_ulp_apart", "normals", 33, 47, NORMAL_BLOCKS, f64=True, fill=_normals(_ulp_apart))
case("normal_signed_zeros", "normals", 33, 47, NORMAL_BLOCKS, f64=True, fill=_normals(_signed_zeros))
case("normal_random", "normals", 33, 47, NORMAL_BLOCKS + [blk(33, 47, 0, 0, 33, 47)], f64=True)
case("normal_lengths", "normals", 33, 47, NORMAL_BLOCKS, fill=_normals(_lengths))
case("normal_nan_tap", "normals", 33, 47, NORMAL_BLOCKS, inject=True, fill=_normals(_nan_taps))
case("normal_nan_centre", "normals", 33, 47, NORMAL_BLOCKS + [blk(33, 47, 20, 3, 1, 1), blk(33, 47, 26, 3, 5, 5)], inject=True, fill=_normals(_nan_centre))
case("normal_apron", "normals", 33, 47, [blk(33, 47, 16, 16, 1, 1), blk(33, 47, 3, 30, 2, 2), blk(33, 47, 20, 5, 5, 5)], f64=True,
     fill=_normals(lambda rng, i, shape: np.broadcast_to(np.asarray([0.3, -0.4, 0.5], F) * (i + 1), shape + (3,))))

NAMES = tuple(CASES)


# --------------------------------------------------------------------------------------- the two sides' inputs

def initial(c):
    """The framebuffer a case starts from, (H, W, 4) float32, a function of its name."""
    if c.init == "zeros":
        return np.zeros((c.H, c.W, 4), F)
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) ^ 0x5EED)
    n = c.H * c.W * 4
    w = words((rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F)).copy()
    kind = rng.random(n)
    idx = np.arange(n, dtype=np.int64)
    sign = (rng.integers(0, 2, n).astype(U) << U(31))
    w = np.where(kind < 0.05, sign, w)                                                     # +-0
    w = np.where((kind >= 0.05) & (kind < 0.10), sign | rng.integers(1, 0x800000, n).astype(U), w)   # denormals
    w = np.where((kind >= 0.10) & (kind < 0.13), sign | U(0x7F800000), w)                # +-inf
    w = np.where((kind >= 0.13) & (kind < 0.15), sign | U(0x7FC00000) | (idx & 0x3FFFFF).astype(U), w)   # quiet NaNs, the word's index as payload
    return w.astype(U).view(F).reshape(c.H, c.W, 4)


def touched_mask(c):
    """Pixels inside some block's rectangle extended by 2 and clipped to the image: how many blocks reach each."""
    t = np.zeros((c.H, c.W), np.int32)
    for b in c.blocks:
        x0, y0 = max(b.origin[0] - 2, 0), max(b.origin[1] - 2, 0)
        x1, y1 = min(b.origin[0] + b.dimension[0] + 2, c.W), min(b.origin[1] + b.dimension[1] + 2, c.H)
        if x0 < x1 and y0 < y1:
            t[y0:y1, x0:x1] += 1
    return t


def opts_of(c):
    o = abi.RenderOpts.default()
    o.recon_stddev = c.stddev
    return o


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's framebuffer of a case: reconstruct_block block by block, in list order, on a copy of the initial one."""
    from oracle import hj_oracle
    c = get(name)
    acc = initial(c).copy()
    for b, s in zip(c.blocks, c.samples):
        hj_oracle.reconstruct_block(b, s, acc, opts_of(c))
    acc.setflags(write=False)
    return acc


def differing(c, got, want, init):
    """Words that differ under the rule of this file, and untouched words that are not the initial framebuffer's."""
    t = touched_mask(c) > 0
    same = bits(got) == bits(want)
    same |= np.isnan(got) & np.isnan(want) & t[..., None]
    kept = (bits(got) == bits(init)) | t[..., None]
    return ~same, ~kept


def walk(c, oracle):
    """The taps of a case, counted by the branch they take, with the oracle's own primitives (hjo_recon_gauss, dot3 and exp of
    hjo_num_batch) on numpy arrays."""
    L = oracle.lib()
    n = collections.Counter()
    t = touched_mask(c)
    n["touched"] = int((t > 0).sum())
    n["touched_3"] = int((t >= 3).sum())
    tiles = [(t[y:y + 16, x:x + 16] > 0).any() for y in range(0, c.H, 16) for x in range(0, c.W, 16)]
    n["tiles_empty"] = len(tiles) - sum(tiles)
    n["tiles_apron_only"] = 0
    with np.errstate(all="ignore"):
        for b, smp in zip(c.blocks, c.samples):
            Dx, Dy, ox, oy = b.dimension[0], b.dimension[1], b.origin[0], b.origin[1]
            ly, lx = np.mgrid[-2:Dy + 2, -2:Dx + 2]
            inimg = (lx + ox >= 0) & (lx + ox < c.W) & (ly + oy >= 0) & (ly + oy < c.H)
            inblk = (lx >= 0) & (lx < Dx) & (ly >= 0) & (ly < Dy)
            for ty in range(0, c.H, 16):
                for tx in range(0, c.W, 16):
                    here = inimg & (lx + ox >= tx) & (lx + ox < tx + 16) & (ly + oy >= ty) & (ly + oy < ty + 16)
                    n["tiles_apron_only"] += int(here.any() and not (here & inblk).any())
            pad = np.zeros((Dy + 8, Dx + 8, 8), F)
            pad[4:4 + Dy, 4:4 + Dx] = smp
            valid = np.zeros((Dy + 8, Dx + 8), bool)
            valid[4:4 + Dy, 4:4 + Dx] = True
            nc = pad[2:Dy + 6, 2:Dx + 6, 4:7]
            for dx in range(-2, 3):
                for dy in range(-2, 3):
                    w = F(L.hjo_recon_gauss(dx, dy, b.sample_offset[0], b.sample_offset[1], c.stddev, 2))
                    sel = valid[2 + dy:Dy + 6 + dy, 2 + dx:Dx + 6 + dx] & inimg
                    k = int(sel.sum())
                    n["taps"] += k
                    if k == 0:
                        continue
                    if w < 0:
                        n["w_negative"] += k
                        n["w_negative_tiny"] += k if w > -1e-6 else 0
                        continue
                    n["w_zero"] += k if w == 0 else 0
                    n["w_positive_tiny"] += k if 0 < w < 1e-6 else 0
                    n["w_nan"] += k if w != w else 0
                    tap = pad[2 + dy:Dy + 6 + dy, 2 + dx:Dx + 6 + dx][sel]
                    no = tap[:, 4:7] - nc[sel]
                    dn = oracle.num_batch("dot3", words(np.concatenate([no, no], axis=1)))[:, 0].view(F) * F(2)
                    e = oracle.num_batch("exp", words(-dn))[:, 0].view(F)
                    v = (w * e)[:, None] * tap[:, 0:4]
                    n["dn_zero"] += int((dn == 0).sum())
                    n["dn_zero_unequal"] += int(((dn == 0) & (words(no) << U(1) != 0).any(axis=1)).sum())   # underflow, not equal normals
                    n["dn_signed_zero"] += int(((dn == 0) & (words(tap[:, 4:7]) != words(nc[sel])).any(axis=1) & (no == 0).all(axis=1)).sum())
                    n["dn_denormal"] += int(((dn > 0) & (dn < FLT_MIN)).sum())
                    n["dn_small_normal"] += int(((dn >= FLT_MIN) & (dn < 16 * FLT_MIN)).sum())
                    n["dn_inf"] += int(np.isinf(dn).sum())
                    n["dn_nan"] += int(np.isnan(dn).sum())
                    n["nan_tap"] += int(np.isnan(v).any(axis=1).sum())
                    n["nan_one_channel"] += int((np.isnan(v).sum(axis=1) == 1).sum())
                    n["zero_times_inf"] += int((np.isinf(tap[:, 0:4]).any(axis=1) & (w * e == 0)).sum())
                    n["apron_centre"] += int((~inblk[sel]).sum())
                    n["apron_centre_normal"] += int((~inblk[sel] & (tap[:, 4:7] != 0).any(axis=1)).sum())
    return n


# ------------------------------------------------------------------------------------------------ premises (no GPU)

def test_case_lists_hold_what_the_issue_names():
    for wh in ((1, 1), (15, 17), (16, 16), (17, 16), (33, 47), (200, 136)):
        assert any((get(n).W, get(n).H) == wh for n in NAMES), wh
    dims = {(b.dimension[0], b.dimension[1]) for n in NAMES for b in get(n).blocks}
    assert {(1, 1), (2, 2), (5, 5), (16, 16), (17, 19), (128, 128)} <= dims
    assert {get(n).stddev for n in NAMES} >= {0.25, 0.5, 1.0, 3.0, 1e-3, 1e-20, 1e20, float("inf"), FLT_MIN}
    offs = [b.sample_offset[0] for n in NAMES for b in get(n).blocks] + [b.sample_offset[1] for n in NAMES for b in get(n).blocks]
    for v in OFFSETS:
        assert any(o == F(v) or (o != o and v != v) for o in offs), v
    assert all(len(get(n).blocks) <= abi.RECON_MAX_BLOCKS for n in NAMES) and len(get("stack_40").blocks) == 40
    assert all(max(get(n).W, get(n).H) <= 200 for n in NAMES)
    a, b = get("stack_40"), get("stack_40_reversed")
    assert all(bytes(x) == bytes(y) for x, y in zip(a.blocks, b.blocks[::-1])) and all((x == y).all() for x, y in zip(a.samples, b.samples[::-1]))
    mags = np.concatenate([s[..., 0:3].ravel() for s in a.samples])
    assert mags.min() < 1e-4 and mags.max() > 1e5
    # the order of the 40 is visible: the reversed list gives other bits
    assert (bits(expected("stack_40")) != bits(expected("stack_40_reversed"))).sum() >= 100
    # the initial framebuffer holds every kind of word, NaNs with distinct payloads
    w = bits(initial(get("four_tile_corner"))).ravel()
    f = w.view(F)
    nan = w[np.isnan(f)]
    assert len(nan) >= 20 and len(np.unique(nan)) == len(nan)
    assert (w == 0).any() and (w == 0x80000000).any() and (f == np.inf).any() and (f == -np.inf).any()
    assert ((w & 0x7F800000 == 0) & (w & 0x7FFFFF != 0)).sum() >= 20


@pytest.fixture(scope="module")
def counts(oracle):
    return {n: walk(get(n), oracle) for n in NAMES}


def test_every_branch_is_reached_in_counted_taps(counts):
    total = collections.Counter()
    for n in NAMES:
        total.update(counts[n])
    print({k: total[k] for k in sorted(total)})
    for key, least in (("w_negative", 10000), ("w_zero", 1000), ("w_negative_tiny", 100), ("w_positive_tiny", 100), ("w_nan", 100),
                       ("nan_tap", 1000), ("nan_one_channel", 100), ("zero_times_inf", 10), ("dn_zero", 10000), ("dn_zero_unequal", 100),
                       ("dn_signed_zero", 100), ("dn_denormal", 100), ("dn_small_normal", 10), ("dn_inf", 100), ("dn_nan", 100),
                       ("apron_centre", 10000), ("apron_centre_normal", 10000), ("touched_3", 500), ("tiles_empty", 50), ("tiles_apron_only", 20)):
        assert total[key] >= least, (key, total[key])
    # where each family claims its branch
    assert counts["stddev_0.5_centred"]["w_zero"] >= 100 and counts["w_zero_0.5_-1.5"]["w_zero"] >= 100
    for n in NAMES:
        if n.startswith("w_zero_") and n[-1] in "xy":
            assert counts[n]["w_negative_tiny"] + counts[n]["w_positive_tiny"] + counts[n]["w_zero"] >= 100, n
    assert counts["offset_nan_nan"]["w_nan"] == counts["offset_nan_nan"]["taps"] > 0
    u = counts["normal_ulp_apart"]
    assert min(u["dn_zero_unequal"], u["dn_denormal"], u["dn_small_normal"]) >= 10 and u["dn_zero"] > u["dn_zero_unequal"]
    assert counts["normal_signed_zeros"]["dn_signed_zero"] >= 100 and counts["normal_lengths"]["dn_inf"] >= 100
    assert counts["normal_nan_tap"]["dn_nan"] >= 100 and counts["normal_nan_centre"]["dn_nan"] >= 100
    assert counts["value_nan_rgb"]["nan_one_channel"] >= 100 and counts["value_nan_weight"]["nan_one_channel"] >= 100
    assert counts["value_inf"]["zero_times_inf"] >= 10
    assert counts["stack_40"]["touched_3"] >= 100 and counts["sparse_tiles"]["tiles_empty"] >= 50
    assert counts["nothing_in_image"]["touched"] == 0 and counts["nothing_in_image"]["taps"] == 0
    assert counts["beyond_the_edge"]["tiles_apron_only"] >= 4
    for o in (16, 17):
        assert counts[f"tile_boundary_{o}"]["tiles_apron_only"] >= 2, o
    assert counts["fb_1x1"]["touched"] == 1 and counts["fb_15x17"]["touched"] == 15 * 17


@pytest.mark.parametrize("name", NAMES)
def test_nan_exception_does_not_do_the_comparing(name, oracle):
    c = get(name)
    init, want = initial(c), expected(name)
    t = touched_mask(c) > 0
    nan_px = np.isnan(want).any(axis=-1) & t
    if c.inject:
        assert nan_px.sum() * 4 <= t.sum(), (int(nan_px.sum()), int(t.sum()))
    else:
        assert not (np.isnan(want) & ~np.isnan(init)).any()
    assert (bits(want)[~t] == bits(init)[~t]).all()                                      # the oracle leaves untouched pixels alone


@pytest.mark.parametrize("name", F64_NAMES)
def test_float64_restatement_agrees_where_samples_are_finite_and_non_negative(name, oracle):
    """The independent check that the oracle is right where the GPU is held to it, stddev != 0.5 included.  Left out: non-finite or
    negative samples, NaN offsets, and the filters whose 2 sigma^2 or gaussFac leaves float32's range (STDDEVS)."""
    c = get(name)
    a32, a64 = np.zeros((c.H, c.W, 4), F), np.zeros((c.H, c.W, 4))
    top = 0.0
    for b, s in zip(c.blocks, c.samples):
        assert np.isfinite(s).all() and (s[..., 0:4] >= 0).all()
        top = max(top, float(s[..., 0:4].max()))
        oracle.reconstruct_block(b, s, a32, opts_of(c))
        G.reconstruct_block(b, s.astype(np.float64), a64, stddev=float(F(c.stddev)))
    np.testing.assert_allclose(a32, a64, rtol=2e-5, atol=1e-6 * top)


# ------------------------------------------------------------------------------------------------------- the GPU

@pytest.fixture(scope="module")
def recon_renderer():
    """A context of this file's own: its framebuffer is a tensor that does not outlive the test."""
    r = device.Renderer(0)
    yield r
    r.close()


def run_on_device(r, c, init):
    import torch
    fb = torch.empty((c.H, c.W, 4), dtype=torch.float32, device=f"cuda:{r.device}")
    r.create_framebuffer(c.W, c.H, fb.data_ptr())                                        # (clears it)
    fb.copy_(torch.from_numpy(init))
    torch.cuda.synchronize()
    r.reconstruct(c.blocks, c.samples, opts_of(c))
    return fb.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_reconstruction_equals_oracle(name, recon_renderer, oracle):
    c = get(name)
    init, want = initial(c), expected(name)
    got = run_on_device(recon_renderer, c, init)
    bad, moved = differing(c, got, want, init)
    print(f"{name}: {bad.sum()} of {bad.size} words differ, {moved.sum()} untouched words moved")
    if bad.any():
        y, x, ch = (int(v[0]) for v in np.nonzero(bad))
        print(f"  first at ({x}, {y}) channel {ch}: device {bits(got)[y, x, ch]:08x} oracle {bits(want)[y, x, ch]:08x} initial {bits(init)[y, x, ch]:08x}")
    assert not bad.any() and not moved.any()


@pytest.mark.gpu
def test_round_trip_equals_the_rendered_frame(recon_renderer, cbox_small):
    """The samples of a real block list pushed through the probe in chunks give hj_render_blocks' framebuffer bit for bit."""
    import torch
    r = recon_renderer
    W, H = 200, 136
    blocks = host.make_blocks(W, H, 3, 2)
    r.upload_scene(cbox_small)
    r.create_framebuffer(W, H)
    r.render_blocks(blocks)
    want = r.read()
    smp = [r.samples(b) for b in blocks]
    fb = torch.empty((H, W, 4), dtype=torch.float32, device=f"cuda:{r.device}")
    r.create_framebuffer(W, H, fb.data_ptr())
    chunk = 5
    assert len(blocks) > 2 * chunk and chunk <= abi.RECON_MAX_BLOCKS
    for i in range(0, len(blocks), chunk):
        r.reconstruct(list(blocks[i:i + chunk]), smp[i:i + chunk])
    got = fb.cpu().numpy()
    assert np.isfinite(want).all() and (want[..., 3] > 0).all()
    assert (bits(got) == bits(want)).all(), int((bits(got) != bits(want)).sum())


@pytest.mark.gpu
def test_refusals(recon_renderer):
    L = device.lib()
    fp = C.POINTER(C.c_float)
    W, H = 33, 47
    smp = np.zeros(8 * 128 * 128, F)
    p = smp.ctypes.data_as(fp)
    one = (abi.ImageBlock * 1)(blk(W, H, 0, 0, 5, 5))
    many = (abi.ImageBlock * (abi.RECON_MAX_BLOCKS + 1))(*[blk(W, H, 0, 0, 1, 1)] * (abi.RECON_MAX_BLOCKS + 1))
    with device.Renderer(recon_renderer.device) as fresh:
        assert L.hj_debug_reconstruct(fresh._h, one, 1, None, p) == abi.HJ_ERR_STATE
        assert "hj_framebuffer_create" in L.hj_last_error(fresh._h).decode()
    recon_renderer.create_framebuffer(W, H)
    h = recon_renderer._h
    o = abi.RenderOpts.default()
    radius3, stddev0 = abi.RenderOpts.default(), abi.RenderOpts.default()
    radius3.recon_radius, stddev0.recon_stddev = 3, 0.0
    for args, status, text in (((None, 1, None, p), abi.HJ_ERR_INVALID, "null"), ((one, 1, None, None), abi.HJ_ERR_INVALID, "null"),
                               ((one, 0, None, p), abi.HJ_ERR_INVALID, "no blocks"),
                               ((many, len(many), None, p), abi.HJ_ERR_INVALID, "at most"),
                               (((abi.ImageBlock * 1)(blk(W, H, 0, 0, 0, 5)), 1, None, p), abi.HJ_ERR_INVALID, "dimension"),
                               (((abi.ImageBlock * 1)(blk(W, H, 0, 0, 5, 129)), 1, None, p), abi.HJ_ERR_INVALID, "dimension"),
                               (((abi.ImageBlock * 1)(blk(W + 1, H, 0, 0, 5, 5)), 1, None, p), abi.HJ_ERR_INVALID, "original_dimension"),
                               ((one, 1, C.byref(radius3), p), abi.HJ_ERR_UNSUPPORTED, "radius"),
                               ((one, 1, C.byref(stddev0), p), abi.HJ_ERR_INVALID, "recon_stddev")):
        assert L.hj_debug_reconstruct(h, *args) == status, (args, L.hj_last_error(h))
        assert text in L.hj_last_error(h).decode(), (text, L.hj_last_error(h))
    assert (recon_renderer.read() == 0).all()                                            # a refused call has written nothing
    assert L.hj_debug_reconstruct(h, one, 1, C.byref(o), p) == abi.HJ_OK
    assert L.hj_debug_reconstruct(None, one, 1, None, p) == abi.HJ_ERR_INVALID
