"""The followed AOV and followed motion kernels at their size and chain edges - the forms test_follow_gpu.py and
test_motion_follow_gpu.py never run - bit for bit against follow_ref and motion_follow_ref:
the tile scan of the motion rounds beyond one count a thread (257 and 516 tiles), a last tile of one live pixel, the side limit of
16384 and its refusal, the device-output form between sentinels; chains that take every continuation up to the cap with both mirrors
moved in `prev`; rounds of exactly 1, 64, 65, 100, 101 and 256 live chains under workgroup segments of 256, 64 and 100 entries, and
counts that shrink round by round down to 1; walk launches of 9, 5 + 4 and 2 + 2 + 2 + 2 + 1 blocks, the last one smaller than the
one before it; and hj_follow_specular on fabricated records at the dielectric branch's decision edges, on degenerate rays and hits,
and on the first and last id of every shape kind.
Every premise - a live count, a chain length, a straddled edge - is asserted on the reference before the GPU is asked, and held
without a GPU by test_follow_edges_host.py, which imports the builders below: importing this module needs no device.
The expected values are the restatements' over the oracle's trace, or, for "rich", over hj_trace_rays of a renderer without a switch."""
import ctypes as C
import functools

import numpy as np
import pytest

import aov_ref as A
import follow_ref as R
import motion_follow_ref as MF
import motion_ref as M
import path_query_ref as P
import temporal_ref as T
from closest_ref import cross3
from hijiki_amd import abi, device, host
from lightmap_ref import normalize3
from test_follow_gpu import _facing_mirrors, camera_rays, gpu_trace, same_bits
from test_motion_follow_gpu import _mirror_scene, _prev
from test_motion_gpu import _cameras, _moved
from test_walk_forms_gpu import SENTINEL, _scene_seen_from_inside

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
SWITCHES = ("HJ_TRACE_WG_RAYS", "HJ_TRACE_CHUNK", "HJ_GROUP_TILE", "HJ_PAIR_LEAVES")
EYE = T.camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 90.0)             # the camera of the scenes built here
PATCH_W, PATCH_H = 128, 16                                              # the patch scenes' image: one AOV block
PATCHES = {1: (1, 1), 64: (8, 8), 65: (13, 5), 100: (10, 10), 101: (101, 1), 256: (16, 16)}   # live chains: pixels (wide, high) that see the mirror
NESTED_W, NESTED_FOLLOW = 127, 4
SLOTS = 16384                                                           # sample slots of a block (kSlotsPerBlock): 64 compaction tiles


# ------------------------------------------------------------------------------------------------------------------------ scenes

def _centre_plane(W, H, z):
    """where the centre rays of EYE's W x H image cross the plane at z: (x of every column, y of every row), float64"""
    d = M.centre_rays(EYE, W, H)[:, 3:6].astype(np.float64).reshape(H, W, 3)
    p = d * (z / d[..., 2:3])
    return p[0, :, 0], p[:, 0, 1]


def _span(c, i0, a):
    """the interval that holds the centres c[i0 : i0 + a] and no other: its ends lie midway to the neighbours"""
    if len(c) == 1:
        return c[0] - 1.0, c[0] + 1.0
    step = c[1] - c[0]
    lo = 0.5 * (c[i0 - 1] + c[i0]) if i0 > 0 else c[0] - 0.5 * step
    hi = 0.5 * (c[i0 + a - 1] + c[i0 + a]) if i0 + a < len(c) else c[-1] + 0.5 * step
    return min(lo, hi), max(lo, hi)


def _walls(s):
    """a diffuse wall that fills the view at z = -4 and a diffuse quad behind the camera at z = +3, for a mirror to show"""
    s.set_camera((0, 0, 0), (0, 0, 0, 1), 90.0)
    s.add_quad((-40, -40, -4), (80, 0, 0), (0, 80, 0), s.add_diffuse((0.5, 0.5, 0.5)))
    s.add_quad((-40, -40, 3), (0, 80, 0), (80, 0, 0), s.add_diffuse((0.2, 0.6, 0.3)))


@functools.lru_cache(maxsize=None)
def patch_scene(live):
    """The walls and, at z = -2, a mirror quad cut from the pixel grid of the PATCH_W x PATCH_H image: it holds the centre rays of
    PATCHES[live] pixels in the middle of the image and ends midway to their neighbours.  Its chains end on the quad behind the
    camera after one continuation.  (quads 0, 1: the walls; 2: the mirror)"""
    a, b = PATCHES[live]
    xs, ys = _centre_plane(PATCH_W, PATCH_H, -2.0)
    (x0, x1), (y0, y1) = _span(xs, (PATCH_W - a) // 2, a), _span(ys, (PATCH_H - b) // 2, b)
    s = host.Scene()
    _walls(s)
    s.add_quad((x0, y0, -2), (x1 - x0, 0, 0), (0, y1 - y0, 0), s.add_mirror())
    return s.compile()


@functools.lru_cache(maxsize=None)
def nested_scene():
    """The walls and two facing mirror strips of one width, at z = -2 and behind the camera at z = +1, seen in a NESTED_W x 1 image.
    A centre ray of slope s meets the planes at 2 s, 5 s, 8 s, 11 s ...: a chain stays between the strips while that is inside
    their half width, so every round loses the outer chains.  The half width is 10.4 pixel slopes: 5.2, 2.08, 1.3 and 0.945 pixels
    beside the middle one stay in rounds 1 to 4 - 11, 5, 3 and 1 live chains (held by test_follow_edges_host.py)."""
    half = 10.4 * 2.0 / NESTED_W
    s = host.Scene()
    _walls(s)
    m = s.add_mirror()
    s.add_quad((-half, -1, -2), (2 * half, 0, 0), (0, 2, 0), m)
    s.add_quad((-half, -1, 1), (0, 2, 0), (2 * half, 0, 0), m)
    return s.compile()


@functools.lru_cache(maxsize=None)
def wide_mirror_scene():
    """test_motion_follow_gpu._mirror_scene(0) with a mirror that fills the view of a 1 x 16384 image as well: the fov spans the
    width, so such an image's centre rays fan out to a slope of 16384 and _mirror_scene's 20 x 20 mirror holds three of them.  The
    steep chains leave: the wall behind the camera is 80 x 80."""
    s = host.Scene()
    s.set_camera((0, 0, 0), (0, 0, 0, 1), 90.0)
    grey = s.add_diffuse((0.5, 0.5, 0.5))
    s.add_quad((-1e5, -1e5, -4), (2e5, 0, 0), (0, 2e5, 0), s.add_mirror())
    s.add_quad((-40, -40, 6), (80, 0, 0), (0, 80, 0), grey)
    s.add_quad((-5.0, -1.25, 2), (2.5, 0, 0), (0, 2.5, 0), grey)
    return s.compile()


def quads_moved(cs, seed=4):
    """prev for the scenes of quads alone: the camera translated, every quad moved"""
    return M.Prev(cs, _cameras(cs)["translated"], **_moved(cs, seed, ["quads"]))


def one_block(W, H, seed=3):
    """the W x H image as one block of one pass through the pixel centres"""
    b = abi.ImageBlock()
    b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:], b.sample_offset[:] = 0, seed, (0, 0), (W, H), (W, H), (0.5, 0.5)
    return [b]


def motion_rounds(det, max_follow):
    """the live pixels of every round of a followed motion image, from the restatement's chains"""
    return [int((det["count"] >= k).sum()) for k in range(1, max_follow + 1)]


def aov_rounds(classes):
    """the live chains of every round of followed_records"""
    return [int((c != R.END).sum()) for c in classes]


def expected_aovs(cs, W, H, blocks, max_follow, trace):
    """-> (the followed image, the live chains per round, the records)"""
    rec, _, classes = R.followed_records(cs, camera_rays(cs, blocks), max_follow, trace)
    return A.accumulate(W, H, blocks, rec), aov_rounds(classes), rec


def launch_blocks():
    """40 x 40 in blocks of 16 - nine blocks of 16384 slots each, the right and bottom ones 8 wide or high - with the 8 x 8 corner last:
    under HJ_TRACE_CHUNK = 2 blocks the last launch is that block alone, behind a launch of two blocks of 128 samples each"""
    out = []
    for oy in (0, 16, 32):
        for ox in (0, 16, 32):
            b = abi.ImageBlock()
            b.id, b.seed = len(out), 17 + 1000 * len(out)
            b.origin[:], b.dimension[:] = (ox, oy), (min(16, 40 - ox), min(16, 40 - oy))
            b.original_dimension[:], b.sample_offset[:] = (40, 40), (0.375, 0.625)
            out.append(b)
    assert len(out) == 9 and tuple(out[8].dimension) == (8, 8) and tuple(out[7].dimension) == (16, 8) and tuple(out[6].dimension) == (16, 8)
    return out


def launch_live(cs, blocks, trace, per_launch):
    """(samples, chains live in round 1) of every launch of `per_launch` blocks, from the reference"""
    out = []
    for c0 in range(0, len(blocks), per_launch):
        part = blocks[c0:c0 + per_launch]
        classes = R.followed_records(cs, camera_rays(cs, part), 1, trace)[2]
        out.append((sum(int(b.dimension[0]) * int(b.dimension[1]) for b in part), aov_rounds(classes)[0]))
    return out


# ------------------------------------------------------------------------------------------------ fabricated (ray, hit) records

ETAS = (1.0, 1.5, float(F(1.0) / F(1.5)), 1e-3, 1e3)
SWEEP = 24                                                              # float32 neighbours on either side of an edge


@functools.lru_cache(maxsize=None)
def record_scene():
    """Spheres of radius 1 on the x axis - 0: a mirror, 1 ... 5: a dielectric of every eta of ETAS -, a dielectric quad in the plane
    z = 0 with unit edges along x and y (its normal is (0, 0, 1) exactly), and a mirror, a dielectric and a diffuse triangle with
    vertex normals that differ.  A record's hit point on a sphere at centre + (0, 0, 1) with t = 0 has the normal (0, 0, 1)
    exactly, so cosI is -d.z, bit for bit."""
    s = host.Scene()
    s.set_camera((0, 0, 10), (0, 0, 0, 1), 40.0)
    s.add_sphere((0, 0, 0), 1.0, s.add_mirror())
    for k, eta in enumerate(ETAS):
        s.add_sphere((4.0 * (k + 1), 0, 0), 1.0, s.add_dielectric(eta))
    glass = s.add_dielectric(1.5)
    s.add_quad((-2, 4, 0), (1, 0, 0), (0, 1, 0), glass)
    n = np.array([(0.1, 0.2, 1.0), (-0.2, 0.1, 1.0), (0.0, -0.3, 1.0)])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    for k, m in enumerate((s.add_mirror(), glass, s.add_diffuse((0.5, 0.4, 0.3)))):
        v = s.add_vertices([(3.0 * k, -6, 0), (3.0 * k + 2, -6, 0.2), (3.0 * k, -4, -0.1)], n)
        s.add_triangle(v, v + 1, v + 2, m)
    cs = s.compile()
    assert (len(cs.spheres), len(cs.quads), len(cs.triangles)) == (6, 1, 3)
    return cs


def surface_of(cs, rays, hits):
    """The populated record follow_ref.continue_rays reads - hit point 0..2, shading normal 3..5 - of fabricated (ray, hit) pairs, in
    numpy float32 as hj_trace_rays populates a hit: p = fma(t, d, o); a sphere's normal (p - c) * (1 / r), a quad's
    cross(normalize(e1), normalize(e2)), a triangle's normalize((na * ((1 - u) - v) + nb * u) + nc * v).  Zeros for an id outside."""
    rays, hits = np.asarray(rays, F), np.asarray(hits, F)
    n = len(rays)
    ns, nq, nt = len(cs.spheres), len(cs.quads), len(cs.triangles)
    ids = hits[:, 0].copy().view(U).astype(np.int64)
    out = np.zeros((n, 16), F)
    with np.errstate(all="ignore"):
        out[:, 0:3] = MF.segment_point(hits[:, 1].copy(), rays[:, 3:6].copy(), rays[:, 0:3].copy())
        m = ids < ns
        if m.any():
            s = np.asarray(cs.spheres, F)[ids[m]]
            out[m, 3:6] = ((out[m, 0:3] - s[:, 0:3]).astype(F) * (F(1) / s[:, 3])[:, None].astype(F)).astype(F)
        m = (ids >= ns) & (ids < ns + nq)
        if m.any():
            q = np.asarray(cs.quads, F)[ids[m] - ns]
            out[m, 3:6] = cross3(normalize3(q[:, 4:7].copy()), normalize3(q[:, 8:11].copy()))
        m = (ids >= ns + nq) & (ids < ns + nq + nt)
        if m.any():
            tri = np.asarray(cs.triangles).astype(np.int64)[ids[m] - ns - nq]
            nrm = np.asarray(cs.vertices, F)[:, 4:7]
            u, v = hits[m, 2][:, None], hits[m, 3][:, None]
            l0 = ((F(1) - u).astype(F) - v).astype(F)
            out[m, 3:6] = normalize3((((nrm[tri[:, 0]] * l0).astype(F) + (nrm[tri[:, 1]] * u).astype(F)).astype(F) + (nrm[tri[:, 2]] * v).astype(F)).astype(F))
    return out


def _neighbours(c, k=SWEEP):
    """the float32 values from k below to k above c (c > 0), by their bits"""
    b = int(np.array(c, F).view(U))
    return np.arange(max(b - k, 1), b + k + 1, dtype=np.int64).astype(U).view(F)


def _dielectric_at(eta, cos_i):
    """follow_ref.dielectric at the normal (0, 0, 1) for directions (sqrt(1 - c^2), 0, -c): cosI is c exactly"""
    c = np.atleast_1d(np.asarray(cos_i, F))
    d = np.zeros((len(c), 3), F)
    d[:, 0], d[:, 2] = np.sqrt(np.maximum(0.0, 1.0 - c.astype(np.float64) ** 2)).astype(F), -c
    return d, R.dielectric(np.full(len(c), eta, F), d, np.tile(np.array([0, 0, 1], F), (len(c), 1)))


def _edge(eta, sign, what):
    """The smallest |cosI| in (0, 1] - cosI = sign * |cosI|: sign -1 is the swap of eta - from which on the restatement has k > 0
    (what "k") or refracts (what "fr": k > 0 and fr < 0.5), by bisection over the float32 bits; None if it is so at both ends or at
    neither.  Both are monotonic in cosI up to rounding; the sweep around the value found straddles whichever step is there."""
    def ok(bits):
        r = _dielectric_at(eta, sign * np.array([bits], U).view(F))[1]
        with np.errstate(invalid="ignore"):
            return bool(r["k"][0] > 0) if what == "k" else bool(r["k"][0] > 0 and r["fr"][0] < F(0.5))
    lo, hi = 1, int(np.array(1.0, F).view(U))
    if what == "fr":                                                    # (from the first cosI with k > 0 on: below it the k edge decides)
        below = _edge(eta, sign, "k")
        lo = 1 if below is None else int(np.array(below, F).view(U))
    if ok(lo) or not ok(hi):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return float(np.array([hi], U).view(F)[0])


@functools.lru_cache(maxsize=None)
def edge_table():
    """{(eta, sign): (the k edge or None, the fr edge or None)}"""
    return {(eta, sign): (_edge(eta, sign, "k"), _edge(eta, sign, "fr")) for eta in ETAS for sign in (1.0, -1.0)}


def _record(o, d, idx, t=0.0, u=0.25, v=0.25):
    ray, hit = np.zeros(8, F), np.zeros(4, F)
    ray[0:3], ray[3:6], ray[6], ray[7] = o, d, R.KEPS, np.inf
    hit.view(U)[0] = np.uint32(idx & 0xFFFFFFFF)
    hit[1], hit[2], hit[3] = t, u, v
    return ray, hit


@functools.lru_cache(maxsize=None)
def fabricated():
    """-> dict: rays (n, 8), hits (n, 4), surface (n, 16), want (n, 8), cls (n,), cand (continue_rays' detail), sweep: per
    (eta, sign, "k" | "fr") the record indices of the sweep around that edge.  A few thousand records, never written to."""
    cs = record_scene()
    ns, nq, nt = len(cs.spheres), len(cs.quads), len(cs.triangles)
    rays, hits, sweep = [], [], {}

    def add(o, d, idx, **kw):
        ray, hit = _record(o, d, idx, **kw)
        rays.append(ray), hits.append(hit)
        return len(rays) - 1

    # the dielectric branch's edges on the sphere of every eta, entering (cosI > 0) and leaving (cosI < 0: eta is swapped)
    for k, eta in enumerate(ETAS):
        top = (4.0 * (k + 1), 0.0, 1.0)
        for sign in (1.0, -1.0):
            for what, c in zip(("k", "fr"), edge_table()[eta, sign]):
                if c is not None:
                    cs_ = sign * _neighbours(c)
                    sweep[eta, sign, what] = [add(top, dd, k + 1) for dd in _dielectric_at(eta, cs_)[0]]
        for c in (0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30):
            add(top, _dielectric_at(eta, [c])[0][0], k + 1)
    for what, c in zip(("k", "fr"), edge_table()[1.5, -1.0]):           # ... and leaving the quad: u, v where the quad's middle is
        sweep["quad", what] = [add((-1.5, 4.5, 0.0), dd, ns, u=0.5, v=0.5) for dd in _dielectric_at(1.5, -_neighbours(c))[0]]
    # every specular shape and a diffuse one: degenerate directions, t and (u, v)
    rng = np.random.default_rng(77)
    bases = [((0.3, 0.2, 2.5), 0), ((8.1, 0.3, 2.0), 2), ((8.0, 0.2, 0.3), 2), ((-1.6, 4.4, 1.5), ns), ((-1.4, 4.6, -1.5), ns),
             ((0.5, -5.5, 2.0), ns + nq), ((3.5, -5.5, 2.0), ns + nq + 1), ((3.6, -5.4, -2.0), ns + nq + 1), ((6.5, -5.5, 2.0), ns + nq + 2)]
    for o, idx in bases:
        d = np.array((0.05, -0.1, -1.0 if o[2] > 1 else 1.0))
        for scale in (1.0, 1e-20, 1e20, 0.0, 3.0):
            add(o, d * scale, idx, t=1.25)
        for t in (0.0, 1e-45, np.inf, np.nan):
            add(o, d, idx, t=t)
        for u, v in ((-1.0, 0.0), (2.0, 2.0), (np.nan, 0.0)):
            add(o, d, idx, t=1.25, u=u, v=v)
    # the first and the last id of every kind, one past the scene, the chain-left word and the miss
    for idx in (0, ns - 1, ns, ns + nq - 1, ns + nq, ns + nq + nt - 1, ns + nq + nt, 0xFFFFFFFE, 0xFFFFFFFF):
        for _ in range(8):
            add(rng.uniform(-1, 1, 3) + (0, 0, 2), rng.normal(size=3), idx, t=rng.uniform(0.5, 2.5), u=rng.uniform(), v=rng.uniform())
    # ordinary records on every shape, from both sides
    for _ in range(1500):
        idx = int(rng.integers(0, ns + nq + nt))
        add(rng.uniform(-2, 2, 3), rng.normal(size=3), idx, t=rng.uniform(0.0, 3.0), u=rng.uniform(), v=rng.uniform())
    rays, hits = np.array(rays, F), np.array(hits, F)
    surf = surface_of(cs, rays, hits)
    want, cls, cand = R.continue_rays(cs, rays, hits, surf, detail=True)
    for a in (rays, hits, surf, want, cls):
        a.setflags(write=False)
    return dict(rays=rays, hits=hits, surface=surf, want=want, cls=cls, cand=cand, sweep=sweep)


def check_fabricated(f):
    """the premises of the fabricated records, on the restatement alone -> a report of the edges"""
    counts = np.bincount(f["cls"], minlength=6)
    assert (counts >= 16).all(), dict(zip(R.CLASS_NAMES, counts.tolist()))
    assert 2000 <= len(f["rays"]) <= 8000 and len(f["rays"]) % 256 != 0
    k, fr, cls = f["cand"]["k"], f["cand"]["fr"], f["cls"]
    report = {}
    for key, idx in f["sweep"].items():
        kk, ff, cc = k[idx], fr[idx], cls[idx]
        if key[-1] == "k":
            assert (kk <= 0).any() and (kk > 0).any(), key              # the sign of k changes inside the sweep
            assert (cc == R.REFLECT_TIR).any() and (cc != R.REFLECT_TIR).any(), key
        else:
            with np.errstate(invalid="ignore"):
                assert (ff >= F(0.5)).any() and (ff < F(0.5)).any(), key   # fr crosses 0.5 inside the sweep
            assert (cc == R.REFLECT_FR).any() and np.isin(cc, (R.REFRACT_IN, R.REFRACT_OUT)).any(), key
        report[key] = dict(zero_k=int((kk == 0).sum()), classes=np.bincount(cc, minlength=6).tolist())
    table = edge_table()
    # every eta has a k edge on the side where light leaves the denser medium - eta 1 on both: 1 - (1 - c * c) is 0 for a small c -
    # and an fr edge on both sides unless it reflects at normal incidence already (eta 1e-3 and 1e3: fr(1) = 0.996) or never
    # (eta 1: fr stays below 0.03 wherever k > 0)
    for eta in ETAS:
        assert (table[eta, 1.0][0] is not None) == (eta <= 1.0) and (table[eta, -1.0][0] is not None) == (eta >= 1.0), (eta, table)
        assert all((table[eta, s][1] is not None) == (eta not in (1.0, 1e-3, 1e3)) for s in (1.0, -1.0)), (eta, table)
    assert sum(r["zero_k"] for key, r in report.items() if key[-1] == "k") >= 1   # some record has k == 0 exactly
    bits = f["want"].view(U)
    assert np.isnan(f["want"]).any() and ((bits & 0x7FFFFFFF) == 0x7F800000)[:, 0:6].any()   # NaN and infinite words are expected
    return report


# ------------------------------------------------------------------------------------------------------------------- the GPU

@pytest.fixture(autouse=True)
def _no_switch_from_outside(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def r():
    """the renderer without a switch: every test uses it before it puts a switch into the environment"""
    with device.Renderer(0) as ctx:
        yield ctx


def switched(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return device.Renderer(0)


# ------------------------------------------------------------------------------------------------------ followed motion: sizes

def _motion(r, cs, prev, W, H, mf, trace, what, live_all=False, min_live=64):
    want, det = MF.render_motion_followed(cs, prev, W, H, mf, trace, detail=True)
    rounds = motion_rounds(det, mf)
    print(f"{what}: {W} x {H}, {-(-W * H // 256)} tiles, max_follow {mf}, live per round {rounds}")
    assert rounds[0] == W * H if live_all else rounds[0] >= min_live, rounds
    same_bits(r.render_motion(prev, W, H, follow=mf), want, f"{what} {W} x {H}, max_follow {mf}")
    return want, det


@pytest.mark.parametrize("size", [(257, 1), (1, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_a_last_tile_of_one_live_pixel(r, size):
    """257 pixels: the second tile holds pixel 256 alone, and it is live - count == n: the list is the identity, the total sits in
    counts[2].  257 x 1 on _mirror_scene; 1 x 257 on wide_mirror_scene (its docstring says why)."""
    W, H = size
    cs = _mirror_scene(0) if H == 1 else wide_mirror_scene()
    r.upload_scene(cs)
    for mf in (2, 8):
        _motion(r, cs, quads_moved(cs), W, H, mf, R.oracle_trace(cs), "mirror", live_all=True)


def test_motion_a_scan_of_two_counts_a_thread(r):
    """257 x 256 = 65 792 pixels: 257 tiles, per == 2, the scan's threads 129 and above own nothing; the mirror-filled scene at 8
    as well: every one of the 257 tiles full in round 1"""
    cs = P.scene("rich")
    r.upload_scene(cs)
    _motion(r, cs, _prev(cs), 257, 256, 2, gpu_trace(r), "rich")
    cs = _mirror_scene(0)
    r.upload_scene(cs)
    for mf in (2, 8):
        _motion(r, cs, quads_moved(cs), 257, 256, mf, R.oracle_trace(cs), "mirror", live_all=True)


def test_motion_a_scan_of_three_counts_a_thread(r):
    """513 x 257 = 131 841 pixels: 516 tiles, per == 3, threads 172 and above own nothing, the last tile holds one pixel; "rich"
    with every shape kind moved"""
    cs = P.scene("rich")
    r.upload_scene(cs)
    _, det = _motion(r, cs, _prev(cs), 513, 257, 2, gpu_trace(r), "rich")
    assert det["left"].sum() > 50 and (det["count"] == 2).sum() > 1000


@pytest.mark.parametrize("size", [(16384, 1), (1, 16384)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_at_the_side_limit(r, size):
    """The camera inside the box that test_walk_forms_gpu.py uses for plain motion takes no continuation at either size (asserted:
    the reference says 0), so the image is wide_mirror_scene's: every pixel live in round 1, the steep chains leave.  One pixel
    more is refused."""
    W, H = size
    inside = _scene_seen_from_inside()
    det = MF.render_motion_followed(inside, _prev(inside), W, H, 2, R.oracle_trace(inside), detail=True)[1]
    assert det["went"].sum() == 0                                       # (were it 64 or more, this scene would be the one to run)
    cs = wide_mirror_scene()
    r.upload_scene(cs)
    want, det = _motion(r, cs, quads_moved(cs), W, H, 2, R.oracle_trace(cs), "wide mirror", live_all=True)
    assert (MF.ids_of(want) == MF.LEFT).sum() >= (0 if H == 1 else 64)
    with pytest.raises(abi.HijikiError) as e:
        r.render_motion(quads_moved(cs), W + (H == 1), H + (W == 1), follow=2)
    assert e.value.status == abi.HJ_ERR_INVALID, str(e.value)


def test_motion_device_output_between_sentinels(r):
    """the device-output form into a 16-byte aligned view in the middle of a tensor of sentinels, as test_walk_forms_gpu.py does for
    plain motion: every pixel written, nothing outside the H x W x 4 words"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", r.device)
    for cs, prev, W, H, trace in ((_mirror_scene(0), None, 257, 1, None), (P.scene("rich"), None, 70, 41, "gpu")):
        r.upload_scene(cs)
        prev = quads_moved(cs) if trace is None else _prev(cs)
        want = MF.render_motion_followed(cs, prev, W, H, 8, R.oracle_trace(cs) if trace is None else gpu_trace(r))
        n, front, back = 4 * W * H, 4 * 1027, 4 * 4099
        big = torch.full((front + n + back,), SENTINEL, dtype=torch.int32, device=dev)
        view = big[front:front + n]
        assert view.data_ptr() % 16 == 0
        torch.cuda.synchronize(dev)
        r._check(device.lib().hj_render_motion_followed(r._h, C.byref(prev.desc), W, H, 8, abi.MOTION_DEVICE_OUT, view.data_ptr()))
        words = big.cpu().numpy().view(U)
        assert (words[:front] == SENTINEL).all() and (words[front + n:] == SENTINEL).all(), f"{W} x {H}: words outside the view were written"
        got = words[front:front + n].reshape(H, W, 4)
        assert not (got[..., 3] == SENTINEL).any()
        same_bits(got.view(F), want, f"the view {W} x {H}")


# ------------------------------------------------------------------------------------------------------- followed motion: the cap

@pytest.mark.parametrize("mf", [1, 7, 8])
def test_motion_the_cap_between_two_facing_mirrors(r, mf):
    """every pixel live in every round, every chain takes all max_follow continuations - the Householder product compounded up to 8
    times -, and both mirrors moved in prev, so the product reaches every record"""
    cs = _facing_mirrors()
    W = H = 64
    prev = quads_moved(cs)
    want, det = MF.render_motion_followed(cs, prev, W, H, mf, R.oracle_trace(cs), detail=True)
    assert (det["count"] == mf).all() and not det["left"].any() and motion_rounds(det, mf) == [W * H] * mf
    still = MF.render_motion_followed(cs, M.Prev(cs, prev.camera), W, H, mf, R.oracle_trace(cs))
    assert (want.view(U)[..., 0:3] != still.view(U)[..., 0:3]).any(-1).mean() > 0.9     # the moved mirrors show: M * (Xp - Xn) is in the records
    r.upload_scene(cs)
    same_bits(r.render_motion(prev, W, H, follow=mf), want, f"facing mirrors, max_follow {mf}")


# ------------------------------------------------------------------------------------------------------------- live-count edges

@pytest.mark.parametrize("live,wg", [(1, None), (256, None), (64, 64), (65, 64), (100, 100), (101, 100)])
def test_a_round_of_exactly_so_many_live_chains(r, monkeypatch, live, wg):
    """count == 1, == wg_rays, == wg_rays + 1: the grid is ceil(count / wg_rays) and the last workgroup takes count - first.  Without
    a switch a small launch's workgroup takes 256 entries; HJ_TRACE_WG_RAYS makes it 64 or 100.  At max_follow 1 as well as 2: a
    chain that a round skips is still live in the next one and ends with the same record, so only a call without a next round shows
    a dropped list entry (a library that drops the last entry of 65 and 101 passes at 2)."""
    cs = patch_scene(live)
    trace = R.oracle_trace(cs)
    prev = quads_moved(cs)
    blocks = one_block(PATCH_W, PATCH_H)
    wants = {}
    for mf in (1, 2):
        want_m, det = MF.render_motion_followed(cs, prev, PATCH_W, PATCH_H, mf, trace, detail=True)
        want_a, rounds, _ = expected_aovs(cs, PATCH_W, PATCH_H, blocks, mf, trace)
        assert motion_rounds(det, mf) == rounds == [live, 0][:mf], (motion_rounds(det, mf), rounds)
        wants[mf] = (want_m, want_a)
    with (switched(monkeypatch, {"HJ_TRACE_WG_RAYS": wg}) if wg else device.Renderer(0)) as ctx:
        ctx.upload_scene(cs)
        for mf, (want_m, want_a) in wants.items():
            same_bits(ctx.render_motion(prev, PATCH_W, PATCH_H, follow=mf), want_m, f"motion, {live} live, wg_rays {wg}, max_follow {mf}")
            same_bits(ctx.render_aovs(PATCH_W, PATCH_H, blocks=blocks, follow=mf), want_a, f"aovs, {live} live, wg_rays {wg}, max_follow {mf}")


def test_every_slot_live(r):
    """count == n for a walk launch of AOV samples: a 128 x 128 block of the facing mirrors fills all 16384 slots, the list is the
    identity.  (For motion: test_motion_a_last_tile_of_one_live_pixel and the cap.)"""
    cs = _facing_mirrors()
    blocks = one_block(128, 128)
    want, rounds, _ = expected_aovs(cs, 128, 128, blocks, 2, R.oracle_trace(cs))
    assert rounds == [SLOTS, SLOTS]
    r.upload_scene(cs)
    same_bits(r.render_aovs(128, 128, blocks=blocks, follow=2), want, "every slot live")


@pytest.mark.parametrize("wg", [None, 64])
def test_live_counts_that_shrink_to_one(r, monkeypatch, wg):
    """nested_scene: 11, 5, 3 and 1 live chains in the rounds 1 to 4, in one scene"""
    cs = nested_scene()
    trace = R.oracle_trace(cs)
    prev = quads_moved(cs)
    W, mf = NESTED_W, NESTED_FOLLOW
    want_m, det = MF.render_motion_followed(cs, prev, W, 1, mf, trace, detail=True)
    blocks = one_block(W, 1)
    want_a, rounds, _ = expected_aovs(cs, W, 1, blocks, mf, trace)
    for counts in (motion_rounds(det, mf), rounds):
        print("live per round:", counts)
        assert all(a > b for a, b in zip(counts, counts[1:])) and counts[-1] == 1 and len(counts) == mf, counts
    with (switched(monkeypatch, {"HJ_TRACE_WG_RAYS": wg}) if wg else device.Renderer(0)) as ctx:
        ctx.upload_scene(cs)
        same_bits(ctx.render_motion(prev, W, 1, follow=mf), want_m, f"motion, shrinking counts, wg_rays {wg}")
        same_bits(ctx.render_aovs(W, 1, blocks=blocks, follow=mf), want_a, f"aovs, shrinking counts, wg_rays {wg}")


# ------------------------------------------------------------------------------------------------------ followed AOVs: launches

@pytest.mark.parametrize("per_launch", [9, 5, 2])
def test_aov_launches_of_ragged_and_differing_size(r, monkeypatch, per_launch):
    """Nine blocks of 16 x 16 and smaller on "rich" at max_follow 2; a block occupies 16384 slots whatever its size.
    HJ_TRACE_CHUNK = 9 blocks: one launch of 576 tiles, per == 3, the scan's threads 192 and above own nothing.
    5 blocks: launches of 5 and 4 - 320 tiles, per == 2, the scan's threads 160 and above own
    nothing; then 256 tiles, per == 1.  2 blocks: 2, 2, 2, 2 and 1 - state, counts and list are reused, and the last launch, one
    8 x 8 block, has fewer samples and fewer live chains than the launch before it: its smaller count lies in front of stale words."""
    torch = pytest.importorskip("torch")
    cs = P.scene("rich")
    blocks = launch_blocks()
    r.upload_scene(cs)
    trace = gpu_trace(r)
    want, rounds, _ = expected_aovs(cs, 40, 40, blocks, 2, trace)
    per = launch_live(cs, blocks, trace, per_launch)
    print(f"{per_launch} blocks a launch: (samples, live in round 1) {per}; the call's live per round {rounds}")
    assert sum(p[1] for p in per) == rounds[0] and rounds[1] > 0 and min(p[1] for p in per) > 0
    if per_launch == 2:
        assert len(per) == 5 and per[4][0] < per[3][0] and per[4][1] < per[3][1], per
    with switched(monkeypatch, {"HJ_TRACE_CHUNK": per_launch * SLOTS}) as ctx:
        ctx.upload_scene(cs)
        same_bits(ctx.render_aovs(40, 40, blocks=blocks, follow=2), want, f"{per_launch} blocks a launch")
        out = ctx.render_aovs(40, 40, blocks=blocks, follow=2, device=True)
        assert out.is_cuda
        same_bits(out.cpu().numpy(), want, f"{per_launch} blocks a launch, device array")


# ------------------------------------------------------------------------------------------- hj_follow_specular, fabricated records

def fabricated_equal(got, want, what):
    """Every word on bits - but a NaN word, which the contract (include/hijiki_hip.h, "The specular continuation") holds to being
    a NaN: of the 60 NaN words these records give, 13 have another sign on the GPU than numpy gives them on an x86 host (the
    default NaN of inf - inf and 0 * inf is negative there), so their bits cannot be asked for."""
    bad = R.nan_equal(got, want)
    odd = int((np.isnan(want) & (np.ascontiguousarray(got, F).view(U) != want.view(U))).sum())
    print(f"{what}: {int(np.isnan(want).sum())} NaN words, {odd} of them with other bits than the restatement's")
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} words differ, first at {at}: {got[at[0]].tolist()} / {want[at[0]].tolist()}")


def test_follow_specular_on_fabricated_records(r, monkeypatch):
    """k_follow at the dielectric branch's edges, on degenerate records and on the edge ids.  Every word on bits; a NaN word is held
    to being a NaN (fabricated_equal)."""
    import torch
    f = fabricated()
    report = check_fabricated(f)
    print({str(k): v for k, v in report.items()})
    rays, hits, want = f["rays"], f["hits"], f["want"]
    cs = record_scene()
    r.upload_scene(cs)
    fabricated_equal(r.follow_specular(rays, hits), want, "host arrays")
    dev = f"cuda:{r.device}"
    tr, th = torch.from_numpy(np.array(rays)).to(dev), torch.from_numpy(np.array(hits)).to(dev)
    fabricated_equal(r.follow_specular(tr, th).cpu().numpy(), want, "device tensors")
    with switched(monkeypatch, {"HJ_TRACE_CHUNK": 256}) as ctx:
        ctx.upload_scene(cs)
        fabricated_equal(ctx.follow_specular(rays, hits), want, "chunks of 256")
        fabricated_equal(ctx.follow_specular(tr, th).cpu().numpy(), want, "device tensors in chunks of 256")
