"""Scenes of the light-map tests (tests/test_lightmap_host.py, tests/test_lightmap_gpu.py): seeded and small - but for scale_scene,
whose triangle count follows the card (tests/test_lightmap_scale_host.py, tests/test_lightmap_scale_gpu.py).  Every triangle has
three vertices of its own, so a triangle's index is its place in the list it was built from."""
import functools

import numpy as np

from hijiki_amd import abi, host

F = np.float32


def _add_mesh(s, uv, pos, nrm, material):
    """uv (n, 3, 2), pos, nrm (n, 3, 3) -> n triangles behind whatever the scene holds already"""
    uv, pos, nrm = np.asarray(uv, F), np.asarray(pos, F), np.asarray(nrm, F)
    base = s.add_vertices(pos.reshape(-1, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2))
    s.add_triangles(base + np.arange(3 * len(uv)).reshape(-1, 3), material)


EDGE_CASES = ("quad lower", "quad upper", "vertex on a centre", "overlap low", "overlap high", "partly outside", "wholly outside", "zero area",
              "collinear", "collinear through centres", "nan uv", "inf uv", "sliver", "zero normals", "cancelling normals",
              "huge finite uv 1e30", "huge finite uv 3e38", "huge negative uv", "just outside")


def _edge_scene(n, centre_cases):
    """edge_scene laid out for an n x n atlas; centre_cases: (m, 3, 2) float32 triangles in front of the named cases"""
    rng = np.random.default_rng(41)
    c = lambda x, y: (x / float(n), y / float(n))                          # noqa: E731  texel-corner coordinates
    m = lambda x, y: ((x + 0.5) / float(n), (y + 0.5) / float(n))          # noqa: E731  the centre of texel (x, y)
    uv = [
        [c(8, 8), c(24, 8), c(24, 24)],                                    # a quad's two triangles: the diagonal runs through centres
        [c(8, 8), c(24, 24), c(8, 24)],
        [m(40, 8), m(50, 8), m(40, 20)],                                   # vertices, two edges and the hypotenuse's ends on centres
        [c(30, 30), c(50, 32), c(34, 52)],                                 # two that overlap: the lower index wins
        [c(36, 28), c(56, 40), c(38, 50)],
        [(-0.2, 0.5), (0.1, 0.4), (0.05, 0.7)],
        [(1.2, 1.2), (1.5, 1.3), (1.3, -1.6)],
        [c(5, 40), c(5, 40), c(5, 40)],
        [(0.6, 0.6), (0.7, 0.7), (0.8, 0.8)],
        [m(10, 60), m(20, 60), m(30, 60)],                                 # every edge value is zero on the centres of row 60
        [(np.nan, 0.2), (0.3, 0.2), (0.3, 0.4)],
        [(0.1, 0.1), (np.inf, 0.2), (0.2, 0.3)],
        [(5 / 64.0, 0.8000), (58 / 64.0, 0.8100), (58 / 64.0, 0.8140)],     # under a third of a texel high at 64, 53 / 64 of the atlas long
        [c(3, 44), c(14, 45), c(4, 58)],
        [m(36, 40), m(52, 40), m(36, 56)],                                 # hu = i / 16, hv = j / 16 at the centre (36 + i, 40 + j)
        [(1e30, 0.5), (0.995, 0.48), (0.995, 0.53)],                       # finite: vmax * n is clamped from far above; a wedge through the right edge
        [(0.2, 0.2), (3e38, 3e38), (0.3, 0.6)],                            # vmax * n overflows; products at this vertex are inf - inf: no texel
        [(-1e30, 0.15), (0.005, 0.13), (0.005, 0.18)],                     # the lower clamp: a wedge through the left edge.  (Along such a wedge the
        #   barycentrics do not change, so texels of one row share a position; these two start so close to the edge that up to 257 texels
        #   a side they hold one column, for the tests that need every texel's position to be its own.)
        [(-1e-7, 1 + 1e-7), (1 + 1e-7, 1 + 1e-7), (0.5, 0.93)],            # the box ends just outside [0, 1] on three sides
    ]
    assert len(uv) == len(EDGE_CASES)
    extra = 26
    centre = rng.uniform(0.0, 1.0, (extra, 1, 2))
    with np.errstate(over="ignore"):
        uv = np.concatenate([np.asarray(centre_cases, F).reshape(-1, 3, 2), np.array(uv, np.float64).astype(F),
                             (centre + rng.uniform(-0.12, 0.12, (extra, 3, 2))).astype(F)])
    case = {name: len(centre_cases) + i for i, name in enumerate(EDGE_CASES)}
    n_tri = len(uv)
    pos = rng.uniform([-1.0, 0.1, -1.0], [1.0, 1.9, 1.0], (n_tri, 1, 3)) + rng.uniform(-0.3, 0.3, (n_tri, 3, 3))
    nrm = rng.normal(size=(n_tri, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    nrm[case["zero normals"]] = 0.0
    nrm[case["cancelling normals"]] = [[0, 1, 0], [0, -1, 0], [0, 1, 0]]   # (l0 - hu) + hv = 0 exactly where hu = 1/2
    s = host.Scene()
    s.set_camera((0.0, 1.0, 3.3), (0.0, 0.0, 0.0, 1.0), 40.0)
    white = s.add_diffuse((0.7, 0.7, 0.7))
    s.add_sphere((-0.5, 0.4, 0.2), 0.3, white)
    s.add_sphere((0.5, 0.3, -0.2), 0.25, s.add_mirror())
    s.add_quad((-1.3, 0.0, 1.3), (2.6, 0.0, 0.0), (0.0, 0.0, -2.6), white)
    _add_mesh(s, uv, pos, nrm, white)
    cs = s.compile()
    assert len(cs.spheres) == 2 and len(cs.quads) == 1 and len(cs.triangles) == n_tri
    return cs, case


@functools.lru_cache(maxsize=None)
def edge_scene():
    """About 45 triangles behind 2 spheres and 1 quad (so a triangle's shape index is not its triangle index), laid out for a 64 x 64
    atlas, whose texel centres are the odd multiples of 1/128.  The first len(EDGE_CASES) triangles are those cases, in that order;
    random triangles follow.  Positions are random (the uv footprints say nothing about the geometry); normals random unless the
    case is about them.  -> (compiled scene, index of each case)"""
    return _edge_scene(64, np.zeros((0, 3, 2), F))


CENTRE_TEXELS = lambda n: (0, 1, n // 2 - 1, n // 2, n - 2, n - 1)        # noqa: E731  (8191 and 8192 at n = 16384)


@functools.lru_cache(maxsize=None)
def edge_scene_at(n, along):
    """edge_scene with its corner and centre helpers dividing by n, for atlases with n texels along u (along = 0) or v (along = 1) and
    1, 3 or 5 along the other axis (n = 16384: the limit).  In front of the named cases stand the per-centre cases, so that no other
    triangle can take their texels.  For each texel i of CENTRE_TEXELS(n), ten triangles with one straight side at centre(i) moved by
    d = -2 ... 2 float32 ulps (np.nextafter): the side is the box's minimum along the axis (the triangle lies above it, sign +1) or
    its maximum (sign -1).  Each is 0.9 texel deep, so it reaches no other centre of the axis, and spans [0.2, 0.8] on the other
    axis, so it reaches the middle centre there.  (Triangles for both axes in one scene would hide each other: the thin ones
    along v at texels 8191 and 8192 hold v = 0.5, the one centre of an atlas of height 1.)  The closed comparison takes centre i in
    exactly when the side has not moved past it, and the owner is the lowest index, so the order decides what a wrong answer
    shows: first the four that do NOT cover (a texel taken by one of them gets an index that is too low), then the two with d = 0
    (minimum side first at every other texel of the list, maximum side first at the rest: a centre ON the side that is missed
    passes the texel to a later index), then the rest.  So texel i of the list's entry k belongs to triangle 10 k + 4.
    -> (compiled scene, index of each case)"""
    tris = []
    w = F(0.9 / n)
    for k, i in enumerate(CENTRE_TEXELS(n)):
        first = (1, 0) if k % 2 == 0 else (-1, 0)
        for sign, d in [(1, 2), (1, 1), (-1, -2), (-1, -1), first, (-first[0], 0), (1, -1), (1, -2), (-1, 1), (-1, 2)]:
            x = F((F(i) + F(0.5)) / F(n))
            for _ in range(abs(d)):
                x = np.nextafter(x, F(2.0 if d > 0 else -2.0), dtype=F)
            t = np.array([(x, 0.2), (x, 0.8), (x + F(sign) * w, 0.5)], F)
            tris.append(t if along == 0 else t[:, ::-1])
    return _edge_scene(n, np.array(tris, F))


def _pair(u0, v0, u1, v1, y=0.0):
    """an upward rectangle (x, z) = (u, v) scaled to [-1, 1] at height y, as two triangles that share the diagonal"""
    q = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
    uv = np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], F)
    pos = np.zeros((2, 3, 3), F)
    pos[:, :, 0], pos[:, :, 1], pos[:, :, 2] = 2 * uv[:, :, 0] - 1, y, 2 * uv[:, :, 1] - 1
    nrm = np.zeros((2, 3, 3), F)
    nrm[:, :, 1] = 1.0
    return uv, pos, nrm


@functools.lru_cache(maxsize=None)
def full_pair_scene():
    """one triangle pair over all of [0, 1]^2"""
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    _add_mesh(s, *_pair(0.0, 0.0, 1.0, 1.0), s.add_diffuse((0.6, 0.6, 0.6)))
    return s.compile()


@functools.lru_cache(maxsize=None)
def tiny_scene(n=20000, side=512):
    """n triangles of under one texel of a side x side atlas each, and a floor quad"""
    rng = np.random.default_rng(43)
    centre = rng.uniform(0.0, 1.0, (n, 1, 2))
    uv = (centre + rng.uniform(-0.45, 0.45, (n, 3, 2)) / side).astype(F)
    pos = np.zeros((n, 3, 3), F)
    pos[:, :, 0], pos[:, :, 2] = 2 * uv[:, :, 0] - 1, 2 * uv[:, :, 1] - 1
    pos[:, :, 1] = rng.uniform(0.1, 1.0, (n, 3))
    nrm = rng.normal(size=(n, 3, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    white = s.add_diffuse((0.7, 0.7, 0.7))
    s.add_quad((-1.3, 0.0, 1.3), (2.6, 0.0, 0.0), (0.0, 0.0, -2.6), white)
    _add_mesh(s, uv, pos, nrm, white)
    return s.compile()


LARGE_SIDE = 12                                                         # a placed large triangle's legs in texels: its box is 14 x 14 > 64 texels
LARGE_AT = ((0.05, 0.06), (0.22, 0.13), (0.41, 0.32), (0.13, 0.52), (0.61, 0.71), (0.78, 0.23), (0.33, 0.83), (0.87, 0.55))


def _two(x, y, side):
    """a triangle over exactly the two centres (x, y) and (x + 1, y) of a side x side atlas: its box is 3 x 1 centres"""
    return np.array([(x - 0.3, y + 0.15), (x + 2.3, y + 0.15), (x + 1.0, y + 0.95)]) / side


def scale_scene_uv(n, side, trip, large):
    """The uv (n, 3, 2) float32 of scale_scene, and where the large triangles stand.  Below index `trip`: tiny_scene's sub-texel
    triangles, centres anywhere but in the last 8 rows.  From `trip` on: each over two neighbouring centres of row side - 4, three
    columns apart - every one of them owns texels, because nothing else reaches that row.  At each index L of `large` (at most
    len(LARGE_AT)): a right triangle with legs of LARGE_SIDE texels on texel corners (X, Y), (X + 12, Y), (X, Y + 12) - it covers the
    centres (X + i, Y + j) with i + j <= 11, those with i + j == 11 exactly on its hypotenuse; L - 1 is a two-centre triangle
    inside it at (X + 2 ... 3, Y + 2), which it loses to; L + 1 is one over (X + 9, Y + 2) and (X + 10, Y + 2): the first inside, which
    the large triangle takes from it, the second outside, which it keeps.  -> (uv, {L: (X, Y)})"""
    assert side >= 256 and n - trip <= (side - 4) // 3 and len(large) <= len(LARGE_AT)
    rng = np.random.default_rng(43)
    centre = rng.uniform(0.0, 1.0, (n, 1, 2)) * [1.0, (side - 8.0) / side]
    uv = centre + rng.uniform(-0.45, 0.45, (n, 3, 2)) / side
    for k in range(trip, n):
        uv[k] = _two(3 * (k - trip), side - 4, side)
    where = {}
    for L, (fx, fy) in zip(large, LARGE_AT):
        X, Y = int(fx * side), int(fy * side)
        assert 0 < L < n - 1 and not {L - 1, L, L + 1} & {m + d for m in where for d in (-1, 0, 1)}
        uv[L] = np.array([(X, Y), (X + LARGE_SIDE, Y), (X, Y + LARGE_SIDE)]) / side
        uv[L - 1], uv[L + 1] = _two(X + 2, Y + 2, side), _two(X + 9, Y + 2, side)
        where[L] = (X, Y)
    return uv.astype(F), where


@functools.lru_cache(maxsize=None)
def scale_scene(n, side, trip, large):
    """scale_scene_uv as a scene without a tree (a mesh of this size is built on the device: compile(with_tree=False)), positions
    from the uv as in tiny_scene -> (compiled shapes, {L: (X, Y)})"""
    uv, where = scale_scene_uv(n, side, trip, large)
    rng = np.random.default_rng(47)
    pos = np.zeros((n, 3, 3), F)
    pos[:, :, 0], pos[:, :, 2] = 2 * uv[:, :, 0] - 1, 2 * uv[:, :, 1] - 1
    pos[:, :, 1] = rng.uniform(0.1, 1.0, (n, 3))
    nrm = rng.normal(size=(n, 3, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    white = s.add_diffuse((0.7, 0.7, 0.7))
    s.add_quad((-1.3, 0.0, 1.3), (2.6, 0.0, 0.0), (0.0, 0.0, -2.6), white)
    _add_mesh(s, uv, pos, nrm, white)
    return s.compile(with_tree=False), where


def scale_count(cus):
    """-> (n, trip): trip = 64 * 4 * 8 * cus triangles are one trip of k_lm_owner's grid on a card with `cus` compute units; n is one
    whole 64-triangle group and one ragged group of 37 beyond it"""
    trip = 64 * 4 * 8 * cus
    return trip + 64 + 37, trip


def scale_large(trip):
    """where the large triangles of the scale scene stand: group 0; groups 2047 and 2048 (the last of k_lm_owner_wide's first trip
    and the first of its second); a group of k_lm_owner's second trip; the ragged last group"""
    return (5, 2047 * 64 + 62, 2048 * 64 + 1, trip + 10, trip + 64 + 20)


@functools.lru_cache(maxsize=None)
def limit_scene(W=16384, H=4096):
    """Four small charts (triangle pairs) for an atlas at both limits, W x H = 2^26 texels: one in the first scan tile (row 0, columns
    0 ... 19); one on both sides of texel index W * H / 2 (rows H / 2 - 2 ... H / 2 + 1, columns 0 ... 9); one over the last 40 columns of the last 30 rows; one that reaches past the corner and holds
    all of the last scan tile (the last 256 texels of the last row) - so the highest texel index, W * H - 1, is owned."""
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    white = s.add_diffuse((0.6, 0.6, 0.6))
    for box in ((0.0, 0.0, 20.0 / W, 3.0 / H), (0.0, 0.5 - 2.0 / H, 10.0 / W, 0.5 + 2.0 / H),
                (1 - 40.0 / W, 1 - 30.0 / H, 1.0, 1.0), (1 - 300.0 / W, 1 - 2.0 / H, 1.001, 1.001)):
        _add_mesh(s, *_pair(*box), white)
    return s.compile()


def check_scale_conditions(owner, first, last, trip, where):
    """What the REFERENCE's owner map of the scale scene's triangles [first, last) must hold for a comparison against it to mean
    something: every placed large triangle owns texels, loses the centre it shares with L - 1 and wins the one it shares with L + 1;
    with the whole scene at least 100 distinct owners from k_lm_owner's second trip (index >= trip) and 100 between
    k_lm_owner_wide's first trip (64 * 2048) and that; the last triangle owns a texel; the owned texels are between 1/40 and 1/5
    of the triangles (a sub-texel triangle covers a centre about one time in 16).  -> the number of owned texels"""
    owners = np.unique(owner[owner != 0xFFFFFFFF]).astype(np.int64)
    for L, (X, Y) in where.items():
        if not first <= L - 1 < L + 1 < last:
            continue
        assert {L - 1, L, L + 1} <= set(owners.tolist()), (L, "a placed triangle owns nothing")
        assert owner[Y + 2, X + 2] <= L - 1 and owner[Y + 2, X + 9] <= L, L                      # the minimum: below, then above
        assert (owner[Y:Y + LARGE_SIDE, X:X + LARGE_SIDE] == L).sum() > 40, L
    if (first, last) == (0, trip + 64 + 37):
        assert (owners >= trip).sum() >= 100, int((owners >= trip).sum())
    assert ((owners >= 64 * 2048) & (owners < trip)).sum() >= 100
    assert trip > 64 * 2048 and owners.min() >= first and owners.max() == last - 1
    count = int((owner != 0xFFFFFFFF).sum())
    assert (last - first) // 40 < count < (last - first) // 5, count
    return count


def _box_scene(s, floor):
    """A UV-mapped floor (two triangles, chart [0.02, 0.6] x [0.05, 0.95]) and a UV-mapped box standing on it (top and four sides,
    one chart each in the strip u > 0.64) in `s`."""
    uv, pos, nrm = _pair(0.02, 0.05, 0.6, 0.95)
    pos[:, :, 0], pos[:, :, 2] = 2.4 * (uv[:, :, 0] - 0.02) / 0.58 - 1.2, 2.4 * (uv[:, :, 1] - 0.05) / 0.9 - 1.2
    _add_mesh(s, uv, pos, nrm, floor)
    lo, hi = np.array([-0.5, 0.0, -0.4]), np.array([0.1, 0.7, 0.3])
    faces = [((0, 1, 0), 1, (0, 2)), ((1, 0, 0), 0, (2, 1)), ((-1, 0, 0), 0, (1, 2)), ((0, 0, 1), 2, (0, 1)), ((0, 0, -1), 2, (1, 0))]
    uvs, poss, nrms = [], [], []
    for k, (n, axis, (a, b)) in enumerate(faces):
        u0, v0 = 0.66, 0.03 + 0.19 * k
        quv = np.array([(u0, v0), (u0 + 0.3, v0), (u0 + 0.3, v0 + 0.16), (u0, v0 + 0.16)])
        corner = np.zeros((4, 3))
        corner[:, axis] = hi[axis] if sum(n) > 0 else lo[axis]
        corner[:, a] = [lo[a], hi[a], hi[a], lo[a]]
        corner[:, b] = [lo[b], lo[b], hi[b], hi[b]]
        for tri in ((0, 1, 2), (0, 2, 3)):
            uvs.append(quv[list(tri)]); poss.append(corner[list(tri)]); nrms.append(np.tile(np.array(n, float), (3, 1)))
    _add_mesh(s, np.array(uvs), np.array(poss), np.array(nrms), s.add_diffuse((0.3, 0.5, 0.7)))


@functools.lru_cache(maxsize=None)
def bake_scene(env=False):
    """A Cornell-like box - quad walls and ceiling, an area light - around _box_scene; env: open instead (no walls, no ceiling, no
    light) under a small sky"""
    s = host.Scene()
    s.set_camera_cbox()
    white = s.add_diffuse((0.7, 0.7, 0.7))
    if env:
        import env_scenes
        s.add_sphere((0.6, 0.3, 0.5), 0.3, white)
        s.set_environment(s.add_texture(env_scenes.sky_texels(8, 16), abi.TEX_BILINEAR), 1.5)
    else:
        s.add_quad((-1.2, 0, -1.2), (2.4, 0, 0), (0, 2.0, 0), white)
        s.add_quad((-1.2, 0, 1.2), (0, 0, -2.4), (0, 2.0, 0), s.add_diffuse((0.6, 0.1, 0.1)))
        s.add_quad((1.2, 0, -1.2), (0, 0, 2.4), (0, 2.0, 0), s.add_diffuse((0.1, 0.6, 0.1)))
        s.add_quad((-1.2, 2.0, -1.2), (2.4, 0, 0), (0, 0, 2.4), white)
        s.add_quad((-0.4, 1.99, -0.4), (0.8, 0, 0), (0, 0, 0.8), s.add_emissive((15.0, 14.0, 12.0)))
    _box_scene(s, white)
    return s.compile()


@functools.lru_cache(maxsize=None)
def sky_pair_scene():
    """one upward triangle pair (chart [0.25, 0.75]^2) alone under the constant sky of 0.5"""
    s = host.Scene()
    s.set_camera((0.0, 3.0, 0.0), (-0.70710678, 0.0, 0.0, 0.70710678), 40.0)
    _add_mesh(s, *_pair(0.25, 0.25, 0.75, 0.75), s.add_diffuse((0.5, 0.5, 0.5)))
    s.set_environment(s.add_texture(np.full((4, 8, 4), 0.5, F), abi.TEX_NEAREST))
    return s.compile()


def moved(cs, seed=7):
    """cs.vertices moved in place: positions jittered, normals turned (uv untouched) -> the arrays before the move"""
    rng = np.random.default_rng(seed)
    v = cs.vertices
    keep = v.copy()
    v[:, 0:3] += rng.uniform(-0.05, 0.05, (len(v), 3)).astype(F)
    n = v[:, 4:7] + rng.uniform(-0.3, 0.3, (len(v), 3)).astype(F)
    live = (keep[:, 4:7] != 0).any(axis=1)
    v[live, 4:7] = n[live]
    return keep
