"""hj_denoise_frame on the GPU against denoise_ref - the contract restated in numpy - bit for bit on every output word: fabricated
frames from 1 x 1 to 70 x 41 (no multiple of the 32 x 8 tile; at step 16 the taps lie +-32 away, past a tile and past the image),
both forms of the iteration forced through HJ_DENOISE_LDS_STEP and a mix of them, holes of every kind, flat regions, albedos at and
below the floor, every sigma off alone and all off, 0 and 8 iterations, device tensors in place; beauty = NULL over a rendered
frame; 517 x 131 and 517 x 259 (several lattice tiles a residue class in both axes up to step 16) and the side limit of 16384;
the command line; and the one condition a denoiser has to meet: less error than the frame it was given."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import path_query_ref as P
from hijiki_amd import abi, device, host
from test_abi import ROOT

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
FORMS = ("0", "128", "2", None)   # HJ_DENOISE_LDS_STEP: direct at every step, the LDS form at every step, LDS up to step 2, the default
DEFAULTS = (0.5, 1.0, 4.0, 0.1)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(U) != want.view(U)
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} words differ, first at {at}: {got[at[:-1]].tolist()} / {want[at[:-1]].tolist()}")


@pytest.fixture(scope="module")
def forms():
    """a renderer per form: the switch is read when the context is created - and again by every upload and render call, so these
    renderers never get a scene: the tests that need one take `scene_r`"""
    before = os.environ.get("HJ_DENOISE_LDS_STEP")
    made = {}
    try:
        for step in FORMS:
            os.environ.pop("HJ_DENOISE_LDS_STEP", None)
            if step is not None:
                os.environ["HJ_DENOISE_LDS_STEP"] = step
            made[step] = device.Renderer(0)
        os.environ.pop("HJ_DENOISE_LDS_STEP", None)
        if before is not None:
            os.environ["HJ_DENOISE_LDS_STEP"] = before
        yield made
    finally:
        for r in made.values():
            r.close()


@pytest.fixture(scope="module")
def scene_r():
    """the renderer of the tests that upload a scene and render frames (the switch at its default)"""
    with device.Renderer(0) as r:
        yield r


@pytest.fixture(autouse=True)
def _the_library_has_the_call():
    """every test of this file is about hj_denoise_frame, the reference's self-checks included: none passes without the symbol"""
    assert hasattr(device.lib(), "hj_denoise_frame") and "hj_denoise_frame" in device.EXPORTS


_FRAMES = {}


def frame(W, H):
    """A fabricated (beauty, aov) of W x H, once per size: 4 samples a pixel; vertical bands of albedo, a normal that turns at a third
    of the height, a depth ramp with a step at 60 % of the width; noisy light except in a flat, black block (there V == 0); and, where the
    image has room for them, every kind of hole and the albedo edge cases."""
    if (W, H) in _FRAMES:
        return _FRAMES[(W, H)]
    rng = np.random.default_rng([W, H, 2027])
    y, x = np.mgrid[0:H, 0:W]
    S = F(4)
    albedo = np.stack([0.2 + 0.6 * ((x // 9) % 2), 0.5 + 0.0 * x, 0.8 - 0.5 * ((x // 5) % 2)], -1).astype(F)
    normal = np.where((y < H // 3)[..., None], (0.0, 0.6, 0.8), (0.0, 0.0, 1.0)).astype(F) + rng.uniform(-0.02, 0.02, (H, W, 3)).astype(F)
    depth = (3.0 + 0.05 * x + 0.02 * y + np.where(x >= (6 * W) // 10, 2.5, 0.0)).astype(F)
    hits = np.full((H, W), 4, F)
    hits[rng.random((H, W)) < 0.15] = 3                                 # (edges of geometry: one sample missed)
    light = (0.5 + 0.3 * np.sin(0.3 * x + 0.2 * y))[..., None] * rng.uniform(0.25, 1.75, (H, W, 3))
    colour = (albedo * light).astype(F)
    bw = rng.uniform(3.0, 5.0, (H, W)).astype(F)
    emission = np.zeros((H, W, 3), F)
    if W >= 30 and H >= 12:
        colour[2:11, 12:24], albedo[2:11, 12:24], hits[2:11, 12:24] = 0.0, (0.5, 0.5, 0.25), 4   # flat (and black, so that every sum is exact): V == 0 inside
        normal[2:11, 12:24], bw[2:11, 12:24] = (0, 0, 1), 4
        albedo[H - 4:, 2:6] = (0.001, 0.5, 0.0)                         # below the floor; exactly 0
        albedo[H - 4:, 8:11], emission[H - 4:, 8:11] = 0.0, (12.0, 10.0, 8.0)   # an emitter: albedo 0, emission, bright
        colour[H - 4:, 8:11] = (12.0, 10.0, 8.0)
        hits[0, 3], hits[H - 1, W - 1], hits[5, 0], hits[6, W // 2], hits[7:9, 26:29] = 0, 0, 0, 0, 0   # Hc == 0 with bw > 0: border, inside
        bw[0, 7], bw[4, W - 1], bw[9, 5], bw[3, 14] = 0, 0, 0, 0       # bw == 0 with Hc > 0 (one of them inside the flat block)
        hits[H - 2, 1], bw[H - 2, 1] = 0, 0                             # neither
    elif W * H > 1:
        hits.flat[1] = 0
        bw.flat[W * H - 1] = 0
    beauty = np.concatenate([colour * bw[..., None], bw[..., None]], -1).astype(F)
    aov = np.zeros((H, W, 12), F)
    aov[..., 0:3], aov[..., 3] = albedo * S, S
    aov[..., 4:7], aov[..., 7] = normal * hits[..., None], depth * hits
    aov[..., 8:11], aov[..., 11] = emission * hits[..., None], hits
    _FRAMES[(W, H)] = (beauty, aov)
    return beauty, aov


_WANT = {}


def want(W, H, iterations, sigmas=DEFAULTS):
    """the reference for a fabricated frame, once; the iterations below come from the same run"""
    key = (W, H, sigmas)
    if key not in _WANT or len(_WANT[key]) <= iterations:
        _WANT[key] = D.run(*frame(W, H), max(iterations, 8 if (W, H) == (70, 41) else 4), *sigmas, keep=True)
    return _WANT[key][iterations]


BIG = (517, 131)      # ceil(517 / 16) = 33 > 32 and ceil(131 / 16) = 9 > 8: at every step up to 16 a residue class has two lattice tiles in x and in y, the last ragged
# 517 / 32 and 131 / 8 are nearly equal: there tiles_x == tiles_y at every step (17, 9, 5, 3, 2), and a decode that took one for the other
# would not show.  517 x 259: tiles_x, tiles_y = (17, 33), (9, 17), (5, 9), (3, 5), (2, 3) at the steps 1 ... 16, both above 1 and never equal.
TALL = (517, 259)
_BIG = {}


def big_frame(size=BIG):
    """frame(W, H) of a size in (BIG, TALL) with its holes near the origin, and hits = 0 (the AOV's normal, depth, emission and hit
    count zero) at about 1 % of the pixels, so that the last lattice tile of a residue class - the pixels from (512, 128) or
    (512, 256) on - holds holes and guided pixels both.  The premise is asserted here, before any GPU call."""
    if size not in _BIG:
        W, H = size
        y0 = (H - 1) // 128 * 128
        assert W > 512 and H - y0 == 3
        beauty, aov = frame(W, H)
        aov = aov.copy()
        holes = np.random.default_rng([W, H, 2030]).random((H, W)) < 0.01
        holes[H - 2, 513] = True                                        # (one inside the last tile that is not frame()'s corner pixel)
        aov[holes, 4:12] = 0
        G = D.prepare(beauty, aov)[0]
        assert 0.007 * W * H < holes.sum() < 0.013 * W * H and not G[holes].any()
        assert (~G)[y0:, 512:].any() and G[y0:, 512:].any() and (~G)[H - 2, 513] and G.mean() > 0.9
        aov.setflags(write=False)
        _BIG[size] = (beauty, aov)
    return _BIG[size]


def big_want(size=BIG):
    """the reference for big_frame(size), five iterations (steps 1 ... 16), once"""
    key = ("want", size)
    if key not in _BIG:
        _BIG[key] = D.run(*big_frame(size), 5)
        assert np.isfinite(_BIG[key]).all()
        _BIG[key].setflags(write=False)
    return _BIG[key]


def test_the_fabricated_frame_holds_what_the_cases_need():
    beauty, aov = frame(70, 41)
    G, c, A, I, n, z = D.prepare(beauty, aov)
    assert (~G).sum() >= 12 and (~G)[0].any() and (~G)[:, 0].any() and (~G)[1:-1, 1:-1].any()
    assert ((aov[..., 11] > 0) & (beauty[..., 3] == 0)).sum() == 4 and ((aov[..., 11] == 0) & (beauty[..., 3] > 0)).sum() >= 5
    V = D.variance(I, G)
    assert (V[4:9, 16:22] == 0).all() and (V[G] > 0).sum() > 2000
    assert (A == F(0.015625)).any() and (aov[..., 0:3] / aov[..., 3:4] < 0.015625)[G].any()
    lit = (aov[..., 8:11] > 0).any(-1)                                  # the emitter: it and the pixels within two of it pass through
    assert lit.sum() == 12 and not G[41 - 6:, 6:13].any() and G[41 - 7, 6:13].all() and G[41 - 4:, 2:6].all()
    out5 = want(70, 41, 5)
    assert np.isfinite(out5).all() and not (out5 == want(70, 41, 0)).all()


@pytest.mark.parametrize("step", FORMS)
@pytest.mark.parametrize("size", [(1, 1, 2), (1, 7, 3), (7, 1, 3), (37, 13, 4), (70, 41, 5)])
def test_every_size_in_every_form(forms, size, step):
    W, H, it = size
    beauty, aov = frame(W, H)
    same_bits(forms[step].denoise_frame(aov, beauty, it), want(W, H, it), f"{W} x {H}, {it} iterations, HJ_DENOISE_LDS_STEP={step}")


@pytest.mark.parametrize("step", ["0", "128", None])
def test_lattice_tiles_beyond_one_a_residue_class(forms, step):
    """517 x 131: k_dn_filter_lds' block decode (rx * tiles_x + tx, ry * tiles_y + ty) with tiles_x > 1 and tiles_y > 1 at the steps
    4, 8 and 16, a ragged last tile in both axes, holes inside it"""
    beauty, aov = big_frame()
    same_bits(forms[step].denoise_frame(aov, beauty, 5), big_want(), f"517 x 131, HJ_DENOISE_LDS_STEP={step}")


def test_lattice_tiles_with_other_counts_in_x_than_in_y(forms):
    """517 x 259 in the LDS form at every step: tiles_x != tiles_y and both above 1 at every step up to 16 - at 517 x 131 the two are
    equal at every step, and a decode that divided by the wrong one would pass there"""
    W, H = TALL
    up = lambda a, b: -(-a // b)                                        # noqa: E731
    for s in (1, 2, 4, 8, 16):
        tx, ty = up(up(W, s), 32), up(up(H, s), 8)
        assert tx > 1 and ty > 1 and tx != ty, (s, tx, ty)
        bx, by = up(up(BIG[0], s), 32), up(up(BIG[1], s), 8)
        assert bx == by > 1, (s, bx, by)
    beauty, aov = big_frame(TALL)
    same_bits(forms["128"].denoise_frame(aov, beauty, 5), big_want(TALL), "517 x 259, HJ_DENOISE_LDS_STEP=128")


SIDE = [(16384, 1), (1, 16384)]       # kDenoiseMaxSide; at step 128 the lattice grid is 128 x tiles blocks, nearly all of them apron


@pytest.mark.parametrize("step", ["0", "128"])
@pytest.mark.parametrize("size", SIDE)
def test_the_side_limit_in_both_forms(forms, size, step):
    W, H = size
    beauty, aov = frame(W, H)
    w = want(W, H, 8)
    assert np.isfinite(w).all() and not (w == want(W, H, 7)).all()
    same_bits(forms[step].denoise_frame(aov, beauty, 8), w, f"{W} x {H}, 8 iterations, HJ_DENOISE_LDS_STEP={step}")


def test_one_pixel_past_the_side_limit_is_refused(forms):
    for W, H in ((16385, 1), (1, 16385)):
        with pytest.raises(abi.HijikiError) as e:
            forms[None].denoise_frame(np.zeros((H, W, 12), F), np.zeros((H, W, 4), F), 1)
        assert e.value.status == abi.HJ_ERR_INVALID and "hj_denoise_frame:" in str(e.value) and "1 ... 16384 each" in str(e.value), str(e.value)


@pytest.mark.parametrize("sigmas", [(0.0, 1.0, 4.0, 0.1), (0.5, 0.0, 4.0, 0.1), (0.5, 1.0, 0.0, 0.1), (0.5, 1.0, 4.0, 0.0), (0.0, 0.0, 0.0, 0.0)])
def test_each_sigma_off_alone_and_all_off(forms, sigmas):
    beauty, aov = frame(37, 13)
    w = want(37, 13, 3, sigmas)
    assert not (w == want(37, 13, 3)).all()                             # (the stop that is off did something)
    for step in ("0", "128"):
        same_bits(forms[step].denoise_frame(aov, beauty, 3, *sigmas), w, f"sigmas {sigmas}, HJ_DENOISE_LDS_STEP={step}")


@pytest.mark.parametrize("iterations", [0, 8])
def test_no_iteration_and_eight(forms, iterations):
    beauty, aov = frame(70, 41)
    w = want(70, 41, iterations)
    for step in ("0", "128"):
        same_bits(forms[step].denoise_frame(aov, beauty, iterations), w, f"{iterations} iterations, HJ_DENOISE_LDS_STEP={step}")
    if iterations == 0:                                                 # the round trip, the initial variance in word 3
        G, c, A, I, n, z = D.prepare(beauty, aov)
        same_bits(w[..., 3], D.variance(I, G), "initial variance")
        same_bits(w[~G][:, 0:3], c[~G], "unguided colour")
        assert np.allclose(w[G][:, 0:3], c[G], rtol=3e-7, atol=0)


def test_device_tensors_in_place_give_the_same_bits_and_stay_unchanged(forms):
    torch = pytest.importorskip("torch")
    r = forms["128"]
    beauty, aov = frame(70, 41)
    dev = torch.device("cuda", r.device)
    tb, ta = torch.from_numpy(beauty).to(dev), torch.from_numpy(aov).to(dev)
    for it in (0, 1, 4, 5):                                              # (an odd and an even count: either working image is the last)
        out = r.denoise_frame(ta, tb, it, device=True)
        assert out.data_ptr() not in (ta.data_ptr(), tb.data_ptr()) and tuple(out.shape) == (41, 70, 4)
        same_bits(out.cpu().numpy(), r.denoise_frame(aov, beauty, it), f"device / host arrays, {it} iterations")
        same_bits(out.cpu().numpy(), want(70, 41, it), f"device arrays, {it} iterations")
    same_bits(tb.cpu().numpy(), beauty, "beauty afterwards")
    same_bits(ta.cpu().numpy(), aov, "aov afterwards")


def test_null_beauty_reads_the_framebuffer_and_leaves_it(scene_r):
    r = scene_r
    r.upload_scene(P.scene("cbox"))
    r.create_framebuffer(64, 64)
    r.render_frame(4, 21)
    before = r.read()
    aov = r.render_aovs(64, 64, spp=4, master_seed=21)
    got = r.denoise_frame(aov)
    same_bits(got, D.run(before, aov), "beauty = NULL / the reference over the framebuffer")
    same_bits(r.read(), before, "the framebuffer afterwards")
    same_bits(got, r.denoise_frame(aov, before), "beauty = NULL / the framebuffer as a host array")
    assert (got[..., 0:3] != (before[..., 0:3] / before[..., 3:4])).any()
    torch = pytest.importorskip("torch")
    same_bits(r.denoise_frame(torch.from_numpy(aov).to(torch.device("cuda", r.device)), device=True).cpu().numpy(), got, "beauty = NULL, device aov")
    # a framebuffer of another size is refused, behind the gate
    with pytest.raises(abi.HijikiError) as e:
        r.denoise_frame(np.zeros((32, 64, 12), F))
    assert e.value.status == abi.HJ_ERR_INVALID and "hj_denoise_frame:" in str(e.value) and "64 x 64" in str(e.value), str(e.value)
    # ... and no scene is needed: a fresh context denoises a fabricated frame
    with device.Renderer(0) as fresh:
        same_bits(fresh.denoise_frame(*frame(37, 13)[::-1], 2), want(37, 13, 2), "a context without a scene")


def test_cli_writes_the_denoised_frame(scene_r, tmp_path):
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    args = [exe, "--use-bvh", "-w", "64", "-h", "48", "-s", "4", "--seed", "6", "-o", str(tmp_path / "o.pfm")]
    run = subprocess.run(args + ["--denoise", str(tmp_path / "d.pfm"), "--denoise-params", "3,0.5,1,4,0.2", "synthetic:cbox"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    r = scene_r
    r.upload_scene(host.Scene.synthetic(host.SYNTH_CBOX).compile())
    r.create_framebuffer(64, 48)
    r.render_frame(4, 6)
    w = r.denoise_frame(r.render_aovs(64, 48, spp=4, master_seed=6), None, 3, 0.5, 1.0, 4.0, 0.2)
    head = b"PF\n64 48\n-1.0\n"
    got = np.frombuffer(open(tmp_path / "d.pfm", "rb").read(), F, offset=len(head)).reshape(48, 64, 3)[::-1]
    same_bits(got, w[..., 0:3], "--denoise")
    for bad in (["--denoise", "x.pfm", "--bake-lightmap", "8x8"], ["--denoise-params", "3,1,1,1,1"], ["--denoise", "x.pfm", "--denoise-params", "9,1,1,1,1"]):
        assert subprocess.run(args + bad + ["synthetic:cbox"], capture_output=True, text=True, timeout=60).returncode == 2, bad


def test_the_denoised_frame_is_nearer_the_truth_than_the_raw_one(scene_r):
    """The cbox at 128 x 128: a 4 spp frame (seed 31) denoised with the defaults against a 256 spp frame (seed 32):
    mse(denoised, truth) < mse(raw, truth).  A condition, not a tuned number: no ratio is asserted (profiles/NOTES.md has them)."""
    W = H = 128
    r = scene_r
    r.upload_scene(host.Scene.synthetic(host.SYNTH_CBOX).compile())
    r.create_framebuffer(W, H)
    r.render_frame(256, 32)
    truth = r.resolve().astype(np.float64)
    r.clear()
    r.render_frame(4, 31)
    raw = r.resolve()
    out = r.denoise_frame(r.render_aovs(W, H, spp=4, master_seed=31))
    mse = lambda img: float(np.mean((img[..., 0:3].astype(np.float64) - truth) ** 2))                # noqa: E731
    print(f"mse raw {mse(raw):.6g}, denoised {mse(out):.6g}, ratio {mse(out) / mse(raw):.4f}")
    assert np.isfinite(out).all() and np.isfinite(truth).all()
    assert mse(out) < mse(raw)
