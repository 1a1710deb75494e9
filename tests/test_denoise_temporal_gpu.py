"""hj_denoise_frame_temporal on the GPU against temporal_ref - the contract restated in numpy - bit for bit on every word of `out`
and of `history_out`: test_denoise_gpu's fabricated frames from 1 x 1 to 70 x 41 with fabricated histories (invalid holes, lengths
from 1 to the cap and across 4, depths and normals on both sides of their tests), cameras that are identical, translated, rotated
about each axis, of another fov and turned by 180 degrees, in both kernel forms; the two anchors against hj_denoise_frame on the GPU;
feedback on and off; a chain of three frames; device tensors; beauty = NULL over a rendered frame; and the one condition a temporal
stage has to meet: after 8 frames it is nearer the truth than the spatial filter alone."""
import os

import numpy as np
import pytest

import denoise_ref as D
import path_query_ref as P
import temporal_ref as T
from hijiki_amd import abi, device, host
from test_denoise_gpu import BIG, SIDE, big_frame, frame, same_bits

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
FORMS = ("0", "128", None)        # HJ_DENOISE_LDS_STEP: direct at every step, the LDS form at every step, the default
SIZES = [(1, 1), (7, 1), (1, 7), (37, 13), (70, 41)]
CAM = T.camera((0.2, -0.1, 0.5), T.axis_angle((0.2, 1, 0.1), 15), 60.0)


def _moved(position=None, then=None, fov=None):
    """CAM with another position, a further rotation (axis, degrees) applied in float64, or another fov"""
    q = np.array(list(CAM.rotation), np.float64)
    if then is not None:
        r = np.array(T.axis_angle(*then), np.float64)
        w = q[3] * r[3] - q[0:3] @ r[0:3]
        q = np.array([*(np.cross(q[0:3], r[0:3]) + r[0:3] * q[3] + q[0:3] * r[3]), w])
    return T.camera(list(CAM.position)[0:3] if position is None else position, [float(F(v)) for v in q], CAM.fov if fov is None else fov)


PREV = {"identical": CAM, "translated": _moved(position=(0.5, 0.05, 0.3)), "about x": _moved(then=((1, 0, 0), 2.0)), "about y": _moved(then=((0, 1, 0), -3.0)),
        "about z": _moved(then=((0, 0, 1), 5.0)), "another fov": _moved(fov=50.0), "turned": _moved(then=((0, 1, 0), 180.0))}


@pytest.fixture(scope="module")
def forms():
    """a renderer per form (the switch is read when the context is created); none of them gets a scene"""
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
    with device.Renderer(0) as r:
        yield r


@pytest.fixture(autouse=True)
def _the_library_has_the_call():
    assert hasattr(device.lib(), "hj_denoise_frame_temporal") and "hj_denoise_frame_temporal" in device.EXPORTS


_HIST = {}


def history(W, H, max_history=64):
    """A fabricated history for frame(W, H), once per size: the frame's own depth and normal, so that an identical camera finds it -
    but a tenth of the records invalid, depths scaled by 1, 1.05, 0.93 (inside the tolerance of 0.1) or 1.15, 0.8 (outside), a sixth
    of the normals turned past the cosine of 0.9, lengths 1 ... max_history with every length up to 6 present; light and moments
    random."""
    if (W, H) in _HIST:
        return _HIST[(W, H)]
    rng = np.random.default_rng([W, H, 2028])
    G, c, A, I, n, z = D.prepare(*frame(W, H))
    h = np.zeros((H, W, 12), F)
    h[..., 0:3] = rng.uniform(0.1, 2.0, (H, W, 3))
    N = rng.integers(1, max_history + 1, (H, W))
    N = np.where(rng.random((H, W)) < 0.4, rng.integers(1, 7, (H, W)), N)
    N.flat[:min(W * H, 12)] = (np.arange(12) % 6 + 1)[:min(W * H, 12)]
    m1 = rng.uniform(0.2, 1.5, (H, W))
    h[..., 3], h[..., 4], h[..., 5] = N, m1, m1 * m1 + rng.uniform(-0.05, 0.5, (H, W))               # (some variances below 0: the fmaxf)
    h[..., 6] = np.where(z > 0, z, 4.0) * rng.choice(np.array([1, 1, 1, 1.05, 0.93, 1.15, 0.8], F), (H, W))
    turned = rng.random((H, W)) < 1 / 6
    h[..., 8:11] = np.where(turned[..., None], (0.8, 0.0, 0.6), np.where((n == 0).all(-1)[..., None], (0.0, 0.0, 1.0), n))
    valid = rng.random((H, W)) >= 0.1
    if W * H == 1:
        valid[:], h[..., 6], h[..., 8:11] = True, z, n
    h.view(U)[..., 7] = valid
    _HIST[(W, H)] = h
    return h


_WANT = {}


def want(W, H, prev, it, **kw):
    key = (W, H, prev, it, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = T.run(*frame(W, H), CAM, PREV[prev], history(W, H), it, **kw)
    return _WANT[key]


def both(got, w, what):
    same_bits(got[0], w[0], what + ": out")
    same_bits(got[1], w[1], what + ": history_out")


def test_the_fabricated_history_holds_what_the_cases_need():
    W, H = 70, 41
    beauty, aov = frame(W, H)
    h = history(W, H)
    G, c, A, I, n, z = D.prepare(beauty, aov)
    valid = h.view(U)[..., 7] != 0
    assert (~valid).sum() > 100 and set(range(1, 7)) <= set(h[..., 3].astype(int).ravel().tolist()) and h[..., 3].max() > 32
    assert ((h[..., 3] < 4) & G & valid).sum() > 100 and ((h[..., 3] >= 4) & G & valid).sum() > 100
    assert (h[..., 5] < h[..., 4] * h[..., 4]).any()
    found, edges = {}, set()
    for name, prev in PREV.items():
        front, fx, fy, zp = T.project(CAM, prev, z, W, H)
        has = T.reproject(G, n, z, CAM, prev, h, 0.1, 0.9)[0]
        found[name] = (int((front & G).sum()), int(has.sum()))
        if name == "turned":
            assert found[name] == (0, 0)
            continue
        assert 200 < has.sum() < G.sum() - 200, (name, found)           # (taps pass and taps fail)
        g = G & front
        if name != "identical":                                         # taps fall off the image, and taps stay inside
            off = {"left": (fx[g] < 0).any(), "right": (fx[g] > W - 1).any(), "top": (fy[g] < 0).any(), "bottom": (fy[g] > H - 1).any()}
            assert any(off.values()), name
            edges |= {k for k, v in off.items() if v}
        else:
            assert np.abs(fx - np.arange(W)[None, :])[g].max() < 1e-3 and np.abs(fy - np.arange(H)[:, None])[g].max() < 1e-3
    assert edges == {"left", "right", "top", "bottom"}, edges
    # both sides of the two tests among the taps an identical camera reaches
    zr = h[..., 6][G & valid] / z[G & valid]
    assert (np.abs(zr - 1) < 0.09).any() and (np.abs(zr - 1) > 0.11).any()
    dots = (h[..., 8:11] * n).sum(-1)
    assert (dots[G & valid] < 0.85).any() and (dots[G & valid] > 0.95).any()
    w = want(W, H, "translated", 5)
    assert np.isfinite(w[0]).all() and np.isfinite(w[1]).all() and not (w[0] == D.run(beauty, aov, 5)).all()
    assert (w[1][..., 3] > 1).any() and (w[1][..., 3] == 1).any() and (w[1].view(U)[~G] == 0).all()


@pytest.mark.parametrize("step", FORMS)
@pytest.mark.parametrize("size", SIZES)
def test_every_size_in_every_form(forms, size, step):
    W, H = size
    it = 5 if (W, H) == (70, 41) else 3
    for prev in ("identical", "translated"):
        got = forms[step].denoise_frame_temporal(frame(W, H)[1], CAM, PREV[prev], history(W, H), frame(W, H)[0], it)
        both(got, want(W, H, prev, it), f"{W} x {H}, {prev}, {it} iterations, HJ_DENOISE_LDS_STEP={step}")


def test_lattice_tiles_beyond_one_a_residue_class(forms):
    """test_denoise_gpu's 517 x 131 frame behind the temporal stage, the LDS form at every step: two lattice tiles a residue class
    in both axes up to step 16, the temporal variance where the history is long enough"""
    W, H = BIG
    beauty, aov = big_frame()
    out, hist, s = T.run(beauty, aov, CAM, PREV["translated"], history(W, H), 5, keep=True)
    assert 10000 < s["has"].sum() < s["G"].sum() - 10000 and (s["N"][s["has"]] >= T.VARIANCE_FRAMES).sum() > 1000
    assert s["has"][128:, 480:].any()                                   # (history found in the last tiles too)
    both(forms["128"].denoise_frame_temporal(aov, CAM, PREV["translated"], history(W, H), beauty, 5), (out, hist), "517 x 131, translated, form 128")


@pytest.mark.parametrize("size", SIDE)
def test_the_side_limit(forms, size):
    """16384 x 1 and 1 x 16384 with an identical camera pair: the accumulate and variance kernels at the side limit, then eight
    iterations in the LDS form"""
    W, H = size
    beauty, aov = frame(W, H)
    out, hist, s = T.run(beauty, aov, CAM, CAM, history(W, H), 8, keep=True)
    assert np.isfinite(out).all() and np.isfinite(hist).all() and 1000 < s["has"].sum() < s["G"].sum() - 1000
    both(forms["128"].denoise_frame_temporal(aov, CAM, CAM, history(W, H), beauty, 8), (out, hist), f"{W} x {H}, identical, form 128")


@pytest.mark.parametrize("prev", sorted(PREV))
def test_every_camera_pair(forms, prev):
    for W, H in ((37, 13), (70, 41)):
        beauty, aov = frame(W, H)
        for step in ("0", "128"):
            both(forms[step].denoise_frame_temporal(aov, CAM, PREV[prev], history(W, H), beauty, 2), want(W, H, prev, 2), f"{W} x {H}, {prev}, form {step}")


def test_the_anchors_are_the_spatial_denoiser_bit_for_bit(forms):
    """no history, a history whose valid words are all 0, a previous camera that looks the other way: hj_denoise_frame's output"""
    W, H = 70, 41
    beauty, aov = frame(W, H)
    holes = history(W, H).copy()
    holes.view(U)[..., 7] = 0
    for step in ("0", "128"):
        r = forms[step]
        spatial = r.denoise_frame(aov, beauty, 5)
        first = r.denoise_frame_temporal(aov, CAM, CAM, None, beauty, 5)
        same_bits(first[0], spatial, f"history None, form {step}")
        both(first, T.run(beauty, aov, CAM, CAM, None, 5), f"history None against the reference, form {step}")
        for what, got in (("valid words 0", r.denoise_frame_temporal(aov, CAM, PREV["translated"], holes, beauty, 5)),
                          ("looking the other way", r.denoise_frame_temporal(aov, CAM, PREV["turned"], history(W, H), beauty, 5))):
            same_bits(got[0], spatial, f"{what}, form {step}")
            same_bits(got[1], first[1], f"{what}: history_out, form {step}")
    guided = first[1].view(U)[..., 7] == 1
    assert (first[1][..., 3][guided] == 1).all() and (first[1].view(U)[~guided] == 0).all() and guided.sum() == D.prepare(beauty, aov)[0].sum()


@pytest.mark.parametrize("kw", [dict(feedback=False), dict(alpha=0.0, alpha_moments=0.0), dict(alpha=1.0, alpha_moments=1.0), dict(max_history=1),
                                dict(max_history=5, depth_tolerance=0.0, normal_cos=-1.0), dict(depth_tolerance=0.06, normal_cos=1.0)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_options(forms, kw):
    W, H = 37, 13
    beauty, aov = frame(W, H)
    for it in (0, 1, 5):
        w = want(W, H, "translated", it, **kw)
        for step in ("0", "128"):
            both(forms[step].denoise_frame_temporal(aov, CAM, PREV["translated"], history(W, H), beauty, it, **kw), w, f"{kw}, {it} iterations, form {step}")


def test_feedback_feeds_the_first_iteration_and_nothing_without_one(forms):
    W, H = 70, 41
    beauty, aov = frame(W, H)
    r = forms[None]
    run = lambda it, fb: r.denoise_frame_temporal(aov, CAM, PREV["about z"], history(W, H), beauty, it, feedback=fb)      # noqa: E731
    for it in (0, 1, 5):
        on, off = run(it, True), run(it, False)
        both(on, want(W, H, "about z", it), f"feedback, {it} iterations")
        both(off, want(W, H, "about z", it, feedback=False), f"no feedback, {it} iterations")
        same_bits(on[0], off[0], "out does not depend on the flag")
        same_bits(on[1][..., 3:], off[1][..., 3:], "nor do the history's other words")
        assert (on[1][..., 0:3] == off[1][..., 0:3]).all() == (it == 0)
    same_bits(run(1, True)[1], run(5, True)[1], "the history is the first iteration's whatever follows")


def test_a_chain_of_three_frames(forms):
    """the GPU's own history_out fed back as history_in, the camera moving, against the reference chained the same way"""
    W, H = 70, 41
    cams = [PREV["translated"], PREV["about y"], CAM]
    rng = np.random.default_rng(77)
    beauty, aov = frame(W, H)
    frames = [np.concatenate([beauty[..., 0:3] * rng.uniform(0.5, 1.5, (H, W, 3)).astype(F), beauty[..., 3:4]], -1) for _ in cams]   # (other noise, the same surfaces)
    want_h, got_h = None, {"0": None, None: None}
    for k, cam in enumerate(cams):
        prev = cams[k - 1] if k else cam
        w = T.run(frames[k], aov, cam, prev, want_h, 3)
        for step in got_h:
            got = forms[step].denoise_frame_temporal(aov, cam, prev, got_h[step], frames[k], 3)
            both(got, w, f"frame {k}, form {step}")
            got_h[step] = got[1]
        want_h = w[1]
    assert (want_h[..., 3] > 2.5).any() and (want_h[..., 3] == 1).any()


def test_device_tensors_in_place_give_the_same_bits_and_stay_unchanged(forms):
    torch = pytest.importorskip("torch")
    r = forms["128"]
    W, H = 70, 41
    beauty, aov = frame(W, H)
    dev = torch.device("cuda", r.device)
    tb, ta, th = (torch.from_numpy(a).to(dev) for a in (beauty, aov, history(W, H)))
    for it in (0, 1, 4, 5):
        out, hist = r.denoise_frame_temporal(ta, CAM, PREV["translated"], th, tb, it, device=True)
        assert len({out.data_ptr(), hist.data_ptr(), ta.data_ptr(), tb.data_ptr(), th.data_ptr()}) == 5 and tuple(hist.shape) == (H, W, 12)
        both((out.cpu().numpy(), hist.cpu().numpy()), want(W, H, "translated", it), f"device arrays, {it} iterations")
    first = r.denoise_frame_temporal(ta, CAM, CAM, None, tb, 2, device=True)
    both([t.cpu().numpy() for t in first], T.run(beauty, aov, CAM, CAM, None, 2), "device arrays, no history")
    for t, a, what in ((tb, beauty, "beauty"), (ta, aov, "aov"), (th, history(W, H), "history_in")):
        same_bits(t.cpu().numpy(), a, what + " afterwards")
    with pytest.raises(abi.HijikiError) as e:                            # an aliased history is refused on the device too
        L, o, t = device.lib(), abi.DenoiseOpts(1, 0.5, 1, 4, 0.1, 1), abi.TemporalOpts(CAM, CAM, 0.2, 0.2, 0.1, 0.9, 64, 1)
        import ctypes as C
        r._check(L.hj_denoise_frame_temporal(r._h, W, H, tb.data_ptr(), ta.data_ptr(), C.byref(o), C.byref(t), th.data_ptr(), th.data_ptr(), out.data_ptr()))
    assert e.value.status == abi.HJ_ERR_INVALID and "history_out aliases" in str(e.value)
    same_bits(th.cpu().numpy(), history(W, H), "history_in after the refusal")


def test_null_beauty_reads_the_framebuffer_and_leaves_it(scene_r):
    r = scene_r
    cs = P.scene("cbox")
    r.upload_scene(cs)
    r.create_framebuffer(64, 64)
    cam = cs.desc.camera
    hist = None
    for seed in (21, 22):
        r.clear()
        r.render_frame(4, seed)
        before = r.read()
        aov = r.render_aovs(64, 64, spp=4, master_seed=seed)
        got = r.denoise_frame_temporal(aov, cam, cam, hist)
        both(got, T.run(before, aov, cam, cam, hist), f"beauty = NULL / the reference over the framebuffer, seed {seed}")
        same_bits(r.read(), before, "the framebuffer afterwards")
        both(r.denoise_frame_temporal(aov, cam, cam, hist, before), got, "beauty = NULL / the framebuffer as a host array")
        hist = got[1]
    assert (hist[..., 3] == 2).sum() > 2000                             # (a fixed camera finds its history)
    with pytest.raises(abi.HijikiError) as e:
        r.denoise_frame_temporal(np.zeros((32, 64, 12), F), cam, cam)
    assert e.value.status == abi.HJ_ERR_INVALID and "hj_denoise_frame_temporal:" in str(e.value) and "64 x 64" in str(e.value), str(e.value)


def test_eight_accumulated_frames_are_nearer_the_truth_than_the_spatial_filter(scene_r):
    """The cbox at 128 x 128 with a fixed camera: 8 frames of 4 spp (seeds 31 ... 38) accumulated with the defaults, against the 256 spp
    truth (seed 32): mse(temporal, frame 8) < mse(denoise_frame, frame 8), over the whole image and over the guided pixels alone, and
    the frame-8 history is longer than HJ_TEMPORAL_VARIANCE_FRAMES on more than half the guided pixels.  Conditions, not tuned
    numbers: no ratio is asserted (profiles/NOTES.md has them)."""
    W = H = 128
    r = scene_r
    cs = host.Scene.synthetic(host.SYNTH_CBOX).compile()
    r.upload_scene(cs)
    r.create_framebuffer(W, H)
    r.render_frame(256, 32)
    truth = r.resolve().astype(np.float64)
    cam = cs.desc.camera
    hist = None
    for seed in range(31, 39):
        r.clear()
        r.render_frame(4, seed)
        aov = r.render_aovs(W, H, spp=4, master_seed=seed)
        temporal, hist = r.denoise_frame_temporal(aov, cam, cam, hist)
    spatial, raw = r.denoise_frame(aov), r.resolve()
    guided = hist.view(U)[..., 7] != 0
    mse = lambda img, m: float(np.mean((img[..., 0:3].astype(np.float64) - truth)[m] ** 2))            # noqa: E731
    everywhere = np.ones((H, W), bool)
    long_enough = float((hist[..., 3][guided] > abi.TEMPORAL_VARIANCE_FRAMES).mean())
    for what, m in (("whole image", everywhere), ("guided pixels", guided)):
        print(f"{what}: mse raw {mse(raw, m):.6g}, spatial {mse(spatial, m):.6g}, temporal {mse(temporal, m):.6g}, temporal / spatial "
              f"{mse(temporal, m) / mse(spatial, m):.4f}, temporal / raw {mse(temporal, m) / mse(raw, m):.4f}")
    print(f"guided {int(guided.sum())} of {W * H}; history longer than {abi.TEMPORAL_VARIANCE_FRAMES} on {long_enough:.4f} of them")
    assert np.isfinite(temporal).all() and np.isfinite(hist).all()
    assert mse(temporal, everywhere) < mse(spatial, everywhere)
    assert mse(temporal, guided) < mse(spatial, guided)
    assert long_enough > 0.5
