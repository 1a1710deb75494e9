"""hj_follow_specular, hj_render_aovs_followed and hj_render_aovs_frame_followed on the GPU against follow_ref - the contract restated
in numpy - bit for bit on every word: the continuation of every (ray, hit) record of the box's query rays, every branch class
among them, from host arrays, device tensors and in chunks; the same records through the oracle-pinned shade stage
(hj_debug_shade_step); the followed sums of ragged and overlapping block lists and of frames against chains made by alternating the
restatement with hj_trace_rays itself; max_follow = 0 and a scene without a specular surface against hj_render_aovs; two facing
mirrors, where every chain reaches the cap; coverage; the walk's other forms; a frame before and after; the denoiser as consumer;
the command line.  No tolerance anywhere."""
import functools
import os
import subprocess

import numpy as np
import pytest

import aov_ref as A
import denoise_ref as D
import follow_ref as R
import path_query_ref as P
from hijiki_amd import abi, device, host
from test_abi import ROOT
from test_shade_step_gpu import records as step_records

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32
FOLLOWS = (1, 2, 8)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(U) != want.view(U)
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} words differ, first at {at}: {got[at[:-1]].tolist()} / {want[at[:-1]].tolist()}")


@pytest.fixture(autouse=True)
def _the_library_has_the_calls():
    assert all(hasattr(device.lib(), n) for n in ("hj_follow_specular", "hj_render_aovs_followed", "hj_render_aovs_frame_followed"))


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as r:
        yield r


def gpu_trace(r):
    """followed_records' trace: hj_trace_rays' two arrays (the scene is uploaded on r)"""
    def trace(rays):
        ids, t, u, v, surf = r.trace_rays(rays, surface=True)
        return np.stack([ids.view(F), t, u, v], 1), surf
    return trace


# ------------------------------------------------------------------------------------------------------------------ per record

_RECORDS = {}


def records(r):
    """once: the box's query rays, their hit and surface records - three ids outside the scene among them - and the restatement"""
    if not _RECORDS:
        cs = P.scene("cbox")
        r.upload_scene(cs)
        rays = R.query_rays("cbox")
        hits, surf = gpu_trace(r)(rays)
        ids = hits[:, 0].copy().view(np.int32)
        hits.view(np.int32)[np.flatnonzero(ids >= 0)[:3], 0] = [cs.num_shapes, 0x7FFFFFFF, -2]
        want, cls, cand = R.continue_rays(cs, rays, hits, surf, detail=True)
        for a in (rays, hits, surf, want, cls):
            a.setflags(write=False)
        _RECORDS["cbox"] = (rays, hits, surf, want, cls, cand)
    return _RECORDS["cbox"]


def test_follow_specular_equals_the_restatement_on_every_class(rq, monkeypatch):
    import torch
    rays, hits, surf, want, cls, _ = records(rq)
    counts = np.bincount(cls, minlength=6)
    print({R.CLASS_NAMES[k]: int(c) for k, c in enumerate(counts)})
    assert (counts >= 16).all(), counts                                 # the condition: every class among the records
    assert len(rays) % 256 != 0
    rq.upload_scene(P.scene("cbox"))
    got = rq.follow_specular(rays, hits)
    same_bits(got, want, "host arrays")
    end = cls == R.END
    assert not got[end][:, 0:6].any() and (got[end, 6] == np.inf).all() and (got[end, 7] == -np.inf).all()
    # the empty ray is a miss at the first node; a continued ray is a ray like any other
    ids = rq.trace_rays(got)[0]
    assert (ids[end] == -1).all() and (ids[~end] >= 0).sum() > 100
    for n in (1, 255, 257):
        same_bits(rq.follow_specular(rays[:n], hits[:n]), want[:n], f"{n} records")
    assert rq.follow_specular(np.zeros((0, 8), F), np.zeros((0, 4), F)).shape == (0, 8)
    dev = f"cuda:{rq.device}"
    tr, th = torch.from_numpy(np.array(rays)).to(dev), torch.from_numpy(np.array(hits)).to(dev)
    out = rq.follow_specular(tr, th)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(rays), 8)
    same_bits(out.cpu().numpy(), want, "device tensors")
    monkeypatch.setenv("HJ_TRACE_CHUNK", "256")
    with device.Renderer(0) as r:
        r.upload_scene(P.scene("cbox"))
        same_bits(r.follow_specular(rays, hits), want, "chunks of 256")
        same_bits(r.follow_specular(tr, th).cpu().numpy(), want, "device tensors in chunks of 256")


def test_the_shade_stage_takes_the_same_step(rq):
    """hj_debug_shade_step - the stage the oracle pins - over the same (ray, hit) records, throughput 1, bounce 0, max_bounces
    large: its next origin is out_rays' origin for every specular hit; its next direction is out_rays' for every mirror and every
    k <= 0 hit and one of the restatement's two candidates for every other dielectric hit, under both RNG states of a pair chosen
    so that both candidates occur."""
    rays, hits, surf, want, cls, cand = records(rq)
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    got = rq.follow_specular(rays, hits)
    spec = np.flatnonzero(cls != R.END)
    o = abi.RenderOpts.default()
    o.max_bounces, o.rr_start = 1000, 1000
    picks = []
    for state in (0x9E3779B9, 0x12345679):
        rec = step_records(rays[spec, 0:3], rays[spec, 3:6], hits[spec, 1], hits[spec, 0].copy().view(np.int32), hits[spec, 2], hits[spec, 3], rng=state)
        out, _ = rq.shade_step(rec, o)
        assert (out[:, 0] == 1).all()                                   # every path stays alive
        same_bits(out[:, 1:4].view(F), got[spec, 0:3], "next origin")
        nd = out[:, 4:7].view(F)
        fixed = (cls[spec] == R.MIRROR) | (cls[spec] == R.REFLECT_TIR)
        same_bits(nd[fixed], got[spec][fixed, 3:6], "mirror and k <= 0: next direction")
        refl = (nd.view(U) == cand["reflect"][spec].view(U)).all(1)
        refr = (nd.view(U) == cand["refract"][spec].view(U)).all(1)
        assert (refl | refr)[~fixed].all(), int((~(refl | refr))[~fixed].sum())
        picks.append((int(refl[~fixed].sum()), int((refr & ~refl)[~fixed].sum())))
    print("reflect / refract picks per RNG state:", picks)
    assert sum(p[0] for p in picks) > 0 and sum(p[1] for p in picks) > 0


# ---------------------------------------------------------------------------------------------------------------------- frames

def block_list(width, height, size, passes):
    """per pass (seed, sample_offset): the raster grid of size x size blocks (ragged at the right and bottom edges)"""
    out = []
    for seed, off in passes:
        for oy in range(0, height, size):
            for ox in range(0, width, size):
                b = abi.ImageBlock()
                b.id, b.seed = len(out), seed + 1000 * len(out)
                b.origin[:], b.dimension[:] = (ox, oy), (min(size, width - ox), min(size, height - oy))
                b.original_dimension[:], b.sample_offset[:] = (width, height), off
                out.append(b)
    return out


def ragged_blocks():
    """40 x 24 in blocks of 16: the edge blocks are 8 wide and 8 high; three passes, then the first pass's first block once more"""
    blocks = block_list(40, 24, 16, [(11, (0.5, 0.5)), (22, (0.125, 0.875)), (33, (0.75, 0.25))])
    assert len(blocks) == 18 and tuple(blocks[2].dimension) == (8, 16) and tuple(blocks[5].dimension) == (8, 8)
    return blocks + [blocks[0]]


def overlapping_blocks():
    blocks = []
    for k, (ox, oy, w, h) in enumerate([(0, 0, 16, 16), (8, 8, 16, 16), (24, 0, 16, 8), (30, 16, 16, 16), (0, 23, 40, 1), (8, 8, 16, 16), (39, 0, 1, 24)]):
        b = abi.ImageBlock()
        b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:] = k, 7 * k, (ox, oy), (w, h), (40, 24)
        b.sample_offset[:] = (0.5, 0.25 + 0.125 * k)
        blocks.append(b)
    return blocks


BLOCKS = {"ragged": (40, 24, ragged_blocks), "overlapping": (40, 24, overlapping_blocks),
          "64": (64, 64, lambda: list(host.make_blocks(64, 64, 2, 31))), "128": (128, 128, lambda: list(host.make_blocks(128, 128, 2, 77))),
          "130": (130, 130, lambda: list(host.make_blocks(130, 130, 2, 77)))}
_WANT = {}


def camera_rays(cs, blocks):
    rays = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    rays[:, 6], rays[:, 7] = P.KEPS, np.inf
    return rays


def expected(r, scene, key, max_follow):
    """(image, chain lengths) of the restatement over hj_trace_rays' own records, computed once per (scene, blocks, max_follow) on a
    renderer without a switch and never written to"""
    k = (scene, key, max_follow)
    if k not in _WANT:
        cs = P.scene(scene) if scene in P.SCENES else EXTRA_SCENES[scene]()
        W, H, make = BLOCKS[key]
        blocks = make()
        r.upload_scene(cs)
        rec, length, _ = R.followed_records(cs, camera_rays(cs, blocks), max_follow, gpu_trace(r))
        img = A.accumulate(W, H, blocks, rec)
        img.setflags(write=False)
        _WANT[k] = (img, length)
    return _WANT[k]


@pytest.mark.parametrize("chunk", [None, "256"])
@pytest.mark.parametrize("scene", ["cbox", "rich"])
def test_followed_block_lists_equal_the_chains(rq, monkeypatch, scene, chunk):
    """ragged and partly overlapping block lists at max_follow 1, 2 and 8, HJ_TRACE_CHUNK unset and at 256 (one block a launch).
    "rich" beside the box: the box's glass sphere holds a diffuse mesh, so its chains end at length 1 (test_follow_host.py); the
    clear glass of "rich" takes them to length 5."""
    wants = {(key, m): expected(rq, scene, key, m) for key in ("ragged", "overlapping") for m in FOLLOWS}
    assert max(int(l.max()) for _, l in wants.values()) >= (3 if scene == "rich" else 1)
    if chunk is not None:
        monkeypatch.setenv("HJ_TRACE_CHUNK", chunk)
    with device.Renderer(0) as r:
        r.upload_scene(P.scene(scene))
        for (key, m), (want, _) in wants.items():
            W, H, make = BLOCKS[key]
            same_bits(r.render_aovs(W, H, blocks=make(), follow=m), want, f"{scene} / {key} / max_follow {m} / chunk {chunk}")
        out = r.render_aovs(40, 24, blocks=ragged_blocks(), follow=2, device=True)
        assert out.is_cuda
        same_bits(out.cpu().numpy(), wants[("ragged", 2)][0], f"{scene} / device array")
        assert not r.render_aovs(40, 24, blocks=[], follow=2).any()


@pytest.mark.parametrize("scene", ["cbox", "rich"])
def test_followed_frames_equal_the_chains(rq, scene):
    """the frame form at 64 x 64 (the condition's frame), at 128 x 128 and at 130 x 130, where a pass has four blocks, two of them two
    pixels wide.  The condition at max_follow = 2: at least 64 chains of length 1 on both scenes, at least 64 of length 2 on
    "rich" (the box has none: test_follow_host.py says why)."""
    cs = P.scene(scene)
    for key, seed in (("64", 31), ("128", 77), ("130", 77)):
        W, H, _ = BLOCKS[key]
        for m in FOLLOWS if key == "64" else (2,):
            want, length = expected(rq, scene, key, m)
            if key == "64" and m == 2:
                print(scene, "chain lengths:", np.bincount(length).tolist())
                assert (length == 1).sum() >= 64 and ((length == 2).sum() >= 64 or scene == "cbox")
            rq.upload_scene(cs)
            same_bits(rq.render_aovs(W, H, spp=2, master_seed=seed, follow=m), want, f"{scene} / frame {key} / max_follow {m}")
    assert host.blocks_per_pass(130, 130) == 4
    want, _ = expected(rq, scene, "130", 2)
    same_bits(rq.render_aovs(130, 130, blocks=BLOCKS["130"][2](), follow=2), want, "block form of the frame")
    one = rq.render_aovs(130, 130, spp=2, master_seed=77, passes=(1, 2), follow=2)
    same_bits(one, rq.render_aovs(130, 130, blocks=BLOCKS["130"][2]()[4:], follow=2), "pass 1 alone")
    # following changes what the specular pixels say, and nothing else
    plain = rq.render_aovs(130, 130, spp=2, master_seed=77)
    assert (plain.view(U) != want.view(U)).any() and (plain[..., [3, 11]].view(U) == want[..., [3, 11]].view(U)).all()


def test_max_follow_zero_and_a_scene_without_a_specular_surface(rq):
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    L = device.lib()
    blocks = ragged_blocks()
    arr = (abi.ImageBlock * len(blocks))(*blocks)
    zero = np.zeros((24, 40, 12), F)
    rq._check(L.hj_render_aovs_followed(rq._h, arr, len(arr), 40, 24, 0, 0, zero.ctypes.data))
    same_bits(zero, rq.render_aovs(40, 24, blocks=blocks), "max_follow 0, block form")
    zero = np.zeros((130, 130, 12), F)
    rq._check(L.hj_render_aovs_frame_followed(rq._h, 130, 130, 2, 77, 0, 2, 0, 0, zero.ctypes.data))
    same_bits(zero, rq.render_aovs(130, 130, spp=2, master_seed=77), "max_follow 0, frame form")
    tex = P.scene("textured")
    tags = set((tex.materials >> abi.MATERIAL_TAG_SHIFT).tolist())
    assert abi.MAT_MIRROR not in tags and abi.MAT_DIELECTRIC not in tags
    rq.upload_scene(tex)
    same_bits(rq.render_aovs(40, 24, blocks=blocks, follow=8), rq.render_aovs(40, 24, blocks=blocks), "no specular surface: no round, the same image")
    same_bits(rq.render_aovs(130, 130, spp=2, master_seed=77, follow=8), rq.render_aovs(130, 130, spp=2, master_seed=77), "... frame form")


@functools.lru_cache(maxsize=None)
def _facing_mirrors():
    """two parallel mirror quads at z = -1 and z = +1 facing each other, 32 x 32: wider than nine segments of any camera ray drift
    sideways; the camera between them, at z = 0.3, looking down -z"""
    s = host.Scene()
    s.set_camera((0.1, 0.05, 0.3), (0, 0, 0, 1), 40.0)
    m = s.add_mirror()
    s.add_quad((-16, -16, -1), (32, 0, 0), (0, 32, 0), m)
    s.add_quad((-16, -16, 1), (0, 32, 0), (32, 0, 0), m)
    return s.compile()


EXTRA_SCENES = {"mirrors": _facing_mirrors}
BLOCKS["mirrors"] = (64, 64, lambda: list(host.make_blocks(64, 64, 2, 9)))


def test_the_cap_between_two_facing_mirrors(rq):
    cs = _facing_mirrors()
    W, H, make = BLOCKS["mirrors"]
    blocks = make()
    rq.upload_scene(cs)
    rays = camera_rays(cs, blocks)
    first = gpu_trace(rq)(rays)[0][:, 0].copy().view(np.int32)
    assert (first == 0).all()                                           # every pixel sees the mirror at z = -1
    cos = np.abs(rays[:, 5].astype(np.float64)) / np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1)
    for m in (1, 8):
        want, length = expected(rq, "mirrors", "mirrors", m)
        assert (length == m).all()                                      # ... and its chain reaches the cap
        rq.upload_scene(cs)
        got = rq.render_aovs(W, H, blocks=blocks, follow=m)
        same_bits(got, want, f"facing mirrors / max_follow {m}")
        # the record is the last mirror's - albedo 1, its normal (0, 0, +-1) - and the depth the sum of max_follow + 1 segments: the
        # first 1.3 along z, every later one 2, all under the camera ray's own angle (a mirror keeps |d.z|)
        rec = R.followed_records(cs, rays, m, gpu_trace(rq))[0]
        assert (rec[:, 0:3] == 1).all() and (rec[:, 4:6] == 0).all() and (rec[:, 6] == (1 if m % 2 == 0 else -1)).all() and (rec[:, 11] == 1).all()
        assert np.abs(rec[:, 7] * cos / (1.3 + 2 * m) - 1).max() < 1e-5


def test_coverage_is_unchanged(rq):
    for scene in ("cbox", "rich"):
        rq.upload_scene(P.scene(scene))
        plain = rq.render_aovs(64, 64, spp=2, master_seed=31)
        for m in (1, 2, 3, 8):
            got = rq.render_aovs(64, 64, spp=2, master_seed=31, follow=m)
            same_bits(got[..., 11], plain[..., 11], f"{scene}: coverage at max_follow {m}")
            same_bits(got[..., 3], plain[..., 3], f"{scene}: sample count at max_follow {m}")


# ------------------------------------------------------------------------------------------------------------------- walk forms

@pytest.mark.parametrize("env", [{"HJ_GROUP_TILE": "1"}, {"HJ_PAIR_LEAVES": "0"}, {"HJ_TRACE_WG_RAYS": "100"}, {"HJ_STREAM_MIN_NODES": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_no_result_bit_changes_under_the_walk_switches(rq, monkeypatch, env):
    """the per-record query and the followed block lists once each in a context created under the switch; the expected values are a
    renderer's without one"""
    text = open(os.path.join(ROOT, "hijiki_amd", "csrc", "api", "hj_tuning.h")).read()
    rays, hits, _, want, _, _ = records(rq)
    wants = {(scene, key): expected(rq, scene, key, 2)[0] for scene in ("cbox", "rich") for key in ("ragged", "64")}
    for k, v in env.items():
        assert f'"{k}"' in text, k
        monkeypatch.setenv(k, v)
    with device.Renderer(0) as r:
        r.upload_scene(P.scene("cbox"))
        same_bits(r.follow_specular(rays, hits), want, f"follow_specular under {env}")
        for (scene, key), w in wants.items():
            r.upload_scene(P.scene(scene))
            W, H, make = BLOCKS[key]
            same_bits(r.render_aovs(W, H, blocks=make(), follow=2), w, f"{scene} / {key} under {env}")


# ------------------------------------------------------------------------------------------------------- neighbours and consumers

def test_a_followed_call_between_two_frames_leaves_them_alone(rq):
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    rq.create_framebuffer(64, 48)

    def two_frames(between):
        rq.clear()
        rq.render_frame(2, 5)
        if between:
            assert rq.render_aovs(64, 48, spp=2, master_seed=5, follow=2)[..., 3].all()
            assert rq.render_aovs(200, 100, spp=1, master_seed=9, follow=8)[..., 3].all()   # (another size than the framebuffer's)
            rays, hits = records(rq)[0:2]
            rq.upload_scene(cs)
            rq.follow_specular(rays[:500], hits[:500])
        rq.render_frame(2, 6)
        return rq.read()

    plain = two_frames(False)
    same_bits(two_frames(True), plain, "second frame")


def test_the_denoiser_takes_the_followed_image(rq):
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    rq.create_framebuffer(64, 48)
    rq.clear()
    rq.render_frame(2, 5)
    beauty = rq.read()
    aov = rq.render_aovs(64, 48, spp=2, master_seed=5, follow=2)
    assert (aov.view(U) != rq.render_aovs(64, 48, spp=2, master_seed=5).view(U)).any()
    same_bits(rq.denoise_frame(aov, beauty, 3), D.run(beauty, aov, 3), "hj_denoise_frame over the followed image / denoise_ref")


def test_cli_writes_the_followed_aovs(rq, tmp_path):
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    head = b"PF\n64 64\n-1.0\n"

    def run(prefix, *extra):
        r = subprocess.run([exe, "--use-bvh", "-w", "64", "-h", "64", "-s", "2", "--seed", "6", "-o", str(tmp_path / "o.pfm"), "--aovs", prefix, *extra,
                            "synthetic:spheres"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return {key: np.frombuffer(open(f"{prefix}_{key}.pfm", "rb").read(), F, offset=len(head)).reshape(64, 64, 3)[::-1] for key in ("albedo", "normal", "depth")}

    plain, followed = run(str(tmp_path / "a")), run(str(tmp_path / "b"), "--aov-follow", "2")
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES).compile()
    rq.upload_scene(cs)
    want = device.resolve_aovs(rq.render_aovs(64, 64, spp=2, master_seed=6, follow=2))
    for key in ("albedo", "normal", "depth"):
        w = want[key] if want[key].ndim == 3 else np.repeat(want[key][..., None], 3, 2)
        same_bits(followed[key], w, key)
    same_bits(plain["albedo"], device.resolve_aovs(rq.render_aovs(64, 64, spp=2, master_seed=6))["albedo"], "without the flag")
    # a pixel whose two samples both hit the mirror sphere first: albedo 1 without the flag, what the mirror shows with it
    hits, _ = gpu_trace(rq)(camera_rays(cs, list(host.make_blocks(64, 64, 2, 6))))
    first = hits[:, 0].copy().view(np.int32).reshape(2, 64, 64)
    tags = cs.materials >> abi.MATERIAL_TAG_SHIFT
    mirror = ((first >= 0) & (tags[np.maximum(first, 0)] == abi.MAT_MIRROR)).all(0)
    assert mirror.sum() > 20 and (plain["albedo"][mirror] == 1).all() and (followed["albedo"][mirror] != 1).any(1).all()
    bad = subprocess.run([exe, "--aov-follow", "2", "-o", str(tmp_path / "o.pfm"), "synthetic:spheres"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--aov-follow without --aovs" in bad.stderr
