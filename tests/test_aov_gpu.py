"""hj_eval_materials, hj_render_aovs and hj_render_aovs_frame on the GPU against aov_ref - the contract restated in numpy - bit for bit
on every word: the material of every first hit of the four query scenes' ray sets (every tag, misses, ids outside the scene), from
host arrays, device tensors and in chunks; the AOV sums of a block list with ragged edge blocks, three passes and a repeated block,
one block a launch and all in one; the normals and depths of a block against hj_debug_samples; a 130 x 130 frame - blocks two pixels
wide - through the frame form, the block form and the restatement; a frame before and after; the command line's three PFMs."""
import os
import subprocess

import numpy as np
import pytest

import aov_ref as A
import path_query_ref as P
from hijiki_amd import abi, device, host
from test_abi import ROOT

pytestmark = pytest.mark.gpu

U, F = np.uint32, np.float32


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(U) != want.view(U)
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} words differ, first at {at}: {got[at[:-1]].tolist()} / {want[at[:-1]].tolist()}")


@pytest.fixture(scope="module")
def rq():
    with device.Renderer(0) as r:
        yield r


def query_rays(name):
    rays = np.array(P.ray_set(name))
    rays[:, 6], rays[:, 7] = P.KEPS, np.inf
    return rays


def hit_records(r, rays):
    """hj_trace_rays' two arrays for `rays`: hits (n, 4: id bits, t, u, v) and surface (n, 16)"""
    ids, t, u, v, surf = r.trace_rays(rays, surface=True)
    return np.stack([ids.view(F), t, u, v], 1), surf


# -------------------------------------------------------------------------------------------------------------- eval_materials

_RECORDS = {}


def records(r, name):
    """per scene, once: the ray set's hit and surface records - three ids outside the scene among them - and the reference"""
    if name not in _RECORDS:
        cs = P.scene(name)
        r.upload_scene(cs)
        hits, surf = hit_records(r, query_rays(name))
        ids = hits[:, 0].copy().view(np.int32)
        tags = cs.materials >> abi.MATERIAL_TAG_SHIFT
        for tag in sorted(set(tags.tolist())):                          # the premise: every tag gets first hits, and rays miss
            assert int(((ids >= 0) & (tags[np.maximum(ids, 0)] == tag)).sum()) >= 20, (name, tag)
        assert int((ids < 0).sum()) >= 100, name
        hit = np.flatnonzero(ids >= 0)[:3]
        hits.view(np.int32)[hit, 0] = [cs.num_shapes, 0x7FFFFFFF, -2]   # outside [0, shapes): a miss, whatever the surface record says
        ids = hits[:, 0].copy().view(np.int32)
        want = A.materials(cs, cs.textures, ids, surf[:, 6], surf[:, 7])
        for a in (hits, surf, want):
            a.setflags(write=False)
        _RECORDS[name] = (hits, surf, want)
    return _RECORDS[name]


@pytest.mark.parametrize("name", list(P.SCENES))
def test_eval_materials_equals_the_restatement_on_every_tag(rq, name):
    hits, surf, want = records(rq, name)
    rq.upload_scene(P.scene(name))
    assert len(hits) % 256 != 0
    got = rq.eval_materials(hits, surf)
    same_bits(got, want, name)
    word = got.view(U)[:, 3]
    assert (word == abi.MATERIAL_MISS).sum() >= 103 and not got[word == abi.MATERIAL_MISS][:, [0, 1, 2, 4, 5, 6, 7]].any()
    for n in (1, 255, 257):
        same_bits(rq.eval_materials(hits[:n], surf[:n]), want[:n], f"{name} / {n} records")
    assert rq.eval_materials(np.zeros((0, 4), F), np.zeros((0, 16), F)).shape == (0, 8)


def test_eval_materials_from_device_tensors_and_in_chunks(rq, monkeypatch):
    import torch
    name = "env"
    hits, surf, want = records(rq, name)
    rq.upload_scene(P.scene(name))
    dev = f"cuda:{rq.device}"
    th, ts = torch.from_numpy(np.array(hits)).to(dev), torch.from_numpy(np.array(surf)).to(dev)
    out = rq.eval_materials(th, ts)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(hits), 8)
    same_bits(out.cpu().numpy(), want, "device tensors")
    monkeypatch.setenv("HJ_TRACE_CHUNK", "1000")
    with device.Renderer(0) as r:
        r.upload_scene(P.scene(name))
        same_bits(r.eval_materials(hits, surf), want, "chunks of 1000")
        same_bits(r.eval_materials(th, ts).cpu().numpy(), want, "device tensors in chunks of 1000")


# ------------------------------------------------------------------------------------------------------------------ render_aovs

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


def expected_aovs(r, cs, width, height, blocks):
    """the restatement over hj_trace_rays' records of the blocks' camera rays (the scene is uploaded on r)"""
    rays = np.concatenate([P.camera_rays(cs, b) for b in blocks])
    rays[:, 6], rays[:, 7] = P.KEPS, np.inf
    hits, surf = hit_records(r, rays)
    return A.accumulate(width, height, blocks, A.sample_records(cs, blocks, hits, surf))


def ragged_blocks():
    """40 x 24 in blocks of 16: the edge blocks are 8 wide and 8 high; three passes, then the first pass's first block once more"""
    blocks = block_list(40, 24, 16, [(11, (0.5, 0.5)), (22, (0.125, 0.875)), (33, (0.75, 0.25))])
    assert len(blocks) == 18 and tuple(blocks[2].dimension) == (8, 16) and tuple(blocks[5].dimension) == (8, 8)
    return blocks + [blocks[0]]


_AOVS = {}


@pytest.mark.parametrize("chunk", ["256", None])
@pytest.mark.parametrize("name", ["cbox", "textured"])
def test_render_aovs_sums_the_blocks_in_list_order(rq, monkeypatch, name, chunk):
    cs = P.scene(name)
    blocks = ragged_blocks()
    if name not in _AOVS:
        rq.upload_scene(cs)
        _AOVS[name] = expected_aovs(rq, cs, 40, 24, blocks)
        _AOVS[name].setflags(write=False)
    want = _AOVS[name]
    assert (want[..., 3] == 3).sum() == 40 * 24 - 256 and (want[:16, :16, 3] == 4).all()       # the repeated block's pixels: four samples
    assert (want[..., 11] > 0).any() and (want[..., 11] < want[..., 3]).any() and want[..., 0:3].any()
    if chunk is not None:
        monkeypatch.setenv("HJ_TRACE_CHUNK", chunk)                     # one block a launch: every run is cut into launches
    with device.Renderer(0) as r:
        r.upload_scene(cs)
        same_bits(r.render_aovs(40, 24, blocks=blocks), want, f"{name} / chunk {chunk}")
        out = r.render_aovs(40, 24, blocks=blocks, device=True)
        assert out.is_cuda
        same_bits(out.cpu().numpy(), want, f"{name} / chunk {chunk} / device array")
        assert not r.render_aovs(40, 24, blocks=[]).any()                # no blocks: an all-zero image


def test_blocks_that_overlap_in_part_and_reach_over_the_edge(rq):
    """rectangles at origins off the block grid: each overlap cuts a run, and the samples beyond the image's edge are dropped"""
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    blocks = []
    for k, (ox, oy, w, h) in enumerate([(0, 0, 16, 16), (8, 8, 16, 16), (24, 0, 16, 8), (30, 16, 16, 16), (0, 23, 40, 1), (8, 8, 16, 16), (39, 0, 1, 24)]):
        b = abi.ImageBlock()
        b.id, b.seed, b.origin[:], b.dimension[:], b.original_dimension[:] = k, 7 * k, (ox, oy), (w, h), (40, 24)
        b.sample_offset[:] = (0.5, 0.25 + 0.125 * k)
        blocks.append(b)
    want = expected_aovs(rq, cs, 40, 24, blocks)
    assert want[12, 12, 3] == 3 and want[20, 35, 3] == 1 and want[23, 35, 3] == 2 and want[0, 39, 3] == 2 and want[..., 3].sum() == 256 * 3 + 128 + 80 + 40 + 24
    same_bits(rq.render_aovs(40, 24, blocks=blocks), want, "overlapping blocks")


def test_normals_and_depths_are_the_frame_s_own(rq):
    """words 4..7 of a one-block render_aovs are hj_debug_samples' first-hit normal and t, bit for bit"""
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    block = P.camera_block()
    aov = rq.render_aovs(32, 32, blocks=[block])
    smp = rq.samples(block)
    same_bits(aov[..., 4:8], smp[..., 4:8], "normal and t")
    assert (aov[..., 3] == 1).all() and ((aov[..., 11] == 1) == (smp[..., 7] != 0)).all() and (aov[..., 11] == 0).any() and (aov[..., 11] == 1).any()


def test_frame_form_at_the_128_boundary(rq):
    W = H = 130
    spp, seed = 2, 77
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    assert host.blocks_per_pass(W, H) == 4
    blocks = host.make_blocks(W, H, spp, seed)
    assert len(blocks) == 8 and sorted(tuple(b.dimension) for b in blocks[:4]) == [(2, 2), (2, 128), (128, 2), (128, 128)]
    frame = rq.render_aovs(W, H, spp=spp, master_seed=seed)
    same_bits(frame, rq.render_aovs(W, H, blocks=blocks), "frame form / block form")
    same_bits(frame, expected_aovs(rq, cs, W, H, list(blocks)), "frame form / restatement")
    assert (frame[..., 3] == spp).all()
    one = rq.render_aovs(W, H, spp=spp, master_seed=seed, passes=(1, 2))
    same_bits(one, rq.render_aovs(W, H, blocks=list(blocks)[4:]), "pass 1 alone")
    assert not rq.render_aovs(W, H, spp=spp, master_seed=seed, passes=(1, 1)).any()


def test_a_call_between_two_frames_leaves_them_alone(rq):
    cs = P.scene("cbox")
    rq.upload_scene(cs)
    rq.create_framebuffer(64, 48)

    def two_frames(between):
        rq.clear()
        rq.render_frame(2, 5)
        if between:
            assert rq.render_aovs(64, 48, spp=2, master_seed=5)[..., 3].all()
            assert rq.render_aovs(200, 100, spp=1, master_seed=9)[..., 3].all()   # (another size than the framebuffer's)
        rq.render_frame(2, 6)
        return rq.read()

    plain = two_frames(False)
    same_bits(two_frames(True), plain, "second frame")


def test_cli_writes_the_resolved_aovs(rq, tmp_path):
    exe = os.path.join(ROOT, "hijiki_amd", "bin", "hijiki-hip")
    prefix = str(tmp_path / "a")
    r = subprocess.run([exe, "--use-bvh", "-w", "64", "-h", "64", "-s", "2", "--seed", "6", "-o", str(tmp_path / "o.pfm"), "--aovs", prefix, "synthetic:cbox"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rq.upload_scene(host.Scene.synthetic(host.SYNTH_CBOX).compile())
    want = device.resolve_aovs(rq.render_aovs(64, 64, spp=2, master_seed=6))
    head = b"PF\n64 64\n-1.0\n"
    for key in ("albedo", "normal", "depth"):
        got = np.frombuffer(open(f"{prefix}_{key}.pfm", "rb").read(), F, offset=len(head)).reshape(64, 64, 3)[::-1]
        w = want[key] if want[key].ndim == 3 else np.repeat(want[key][..., None], 3, 2)
        same_bits(got, w, key)
    assert want["albedo"].any() and want["depth"].any()
