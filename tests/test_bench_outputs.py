"""bench.py --dump-outputs on the CPU: what it writes for a frame small enough to keep whole (c2, c3) and for one it samples
(c4's 2048 x 2048): float32 / float64 files, at most 64 MB in all, the same pixels from run to run."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    # bench.py sets a default GPU_MAX_HW_QUEUES for its own process when imported: keep this process's value as it is
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _written(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}, sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))


def test_whole_frame(bench, tmp_path):
    frame = np.random.default_rng(1).random((1024, 1024, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "o"), frame)
    files, size = _written(tmp_path / "o")
    assert list(files) == ["frame.npy"] and size <= 64 << 20
    assert files["frame.npy"].dtype == np.float32 and (files["frame.npy"].view(np.uint32) == frame.view(np.uint32)).all()


def test_large_frame_is_a_fixed_sample(bench, tmp_path):
    H = W = 2048
    picks = []
    for run, seed in enumerate((2, 3)):
        frame = np.random.default_rng(seed).random((H, W, 4), dtype=np.float32)
        bench.dump_outputs(str(tmp_path / str(run)), frame)
        files, size = _written(tmp_path / str(run))
        assert list(files) == ["frame_sample.npy", "frame_sample_pixels.npy"] and size <= 64 << 20
        smp, pix = files["frame_sample.npy"], files["frame_sample_pixels.npy"]
        assert smp.dtype == np.float32 and pix.dtype == np.float64 and smp.shape == (len(pix), 4) and len(pix) >= 1 << 20
        idx = pix.astype(np.int64)
        assert (idx == pix).all() and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < H * W
        assert (smp.view(np.uint32) == frame.reshape(H * W, 4)[idx].view(np.uint32)).all()
        picks.append(idx)
    assert (picks[0] == picks[1]).all()            # the pixels depend on the frame's size alone
