"""hj_scene_update_shapes, the part that needs no GPU: the symbols are declared, listed and exported, a null context is refused, and
the numpy restatement of the guard-box formula (tests/update_scenes.py, the GPU tests' yardstick) has the properties the upload's
comment states.  No host-side path reaches the upload's guard records: the GPU probe pins the formula (test_scene_update_gpu.py)."""
import numpy as np
import pytest

import refit_scenes
import update_scenes as U
from hijiki_amd import abi, device, host
from test_abi import declared_functions


def test_update_entry_points_are_declared_listed_and_exported():
    for name in ("hj_scene_update_shapes", "hj_debug_scene_tree"):
        assert name in declared_functions("hijiki_hip.h")
        assert name in device.EXPORTS
        assert hasattr(device.lib(), name)
    L = device.lib()
    assert L.hj_version() >= 0x000700
    assert L.hj_scene_update_shapes(None, None, 0, None) == abi.HJ_ERR_INVALID       # (a null context: no device touched)
    assert L.hj_debug_scene_tree(None, None, 0, None, None) == abi.HJ_ERR_INVALID
    assert callable(device.Renderer.update_shapes) and callable(device.Renderer.scene_tree)
    assert abi.UPDATE_DEVICE_ARRAYS == 1 and abi.UPDATE_NO_LIGHT_GRID == 2
    header = open(declared_functions.__globals__["ROOT"] + "/include/hijiki_hip.h").read()
    assert "#define HJ_UPDATE_DEVICE_ARRAYS 1u" in header and "#define HJ_UPDATE_NO_LIGHT_GRID 2u" in header


@pytest.mark.parametrize("kind", [host.SYNTH_CBOX, host.SYNTH_CBOX_SPHERES])
def test_numpy_guard_boxes_contain_their_padded_shapes(kind):
    """A check of the yardstick itself, not of the library: it passes without hj_scene_update_shapes.  The numpy restatement that the
    GPU tests compare guard records with must at least pad every shape's bounds by the absolute part and by little more than a
    thousandth of its size; that it IS the upload's formula, bit for bit, only test_scene_update_gpu.py can show, through the probe."""
    cs = host.Scene.synthetic(kind, mesh_triangles=1280).compile()
    d = refit_scenes.Deformation(cs, seed=3)
    d.apply(0.03, t=0.5)
    want = U.refitted(cs, cs.bvh)
    f = want.view(np.float32)
    gmin, gmax = U.guard_boxes(cs, f[0, 0:3], f[0, 4:7])
    lo, hi = refit_scenes.shape_boxes(cs)
    assert gmin.dtype == np.float32 and gmin.shape == lo.shape
    assert (gmin < lo - np.float32(1.9e-4)).all() and (gmax > hi + np.float32(1.9e-4)).all()    # the absolute padding, at least
    size = (hi - lo).max(axis=1)
    assert ((lo - gmin).max(axis=1) < 1.1e-3 * size + 4e-4).all()                               # ... and not much more than a thousandth
    d.restore()
