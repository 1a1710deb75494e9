"""hj_refit_bvh_device, the part that needs no GPU: the symbol is declared, listed and exported, and the yardsticks of
tests/test_refit_gpu.py (the numpy restatement of the refit, the deformation helper) are themselves checked on the CPU."""
import numpy as np
import pytest

import refit_scenes
from hijiki_amd import abi, device, host
from test_abi import declared_functions
from test_gpu_parity import _check_skip_link_tree, _shape_boxes


def test_refit_entry_point_is_declared_listed_and_exported():
    assert "hj_refit_bvh_device" in declared_functions("hijiki_hip.h")
    assert "hj_refit_bvh_device" in device.EXPORTS
    L = device.lib()
    assert hasattr(L, "hj_refit_bvh_device")
    assert L.hj_version() >= 0x000600
    assert L.hj_refit_bvh_device(None, None, None, 0, None, None) == abi.HJ_ERR_INVALID      # (a null context: no device touched)
    assert callable(device.Renderer.refit_bvh)


@pytest.mark.parametrize("kind", [host.SYNTH_CBOX, host.SYNTH_CBOX_SPHERES])
def test_numpy_restatement_of_the_refit_is_a_valid_tree(kind):
    """The GPU test's yardstick before it travels: refitting the host-compiled tree of a DEFORMED scene in numpy gives an array that
    satisfies every invariant of the flattened tree for the deformed shapes, keeps the links, and differs from the stale tree."""
    cs = host.Scene.synthetic(kind, mesh_triangles=1280).compile()
    topo = cs.bvh.copy()
    assert (refit_scenes.shape_boxes(cs)[0] == _shape_boxes(cs)[0]).all() and (refit_scenes.shape_boxes(cs)[1] == _shape_boxes(cs)[1]).all()
    d = refit_scenes.Deformation(cs, seed=3)
    d.apply(0.03, t=0.5)
    moved = _shape_boxes(cs)
    got = refit_scenes.refit_numpy(topo, moved)
    _check_skip_link_tree(got, moved)
    assert (got[:, 3] == topo[:, 3]).all() and (got[:, 7] == topo[:, 7]).all()
    assert (got[:, 0:3] != topo[:, 0:3]).any()
    with pytest.raises(AssertionError):
        _check_skip_link_tree(topo, moved)                                 # the stale boxes do not bound the moved shapes
    cost = refit_scenes.sa_cost(got)
    assert np.isfinite(cost) and cost >= 1.0                               # the root itself counts 1
    d.restore()
    print("unmoved refit reproduces Scene::compile's boxes:", bool((refit_scenes.refit_numpy(topo, _shape_boxes(cs)) == topo).all()))


def test_numpy_restatement_on_a_chain():
    cs = refit_scenes.sphere_chain_scene(300)
    chain = refit_scenes.chain_topology(300)
    d = refit_scenes.Deformation(cs, seed=5)
    d.apply(0.02, t=1.0)
    got = refit_scenes.refit_numpy(chain, _shape_boxes(cs))
    _check_skip_link_tree(got, _shape_boxes(cs))


def test_deformation_helper_refuses_to_move_an_emitter():
    cs = host.Scene.synthetic(host.SYNTH_CBOX_SPHERES, mesh_triangles=1280).compile()
    d = refit_scenes.Deformation(cs, seed=1)
    assert len(cs.emitters) > 0 and d.emitter_shapes.any()
    ns, nq = len(cs.spheres), len(cs.quads)
    shape = int(cs.emitters[0, 0])
    before = (cs.vertices.copy(), cs.spheres.copy(), cs.quads.copy())
    with pytest.raises(ValueError):
        if shape < ns:
            d.apply(0.01, spheres=[shape])
        elif shape < ns + nq:
            d.apply(0.01, quads=[shape - ns])
        else:
            d.apply(0.01, vertices=cs.triangles[shape - ns - nq])
    assert all((a == b).all() for a, b in zip(before, (cs.vertices, cs.spheres, cs.quads)))   # refused before anything moved
    d.apply(0.02, t=0.3)                                                   # the default moves everything else ...
    assert len(d.free_vertices) + len(d.free_spheres) + len(d.free_quads) > 0
    assert (cs.vertices[:, 0:3] != before[0][:, 0:3]).any() or (cs.spheres != before[1]).any()
    tri_em = d.emitter_shapes[ns + nq:]
    assert (cs.vertices[cs.triangles[tri_em].reshape(-1)] == before[0][cs.triangles[tri_em].reshape(-1)]).all()   # ... and no emitter
    d.restore()
    assert all((a == b).all() for a, b in zip(before, (cs.vertices, cs.spheres, cs.quads)))
