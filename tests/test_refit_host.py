"""rt_bvh_refit_host (CPU): the bottom-up box refit behind Scene.update_triangles, on the host.

Boxes are min / max of floats, which never round: with the primitives a tree was built from, the
refit returns the builder's bytes; with deformed primitives it equals the numpy restatement
(refit_util.numpy_refit) byte for byte, and every child box lies inside its parent's."""
import numpy as np
import pytest

from refit_util import (assert_nested, numpy_refit, scene_cases, tree_of, triangle_ids, twist, verts_of,
                        with_verts)

NAMES = ["kat", "teapotF", "chain"]


@pytest.fixture(scope="module")
def cases(rt):
    return scene_cases(rt)


@pytest.mark.parametrize("name", NAMES)
def test_refit_with_unchanged_prims_returns_the_builders_bytes(rt, cases, name):
    prims, _, bvh = cases[name]
    nodes, idx = tree_of(rt, prims, bvh)
    got = rt.refit_bvh_host(prims, nodes, idx)
    assert got.tobytes() == nodes.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_refit_of_deformed_prims_equals_numpy(rt, cases, name):
    prims, _, bvh = cases[name]
    nodes, idx = tree_of(rt, prims, bvh)
    ids = triangle_ids(rt, prims)
    moved = with_verts(rt, prims, ids, twist(verts_of(prims, ids), 0.7))
    got = rt.refit_bvh_host(moved, nodes, idx)
    assert got.tobytes() != nodes.tobytes()          # the twist moved boxes
    assert got.tobytes() == numpy_refit(rt, moved, nodes, idx).tobytes()
    assert_nested(got)
    u0, u1 = nodes.view(np.uint32).reshape(-1, 8), got.view(np.uint32).reshape(-1, 8)
    assert np.array_equal(u0[:, 6:8], u1[:, 6:8])    # topology untouched


def test_refit_rejects_an_sbvh_index_array(rt, cases):
    """A primitive in two leaves (an SBVH's index array repeats ids): RT_ERR_UNSUPPORTED, nodes untouched;
    so is the library's own SBVH, whose leaves reach past the n indices of a plain tree."""
    prims, _, _ = cases["kat"]
    nodes, idx, _ = rt.build_bvh_host(prims)
    rep = idx.copy()
    rep[1] = rep[0]
    with pytest.raises(rt.RTError) as e:
        rt.refit_bvh_host(prims, nodes, rep)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    tprims, _, _ = cases["teapotF"]
    snodes, sidx, info = rt.build_sbvh_host(tprims)
    assert info["num_refs"] > len(tprims)
    with pytest.raises(rt.RTError) as e:
        rt.refit_bvh_host(tprims, snodes, sidx)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED


def test_refit_rejects_a_broken_tree(rt, cases):
    prims, _, _ = cases["kat"]
    nodes, idx, _ = rt.build_bvh_host(prims)
    bad = nodes.copy()
    u = bad.view(np.uint32).reshape(-1, 8)
    assert u[0, 7] == 0
    u[0, 6] = len(nodes) + 4                         # child pair out of range
    with pytest.raises(rt.RTError) as e:
        rt.refit_bvh_host(prims, bad, idx)
    assert e.value.code == rt.RT_ERR_INVALID
    u[0, 6] = 0                                      # the root is its own child: a cycle
    with pytest.raises(rt.RTError) as e:
        rt.refit_bvh_host(prims, bad, idx)
    assert e.value.code == rt.RT_ERR_INVALID
