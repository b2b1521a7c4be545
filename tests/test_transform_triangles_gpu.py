"""Scene.transform_triangles on the GPU: whole meshes moved by matrix, many ranges in one call.

World vertices are TransformPosition(rest, M) exactly as rt.mesh_to_prims computes them on the host, and
everything after that is update_triangles: the updated scene equals a twin updated with update_triangles
on the mesh_to_prims vertices, the oracle on those vertices over the host-refitted tree, and the host
refit's node bytes -- exactly, no tie allowance.  TEAPOT-F's teapot in three disjoint ranges given out
of order: one triangle, 300 (more than a 256-lane block) and the rest."""
import os

import numpy as np
import pytest

from refit_util import verts_of, with_verts
from scenes_util import oracle_scene
from test_refit_gpu import W, H, assert_frames_equal, assert_rays_equal, gpu_frames, oracle_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def specs(rt):
    return [(rt.MODE_PATH, 1, 1), (rt.MODE_WHITTED, 4, 1), (rt.MODE_PATH, 4, 2)]


@pytest.fixture(scope="module")
def teapot(rt):
    """TEAPOT-F built from the teapot's rest vertices placed by the identity: the light, the mesh's
    triangles [1, 1 + nt), the two floor triangles.  rest: [nt, 9] object-space A, B, C."""
    V, F = rt.load_mesh(os.path.join(rt.DATA_DIR, "teapot.rtmesh"))
    recipe, mats = rt.recipe_describe("teapotF")
    nt = len(F)
    assert len(recipe) == 1 + nt + 2
    ident = np.eye(4, dtype=np.float32).reshape(16)
    # in front of the camera: the recipe's placement is a matrix too, but here the scene starts at rest
    prims = [recipe[0]] + rt.mesh_to_prims(V, F, ident, 1) + recipe[-2:]
    rest = V[F].reshape(nt, 9).astype(np.float32)
    assert np.array_equal(rest.view(np.uint32), verts_of(prims, range(1, 1 + nt)).view(np.uint32))
    nodes, idx, _ = rt.build_bvh_host(prims)
    # (first, count) out of order: the rest, one triangle, 300
    spans = [(1 + 301, nt - 301), (1, 1), (1 + 1, 300)]
    return V, F, prims, mats, nt, rest, nodes, idx, spans


def matrices(rt):
    """rotate x translate x scale, one per range; they bring the teapot in front of the camera"""
    out = []
    for k, (axis, ang, tr, sc) in enumerate([(1, 0.5 * np.pi, (0.0, 0.0, 2.0), 2.5), (0, 0.3, (0.4, 0.9, 0.1), 1.5),
                                             (2, -0.7, (-0.5, 0.2, 0.3), 0.8)]):
        out.append(rt.mat4_mul(rt.mat4_rotate(axis, np.float32(ang)), rt.mat4_translate(*tr), rt.mat4_scale(sc)))
    return out


def rest_of(rest, spans):
    return np.concatenate([rest[f - 1:f - 1 + n] for f, n in spans], axis=0)


def test_three_ranges_equal_update_triangles_and_the_oracle(rt, oracle, torch, specs, teapot):
    V, F, prims, mats, nt, rest, nodes, idx, spans = teapot
    Ms = matrices(rt)
    moved = list(prims)
    for (first, count), M in zip(spans, Ms):
        world = rt.mesh_to_prims(V, F[first - 1:first - 1 + count], M, 1)
        moved = with_verts(rt, moved, range(first, first + count), verts_of(world, range(count)))
    g, twin = rt.Scene(prims, mats), rt.Scene(prims, mats)
    packed = torch.from_numpy(rest_of(rest, spans)).to(f"cuda:{g.device}")
    g.transform_triangles([(f, n, M) for (f, n), M in zip(spans, Ms)], packed)
    twin.update_triangles(1, verts_of(moved, range(1, 1 + nt)))
    host = rt.refit_bvh_host(moved, nodes, idx)
    assert host.tobytes() != nodes.tobytes()
    assert g.bvh()[0].tobytes() == host.tobytes() == twin.bvh()[0].tobytes()
    assert_frames_equal(gpu_frames(rt, g, specs), gpu_frames(rt, twin, specs))
    o = oracle_scene(rt, oracle, moved, mats, bvh=(host, idx))
    assert_rays_equal(g, o)
    assert_frames_equal(gpu_frames(rt, g, specs), oracle_frames(o, specs))


def test_identity_changes_nothing(rt, specs, teapot):
    V, F, prims, mats, nt, rest, nodes, idx, spans = teapot
    g, twin = rt.Scene(prims, mats), rt.Scene(prims, mats)
    ident = np.eye(4, dtype=np.float32).reshape(16)
    g.transform_triangles([(f, n, ident) for f, n in spans], rest_of(rest, spans))     # numpy rest: uploaded
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    assert_frames_equal(gpu_frames(rt, g, specs), gpu_frames(rt, twin, specs))


def test_errors_leave_the_scene_untouched(rt, specs, teapot):
    V, F, prims, mats, nt, rest, nodes, idx, spans = teapot
    g = rt.Scene(prims, mats)
    spec = specs[:1]
    frame0 = gpu_frames(rt, g, spec)
    M = matrices(rt)[0]

    def refused(ranges, code=rt.RT_ERR_INVALID):
        n = sum(c for _, c, _ in ranges)
        with pytest.raises(rt.RTError) as e:
            g.transform_triangles(ranges, np.resize(rest, (n, 9)))
        assert e.value.code == code

    refused([(1, 300, M), (300, 10, M)])                 # overlap by one triangle
    refused([(400, 10, M), (1, 300, M), (405, 1, M)])    # ... out of order, one inside another
    refused([(0, 5, M)])                                 # the light is no triangle
    refused([(nt, 5, M)])                                # ... reaching past the primitives
    refused([(len(prims) - 1, 2, M)])
    big = rt.mat4_scale(3e38)                            # a finite matrix that overflows vertices to infinity
    big[[3, 7, 11]] = 3e38
    assert np.isfinite(big).all() and np.isfinite(rest).all()
    assert not np.isfinite(verts_of(rt.mesh_to_prims(V, F[1:301], big, 1), range(300))).all()
    refused([(1, 1, M), (2, 300, big)])
    nan = np.array(M, np.float32)
    nan[5] = np.nan
    refused([(2, 300, nan)])
    g.transform_triangles([], np.zeros((0, 9), np.float32))              # no range: a no-op
    g.transform_triangles([(7, 0, M)], np.zeros((0, 9), np.float32))     # an empty range is skipped
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    assert_frames_equal(gpu_frames(rt, g, spec), frame0)
    sb = rt.Scene(prims, mats, bvh_kind=rt.BVH_SBVH)
    with pytest.raises(rt.RTError) as e:
        sb.transform_triangles([(1, 10, M)], rest[:10])
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
