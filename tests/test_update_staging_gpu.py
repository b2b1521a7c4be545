"""The host-memory calls of a scene share one staging buffer, grown on demand (grow, csrc/rt_refit.h):
update_prims and update_triangles from host arrays and the staged ray batches.  In one scene's
lifetime a small update, a ray batch that regrows the buffer, an update that fits the regrown buffer
and the small update again must each leave the scene exactly as the same call fed device tensors
leaves a second scene: the tree bytes, and the hits of a fixed ray batch bit for bit."""
import numpy as np
import pytest

from refit_util import triangle_ids, twist, verts_of
from test_refit_gpu import random_rays
from test_update_prims_gpu import device_prims

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def hit_bytes(hits):
    return b"".join(np.ascontiguousarray(x.cpu().numpy()).tobytes() for x in hits)


def test_staged_calls_share_one_buffer(rt, torch):
    prims, mats = rt.recipe_describe("teapotF")
    n = len(prims)
    prims = prims + [rt.sphere((-2.0, 0.2, 3.0), 0.4, 1)]
    tri = triangle_ids(rt, prims)
    assert len(tri) == 1026 and prims[n - 1].type == rt.TRIANGLE
    g, twin = rt.Scene(prims, mats), rt.Scene(prims, mats)
    fixed = torch.from_numpy(random_rays(1024, 11)).cuda()
    seen = []

    def same():
        gb, tb = g.bvh(), twin.bvh()
        assert gb[0].tobytes() == tb[0].tobytes() and np.array_equal(gb[1], tb[1])
        hg = hit_bytes(g.IntersectBVH(fixed))
        assert hg == hit_bytes(twin.IntersectBVH(fixed))
        seen.append((gb[0].tobytes(), hg))

    same()
    v = [float(x) for x in prims[n - 1].v]

    def pair(dy, c):
        """two records: the last triangle lifted by dy, the sphere at c"""
        return [rt.triangle((v[0], v[1] + dy, v[2]), (v[3], v[4] + dy, v[5]), (v[6], v[7] + dy, v[8]), prims[n - 1].material),
                rt.sphere(c, 0.3, 1)]

    first = pair(0.5, (-1.6, 0.6, 2.6))
    g.update_prims(n - 1, first)                                     # 1. two records from host memory
    twin.update_prims(n - 1, device_prims(rt, torch, twin, first))
    same()
    rays = random_rays(4096, 3)                                      # 2. a staged ray batch regrows the buffer
    hits = g.intersect_host(rays)
    t, obj, u, w = (x.cpu().numpy() for x in twin.IntersectBVH(torch.from_numpy(rays).cuda()))
    assert (obj >= 0).sum() > 100
    assert hits["t"].tobytes() == t.tobytes() and np.array_equal(hits["obj"], obj)
    assert hits["u"].tobytes() == u.tobytes() and hits["v"].tobytes() == w.tobytes()
    same()
    ids = tri[100:400]                                               # 3. 300 triangles from a numpy array
    moved = twist(verts_of(prims, ids), 0.15)
    g.update_triangles(int(ids[0]), moved)
    twin.update_triangles(int(ids[0]), torch.from_numpy(moved).cuda())
    same()
    second = pair(-0.25, (-2.2, 0.1, 3.3))
    g.update_prims(n - 1, second)                                    # 4. the two-record host update again
    twin.update_prims(n - 1, device_prims(rt, torch, twin, second))
    same()
    # every update moved the tree; the ray batch moved nothing
    assert seen[2] == seen[1]
    for a, b in ((0, 1), (2, 3), (3, 4)):
        assert seen[a][0] != seen[b][0]
