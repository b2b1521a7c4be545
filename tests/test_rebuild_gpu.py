"""Scene.rebuild on the GPU: the BVH rebuilt from the scene's current primitives, bit for bit the
tree rt_bvh_build_host builds for them, so that a rebuilt scene is indistinguishable from a scene
created fresh from those primitives -- node and index bytes, info, hit ids and t / u / v bits,
occlusion, RGB8 frames and accumulator bits in every mode, the wave walk's counters.  Frames are
64 x 64; kBuildWide (csrc/rt_build.h) is the node size above which many workgroups split a node."""
import numpy as np
import pytest

from anim_util import MOVERS, room_mats, room_prims, with_prims
from refit_util import scene_cases, triangle_ids, twist, verts_of, with_verts
from scenes_util import oracle_scene
from test_refit_gpu import assert_frames_equal, random_rays, update

pytestmark = pytest.mark.gpu

W, H = 64, 64
BUILD_WIDE = 64       # kBuildWide of csrc/rt_build.h


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cases(rt):
    return scene_cases(rt)


@pytest.fixture(scope="module")
def teapot_twisted(rt, cases):
    """TEAPOT-F, its triangle ids, and the scene twisted by 1 rad per unit of y"""
    prims, mats, _ = cases["teapotF"]
    ids = triangle_ids(rt, prims)
    return prims, mats, ids, with_verts(rt, prims, ids, twist(verts_of(prims, ids), 1.0))


def soup(rt, n, seed):
    """the light and n - 1 small random triangles"""
    rng = np.random.default_rng(seed)
    c = rng.uniform((-5, -2, 2), (5, 2, 8), (n - 1, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-0.15, 0.15, (n - 1, 3, 3)).astype(np.float32)).astype(np.float32)
    return [rt.sphere((0, 8, 0), 0.5, 0)] + [rt.triangle(t[0], t[1], t[2], 1) for t in v]


def soup_mats(rt):
    return [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.DIFFUSE, (0.8, 0.6, 0.5))]


def frames(rt, g, specs):
    """[(rgb8, accumulator)] per (mode, depth, spp), frame 0 with reset"""
    out = []
    for mode, depth, spp in specs:
        r = rt.Renderer(g, W, H)
        r.mode = mode
        rgb = r.tick_host(spp=spp, depth=depth, frame=0, reset=True)
        out.append((rgb.copy(), r.accumulator().copy()))
        r.close()
    return out


def walk_frame(rt, g):
    g.set_camera_walk(rt.WALK_WAVE)
    r = rt.Renderer(g, W, H)
    r.set_walk_check(rt.WALK_CHECK_VERIFY)
    rgb = r.tick_host(spp=1, depth=1, frame=0, reset=True)
    out = (rgb.copy(), r.accumulator().copy(), r.walk_stats())
    r.close()
    return out


def all_specs(rt):
    return [(rt.MODE_PATH, 1, 1), (rt.MODE_PATH, 4, 2), (rt.MODE_WHITTED, 4, 1), (rt.MODE_PACKET, 1, 1)]


def assert_tree_is_hosts(rt, g, prims):
    nodes, idx, info = rt.build_bvh_host(prims)
    gn, gi = g.bvh()
    assert g.info["nodes_used"] == info["nodes_used"] and g.info["depth"] == info["depth"]
    assert gn.tobytes() == nodes[:info["nodes_used"]].tobytes(), "node bytes differ from the host builder's"
    assert np.array_equal(gi, idx), "index array differs from the host builder's"


def assert_same_as_twin(rt, oracle, g, twin, prims, mats, specs):
    """hits on 4,096 random rays and the camera rays, occlusion, frames"""
    assert g.info == twin.info
    o = oracle_scene(rt, oracle, prims, mats, bvh=twin.bvh())
    cam = o.camera_rays(W, H, np.arange(W * H, dtype=np.int32))
    for k, rays in enumerate((random_rays(4096, 11), cam)):
        a, b = g.intersect_host(rays), twin.intersect_host(rays)
        assert a.tobytes() == b.tobytes(), "t / obj / u / v bits differ from the twin's"
        short = rays.copy()
        short[:, 6] = np.random.default_rng(3 + k).uniform(0.0, 8.0, len(rays)).astype(np.float32)
        assert np.array_equal(g.occluded_host(short), twin.occluded_host(short))
    assert_frames_equal(frames(rt, g, specs), frames(rt, twin, specs))


@pytest.mark.parametrize("name", ["kat", "leaf", "teapotF", "soup"])
def test_fresh_scene_rebuilds_to_the_hosts_tree(rt, torch, cases, name):
    if name == "soup":
        prims, mats, bvh = soup(rt, 4 * BUILD_WIDE + 3, 5), soup_mats(rt), None
    else:
        prims, mats, bvh = cases[name]
    g, twin = rt.Scene(prims, mats, bvh=bvh), rt.Scene(prims, mats)
    r = rt.Renderer(g, W, H)
    r.tick_host(spp=1, depth=1, frame=0, reset=True)     # a renderer has run on the old tree
    g.rebuild()
    assert_tree_is_hosts(rt, g, prims)
    assert g.info == twin.info
    st = g.rebuild_stats()
    print(name, "rebuild stats", st)
    # the launch order: init, seven steps a level, the subtrees if any, three scans and emit, permute, a box pass per depth
    assert st[3] == 1 + 7 * st[0] + (1 if st[2] else 0) + 4 + 1 + (g.info["depth"] + 1)
    if name == "soup":                                  # both kernel paths ran
        assert st[0] >= 2 and st[1] > 0 and st[2] > 0
    if name == "leaf":                                   # the one-leaf tree was split, by one workgroup
        assert g.info["nodes_used"] > 2 and st[1] == 0 and st[2] == 1
    rgb = r.tick_host(spp=1, depth=1, frame=0, reset=True)
    t = rt.Renderer(twin, W, H)
    assert np.array_equal(rgb, t.tick_host(spp=1, depth=1, frame=0, reset=True))
    assert r.accumulator().tobytes() == t.accumulator().tobytes()
    r.close()
    t.close()


def test_update_then_rebuild_equals_a_fresh_scene(rt, oracle, torch, teapot_twisted):
    prims, mats, ids, moved = teapot_twisted
    g = rt.Scene(prims, mats)
    update(g, moved, ids, device=torch)                  # the vertices exist on the device only
    refit_nodes = g.bvh()[0].copy()
    g.rebuild()
    assert_tree_is_hosts(rt, g, moved)
    assert g.bvh()[0].tobytes() != refit_nodes.tobytes()
    twin = rt.Scene(moved, mats)
    assert_same_as_twin(rt, oracle, g, twin, moved, mats, all_specs(rt))
    a, b = walk_frame(rt, g), walk_frame(rt, twin)
    print("walk stats (rebuilt, fresh):", a[2], b[2])
    assert a[2] == b[2] and a[2]["walked"] > 0 and a[2]["verify_mismatch"] == 0
    assert_frames_equal([a[:2]], [b[:2]])


def test_every_kind_moves_then_rebuilds(rt, oracle, torch):
    """the animated room's movers -- the quad light, the bouncing sphere, the spinning cube -- at a
    second pose through update_prims, and the KAT scene's spheres (its light among them); the
    depth-4 frames pin the light's sampling"""
    base, mats = room_prims(rt, 0.0), room_mats(rt)
    pose = room_prims(rt, 1.3)
    new = base
    for i in MOVERS:
        new = with_prims(new, i, [pose[i]])
    g = rt.Scene(base, mats)
    for i in MOVERS:
        g.update_prims(i, [new[i]])
    g.rebuild()
    assert_tree_is_hosts(rt, g, new)
    assert_same_as_twin(rt, oracle, g, rt.Scene(new, mats), new, mats, all_specs(rt))
    kp, km, _ = scene_cases(rt)["kat"]
    k2 = with_prims(with_prims(kp, 0, [rt.sphere((1.5, 3.0, 1.0), 0.8, 0)]), 5, [rt.sphere((-4.0, 0.5, 9.0), 1.0, 2)])
    g = rt.Scene(kp, km)
    g.update_prims(0, [k2[0]])
    g.update_prims(5, [k2[5]])
    g.rebuild()
    assert_tree_is_hosts(rt, g, k2)
    assert_same_as_twin(rt, oracle, g, rt.Scene(k2, km), k2, km, all_specs(rt))


def test_life_after_a_rebuild(rt, torch, teapot_twisted):
    """rebuild -> update (a second pose) equals a twin created at the first pose and updated: the refit
    schedule and the slot map follow the new tree; a second rebuild is the host's tree again; and
    transform_triangles runs on a rebuilt scene"""
    prims, mats, ids, pose1 = teapot_twisted
    pose2 = with_verts(rt, prims, ids, twist(verts_of(prims, ids), -0.4))
    g = rt.Scene(prims, mats)
    update(g, pose1, ids, device=torch)
    g.rebuild()
    update(g, pose2, ids, device=torch)
    twin = rt.Scene(pose1, mats)
    update(twin, pose2, ids)
    assert g.bvh()[0].tobytes() == twin.bvh()[0].tobytes() and np.array_equal(g.bvh()[1], twin.bvh()[1])
    specs = [(rt.MODE_PATH, 1, 1), (rt.MODE_PATH, 4, 2)]
    assert_frames_equal(frames(rt, g, specs), frames(rt, twin, specs))
    rays = random_rays(4096, 12)
    assert g.intersect_host(rays).tobytes() == twin.intersect_host(rays).tobytes()
    g.rebuild()
    assert_tree_is_hosts(rt, g, pose2)
    # every triangle back to its rest pose by the identity matrix
    first, n = int(ids[0]), len(ids)
    rest = verts_of(prims, ids)
    g.transform_triangles([(first, n, rt.mat4_translate(0, 0, 0))], rest)
    twin2 = rt.Scene(pose2, mats)
    update(twin2, prims, ids)
    assert g.bvh()[0].tobytes() == twin2.bvh()[0].tobytes()
    assert_frames_equal(frames(rt, g, specs[:1]), frames(rt, twin2, specs[:1]))
    g.rebuild()
    assert_tree_is_hosts(rt, g, prims)


def test_refusal_leaves_the_scene_untouched(rt, torch, cases):
    """300 distinct triangles moved onto one another refit fine, but their tree is one leaf of 300"""
    prims, mats = soup(rt, 301, 6), soup_mats(rt)
    g = rt.Scene(prims, mats)
    one = rt.triangle((0, 0, 4), (1.5, 0, 4), (0, 1.5, 4), 1)
    g.update_prims(1, [one] * 300)
    spec = [(rt.MODE_PATH, 1, 1)]
    nodes0, idx0, info0, frame0 = g.bvh()[0].copy(), g.bvh()[1].copy(), g.info, frames(rt, g, spec)
    with pytest.raises(rt.RTError) as e:
        g.rebuild()
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    assert g.bvh()[0].tobytes() == nodes0.tobytes() and np.array_equal(g.bvh()[1], idx0) and g.info == info0
    assert_frames_equal(frames(rt, g, spec), frame0)
    g.update_prims(1, prims[1:])                         # and the scene still updates, and then rebuilds
    g.rebuild()
    assert_tree_is_hosts(rt, g, prims)
    tp, tm, _ = cases["teapotF"]
    sb = rt.Scene(tp, tm, bvh_kind=rt.BVH_SBVH)
    with pytest.raises(rt.RTError) as e:
        sb.rebuild()
    assert e.value.code == rt.RT_ERR_UNSUPPORTED


def test_full_size_mig16(rt, torch):
    """mig29 x16, 104,737 primitives: the rebuilt tree is the host builder's, 206,091 nodes (and the
    unused node 1)"""
    prims, _ = rt.recipe_describe("mig16")
    g = rt.Scene.recipe("mig16")
    g.rebuild()
    print("mig16 rebuild stats", g.rebuild_stats())
    assert g.info["num_prims"] == 104737 and g.info["nodes_used"] - 1 == 206091
    assert_tree_is_hosts(rt, g, prims)
