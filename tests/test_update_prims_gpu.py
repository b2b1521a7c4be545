"""Scene.update_prims on the GPU: primitives of every kind updated in place, then the BVH refit.

The contract is update_triangles': afterwards the scene is bit for bit a fresh scene of the new
description over the same tree topology.  So an updated scene must equal the oracle holding the same
primitives over the host-refitted tree -- hit ids, t / u / v bits, occlusion, RGB8 frames and
accumulator bits, no tie allowance -- and its node array the host refit's byte for byte.  Scenes: the
reference's animated room (SetTime's swinging quad light, bouncing sphere and spinning cube, plus two
triangles) under the builder's tree and under one that keeps the planes apart; the KAT scene with its
sphere light moved and resized; a tree whose root is a leaf; TEAPOT-F with a sphere, a cube and a
quad appended (non-triangles among many treelets and nodes above the cut)."""
import numpy as np
import pytest

from anim_util import MOVERS, TIMES, room_mats, room_prims, split_tree, with_prims
from refit_util import scene_cases, tree_of
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
    """(mode, depth, spp): primary + shadow, Whitted depth 4, path depth 4 x 2 spp"""
    return [(rt.MODE_PATH, 1, 1), (rt.MODE_WHITTED, 4, 1), (rt.MODE_PATH, 4, 2)]


def room_at(rt, base, t):
    """the t = 0 room with the three movers at SetTime(t)"""
    pose, out = room_prims(rt, t), base
    for i in MOVERS:
        out = with_prims(out, i, [pose[i]])
    return out


def device_prims(rt, torch, g, prims):
    rec, T = rt.pack_prims(prims)
    dev = f"cuda:{g.device}"
    return torch.from_numpy(rec).to(dev), torch.from_numpy(T).to(dev)


def assert_equals_oracle(rt, oracle, g, prims, mats, nodes, idx, specs, rays=True):
    host = rt.refit_bvh_host(prims, nodes, idx)
    assert g.bvh()[0].tobytes() == host.tobytes()
    assert np.array_equal(g.bvh()[1], idx)
    o = oracle_scene(rt, oracle, prims, mats, bvh=(host, idx))
    if rays:
        assert_rays_equal(g, o)
    assert_frames_equal(gpu_frames(rt, g, specs), oracle_frames(o, specs))
    return host


@pytest.mark.parametrize("tree", ["built", "split"])
def test_room_follows_set_time(rt, oracle, torch, specs, tree):
    base, mats = room_prims(rt, 0.0), room_mats(rt)
    nodes, idx = rt.build_bvh_host(base)[:2] if tree == "built" else split_tree(rt, base)
    g = rt.Scene(base, mats, bvh=(nodes, idx))
    rs = [rt.Renderer(g, W, H) for _ in specs]
    frames0 = gpu_frames(rt, g, specs, rs)               # the renderers have run before the updates
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    seen = set()
    for k, t in enumerate(TIMES[1:]):
        new = room_at(rt, base, t)
        if k % 2 == 0:                                   # one call per mover, host records
            for i in MOVERS:
                g.update_prims(i, [new[i]])
        else:                                            # one range over all of them, device tensors
            g.update_prims(0, device_prims(rt, torch, g, new[0:4]))
        seen.add(assert_equals_oracle(rt, oracle, g, new, mats, nodes, idx, specs).tobytes())
    if tree == "split":
        assert len(seen) == len(TIMES) - 1 and nodes.tobytes() not in seen
    g.update_prims(0, base[0:4])                         # back to t = 0: the creation-time bytes and frames
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    assert_frames_equal(gpu_frames(rt, g, specs, rs), frames0)
    assert_equals_oracle(rt, oracle, g, base, mats, nodes, idx, specs[:1])
    for r in rs:
        r.close()


def test_kat_sphere_light_moves_and_resizes(rt, oracle, specs):
    """depth-1 frames pin next-event estimation on the moved light, and the shadow-ray counts"""
    prims, mats, bvh = scene_cases(rt)["kat"]
    nodes, idx = tree_of(rt, prims, bvh)
    g, r = rt.Scene(prims, mats), None
    new = with_prims(prims, 0, [rt.sphere((1.5, 3.0, 1.0), 0.8, 0)])
    g.update_prims(0, [new[0]])
    host = assert_equals_oracle(rt, oracle, g, new, mats, nodes, idx, specs)
    fresh = rt.Scene(new, mats, bvh=(host, idx))
    counts = []
    for s in (g, fresh):
        r = rt.Renderer(s, W, H)
        rgb = r.tick_host(spp=1, depth=1, frame=0, reset=True)
        counts.append((r.counters(), rgb, r.accumulator()))
        r.close()
    assert counts[0][0] == counts[1][0] and counts[0][0]["shadow"] > 0
    assert_frames_equal([counts[0][1:]], [counts[1][1:]])
    before = rt.Scene(prims, mats)
    assert not np.array_equal(gpu_frames(rt, before, specs[:1])[0][0], counts[0][1])   # the light did move


def test_root_leaf(rt, oracle, specs):
    prims, mats, bvh = scene_cases(rt)["leaf"]
    nodes, idx = tree_of(rt, prims, bvh)
    g = rt.Scene(prims, mats, bvh=bvh)
    new = [rt.sphere((0.5, 3.5, -1.0), 0.75, 0), prims[1],
           rt.triangle((-1.5, -1.0, 4.0), (0.5, 1.9, 4.2), (1.7, -1.0, 4.0), 1)]
    g.update_prims(0, new)
    assert_equals_oracle(rt, oracle, g, new, mats, nodes, idx, specs)


@pytest.fixture(scope="module")
def teapot_plus(rt):
    """TEAPOT-F with a sphere, a cube (pos != 0) and a quad appended, and their second pose"""
    prims, mats = rt.recipe_describe("teapotF")
    n = len(prims)
    a = [rt.sphere((-2.0, 0.2, 3.0), 0.4, 1), rt.cube((1.9, -0.6, 1.5), (0.5, 0.7, 0.4), 1, rt.mat4_rotate(1, 0.3)),
         rt.quad(0.9, 2, rt.mat4_mul(rt.mat4_translate(0.2, 1.9, 2.2), rt.mat4_rotate(0, 0.2)))]
    b = [rt.sphere((-1.6, 0.6, 2.6), 0.3, 1), rt.cube((1.7, -0.3, 1.9), (0.6, 0.5, 0.4), 1, rt.mat4_rotate(2, -0.5)),
         rt.quad(1.2, 2, rt.mat4_mul(rt.mat4_translate(-0.3, 1.7, 2.5), rt.mat4_rotate(2, 0.4)))]
    nodes, idx, _ = rt.build_bvh_host(prims + a)
    return prims + a, prims + b, mats, n, nodes, idx


def test_non_triangles_in_a_large_tree(rt, oracle, torch, specs, teapot_plus):
    first, second, mats, n, nodes, idx = teapot_plus
    g, twin = rt.Scene(first, mats), rt.Scene(first, mats)
    g.update_prims(n, second[n:])                                        # host records
    twin.update_prims(n, device_prims(rt, torch, twin, second[n:]))      # device tensors: identical bytes
    host = assert_equals_oracle(rt, oracle, g, second, mats, nodes, idx, specs)
    assert host.tobytes() != nodes.tobytes() and twin.bvh()[0].tobytes() == host.tobytes()
    assert_frames_equal(gpu_frames(rt, twin, specs), gpu_frames(rt, g, specs))
    # a mixed range over the tail: the last two triangles re-sent unchanged, the sphere back to its
    # first pose, the cube and the quad staying at their second
    mixed = second[:n] + [first[n]] + second[n + 1:]
    g.update_prims(n - 2, mixed[n - 2:n + 2])
    assert_equals_oracle(rt, oracle, g, mixed, mats, nodes, idx, specs[:1])


def test_mixed_range_resends_an_unmoved_primitive(rt, oracle, specs):
    """range [0, 4) of the room: the corner sphere (2) goes along unchanged"""
    base, mats = room_prims(rt, 0.0), room_mats(rt)
    nodes, idx = split_tree(rt, base)
    g = rt.Scene(base, mats, bvh=(nodes, idx))
    new = room_at(rt, base, 1.3)
    assert bytes(new[2]) == bytes(base[2])
    g.update_prims(0, new[0:4])
    assert_equals_oracle(rt, oracle, g, new, mats, nodes, idx, specs[:1], rays=False)
    twin = rt.Scene(base, mats, bvh=(nodes, idx))
    for i in MOVERS:
        twin.update_prims(i, [new[i]])
    assert_frames_equal(gpu_frames(rt, twin, specs), gpu_frames(rt, g, specs))


def test_errors_leave_the_scene_untouched(rt, torch, specs, teapot_plus):
    first, second, mats, n, nodes, idx = teapot_plus
    g = rt.Scene(first, mats)
    spec = specs[:1]
    frame0 = gpu_frames(rt, g, spec)

    def refused(start, prims, code=rt.RT_ERR_INVALID, device=False):
        with pytest.raises(rt.RTError) as e:
            g.update_prims(start, device_prims(rt, torch, g, prims) if device else prims)
        assert e.value.code == code

    good = second[n:]
    for dev in (False, True):
        refused(n, [rt.cube((0, 0, 0), 1.0, 1)] + good[1:], device=dev)                  # a wrong type
        refused(n, [rt.sphere((-1.6, 0.6, 2.6), 0.3, 2)] + good[1:], device=dev)         # a wrong material
        refused(n, good[:2] + [rt.quad(float("nan"), 2, good[2].T)], device=dev)         # a NaN field
        bad = np.array(good[1].T, np.float32)
        bad[7] = np.inf
        refused(n, [good[0], rt.cube((1.7, -0.3, 1.9), (0.6, 0.5, 0.4), 1, bad)], device=dev)   # a matrix
        refused(n, [rt.sphere((3e38, 0, 0), 3e38, 1)], device=dev)                       # finite fields, infinite box
        v = [float(x) for x in first[5].v]
        refused(5, [rt.triangle(v[0:3], (v[3], np.nan, v[5]), v[6:9], first[5].material)], device=dev)
    refused(n + 2, good)                                                                 # past the end
    g.update_prims(n, [])                                                                # count 0: a no-op
    # a sphere reads v[0..3] only: garbage beyond them is not its business
    odd = rt.sphere((-2.0, 0.2, 3.0), 0.4, 1)
    odd.v[8] = float("nan")
    g.update_prims(n, [odd])
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    assert_frames_equal(gpu_frames(rt, g, spec), frame0)
    sb = rt.Scene(first, mats, bvh_kind=rt.BVH_SBVH)
    assert sb.info["num_refs"] != sb.info["num_prims"]
    with pytest.raises(rt.RTError) as e:
        sb.update_prims(n, good)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
