"""BVH analysis on the GPU: Scene.BVHVisualization (k_bvh_visualize) and the RT_MODE_BVH_HEAT frame
(k_render_heat) against the numpy model of bvh_heat_util.py -- counts equal, RGB8 and accumulator bits
equal --, and Scene.bvh_cost (rt_cost.hip) against rt_bvh_cost_host and numpy on live scenes.
Frames are 36 x 20: a 5 x 3 tile grid with a partial tile on both edges."""
import ctypes as C

import numpy as np
import pytest

from bvh_heat_util import (BATCHES, H, TWIST, W, assert_cost_close, heat_frames, np_cost, np_visualize, probe_rays,
                           tree_cases)
from refit_util import triangle_ids, twist, verts_of, with_verts
from scenes_util import kat_rays

pytestmark = pytest.mark.gpu

CASES = ("kat", "leaf", "chain", "teapotF", "sbvh", "room")
NPX = W * H


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cases(rt):
    return tree_cases(rt)


@pytest.fixture(scope="module")
def cam_rays(oracle, rt):
    """the camera rays of frames 0 and 1 (sample 0), the same for every scene: [2][W*H, 7]"""
    o = oracle.Scene("teapotF", rt.DATA_DIR)
    px = np.arange(NPX, dtype=np.int32)
    return o.camera_rays(W, H, px, frame=0), o.camera_rays(W, H, px, frame=1)


def make_scene(rt, case):
    prims, mats, bvh, kind = case
    return rt.Scene(prims, mats, bvh=bvh, bvh_kind=kind)


@pytest.mark.parametrize("name", CASES)
def test_visualization_equals_host_walk_and_model(rt, torch, cases, cam_rays, name):
    g = make_scene(rt, cases[name])
    nodes = g.bvh()[0]
    rays = probe_rays(nodes, cam_rays[0], kat_rays())
    want = np_visualize(nodes, rays[:max(BATCHES)])
    assert np.array_equal(rt.bvh_visualize_nodes(nodes, rays[:max(BATCHES)]), want)
    for n in BATCHES:
        got = g.BVHVisualization(rays[:n])
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, 2) and got.is_cuda
        got = got.cpu().numpy().view(np.uint32)
        bad = np.nonzero((got != want[:n]).any(axis=1))[0]
        assert len(bad) == 0, (name, n, rays[bad[:3]], got[bad[:3]], want[bad[:3]])
    assert np.array_equal(g.bvh_visualize_host(rays[:65]), want[:65])
    if name == "leaf":
        assert (want == 1).all()
    # n = 0 is RT_OK, with and without pointers
    assert tuple(g.BVHVisualization(np.zeros((0, 7), np.float32)).shape) == (0, 2)
    assert g.bvh_visualize_host(np.zeros((0, 7), np.float32)).shape == (0, 2)
    L = rt.lib()
    assert L.rt_bvh_visualize(g.h, None, None, 0, None) == rt.RT_OK
    assert L.rt_bvh_visualize(g.h, None, None, 4, None) == rt.RT_ERR_INVALID
    assert L.rt_bvh_visualize_host(g.h, None, None, 4) == rt.RT_ERR_INVALID
    g.close()


def heat_renderer(rt, g):
    r = rt.Renderer(g, W, H)
    r.mode = rt.MODE_BVH_HEAT
    return r


def assert_frame(name, rgb, acc, want):
    wacc, wrgb = want
    nb = int((np.ascontiguousarray(acc, np.float32).view(np.uint32) != wacc.view(np.uint32)).any(axis=1).sum())
    assert nb == 0, f"{name}: {nb} accumulator pixels differ in their bits"
    assert np.array_equal(np.asarray(rgb, np.uint32), wrgb), f"{name}: {int((rgb != wrgb).sum())} RGB8 pixels differ"


@pytest.mark.parametrize("name", ("teapotF", "room"))
def test_heat_frames(rt, torch, cases, cam_rays, name):
    g = make_scene(rt, cases[name])
    nodes, depth = g.bvh()[0], g.info["depth"]
    c0, c1 = np_visualize(nodes, cam_rays[0]), np_visualize(nodes, cam_rays[1])
    want = heat_frames(c0, c1, depth)
    if name == "teapotF":
        assert (c0[:, 1] > depth).any(), "red saturates on some pixels of this frame"
    r = heat_renderer(rt, g)
    assert r.kernel_name() == "k_render_heat"
    before = r.counters()
    # depth is ignored in this mode: any value gives the same frame
    rgb = r.tick_host(spp=1, depth=7, frame=0, reset=True)
    assert_frame("frame 0, reset", rgb, r.accumulator(), want["reset0"])
    rgb = r.tick_host(spp=1, depth=99, frame=1, reset=False)
    assert_frame("frame 1, running average", rgb, r.accumulator(), want["avg1"])
    rgb2 = r.tick_host(spp=2, frame=0, reset=True)
    assert_frame("spp 2", rgb2, r.accumulator(), want["spp2"])
    after = r.counters()
    assert after["primary"] - before["primary"] == NPX * (1 + 1 + 2)
    assert after["shadow"] == before["shadow"] and after["bounce"] == before["bounce"]
    assert after["frames"] - before["frames"] == 3
    # the device-output entry point
    out = r.Tick(spp=1, frame=0, reset=True)
    torch.cuda.synchronize()
    assert_frame("Tick", out.cpu().numpy().view(np.uint32), r.accumulator(), want["reset0"])
    full_rgb, full_acc = want["reset0"][1], want["reset0"][0]

    # three interleaved shards, then the assembly
    dev = f"cuda:{g.device}"
    cap = r.shard_capacity(3)
    gathered = torch.zeros(3 * cap, dtype=torch.int32, device=dev)
    for k in range(3):
        r.render_shard(gathered[k * cap:(k + 1) * cap], k, 3, spp=1, frame=0, reset=True)
    img = torch.zeros(NPX, dtype=torch.int32, device=dev)
    r.assemble(gathered, 3, img)
    torch.cuda.synchronize()
    assert_frame("3 shards", img.cpu().numpy().view(np.uint32), r.accumulator(), (full_acc, full_rgb))

    # an explicit deal over a shuffled tile list, two shards of unequal size
    ntiles = ((W + 7) // 8) * ((H + 7) // 8)
    tiles = np.random.default_rng(9).permutation(ntiles).astype(np.uint32)
    off = np.array([0, 6, ntiles], np.uint32)
    stride = 64 * ntiles
    gathered = torch.zeros(2 * stride, dtype=torch.int32, device=dev)
    r2 = heat_renderer(rt, g)
    for k in range(2):
        r2.render_shard_tiles(gathered[k * stride:(k + 1) * stride], tiles[off[k]:off[k + 1]], spp=1, frame=0, reset=True)
    img2 = torch.zeros(NPX, dtype=torch.int32, device=dev)
    r2.assemble_tiles(gathered, stride, tiles, off, img2)
    torch.cuda.synchronize()
    assert_frame("tile deal", img2.cpu().numpy().view(np.uint32), r2.accumulator(), (full_acc, full_rgb))
    assert r2.counters()["primary"] == NPX

    # superset invariant: the heat walk's visits, recovered from green, cover the closest-hit walk's
    p = rt.Renderer(g, W, H)
    _, pix = p.tile_work(spp=1, depth=1, frame=0, pixels=True)
    green = full_acc[:, 1].astype(np.float64)
    visits = np.rint(green * depth * 4.0).astype(np.int64)
    assert np.array_equal(visits, c0[:, 0].astype(np.int64))
    assert (visits >= pix[:, 0].astype(np.int64)).all()
    assert (visits > pix[:, 0].astype(np.int64)).any() or name == "room"
    for x in (p, r2, r):
        x.close()
    g.close()


def test_heat_frames_leave_the_timed_choices_alone(rt, torch, cases):
    g = make_scene(rt, cases["teapotF"])
    r = rt.Renderer(g, W, H)
    path0 = r.tick_host(spp=1, depth=1, frame=0, reset=True).copy()
    acc0 = r.accumulator().copy()
    state0 = (r.choices(), r.overlap(), r.overlap_depth(), r.tile_costs().tobytes())
    r.mode = rt.MODE_BVH_HEAT
    for f in range(4):
        r.tick_host(spp=1, frame=f, reset=f == 0)
    assert (r.choices(), r.overlap(), r.overlap_depth(), r.tile_costs().tobytes()) == state0
    r.mode = rt.MODE_PATH
    assert np.array_equal(r.tick_host(spp=1, depth=1, frame=0, reset=True), path0)
    assert r.accumulator().tobytes() == acc0.tobytes()
    r.close()
    g.close()


def test_live_scene_costs(rt, torch, cases, cam_rays):
    prims, mats, _, _ = cases["teapotF"]
    ids = triangle_ids(rt, prims)
    assert np.array_equal(ids, np.arange(ids[0], ids[0] + len(ids)))
    tw = twist(verts_of(prims, ids), TWIST)
    moved = with_verts(rt, prims, ids, tw)
    g = rt.Scene(prims, mats)
    rest = g.bvh_cost()
    assert_cost_close(rest, np_cost(g.bvh()[0]), g.info["nodes_used"])
    g.update_triangles(int(ids[0]), tw)
    nodes = g.bvh()[0]                                     # the refitted tree, downloaded
    rays = probe_rays(nodes, cam_rays[0], kat_rays())[:257]
    got = g.BVHVisualization(rays).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, np_visualize(nodes, rays))
    refit = g.bvh_cost()
    assert_cost_close(refit, rt.bvh_cost_host(nodes), len(nodes))
    assert_cost_close(refit, np_cost(nodes), len(nodes))
    assert_cost_close(refit, np_cost(rt.refit_bvh_host(moved, *rt.build_bvh_host(prims)[:2])), len(nodes))
    g.rebuild()
    rebuilt = g.bvh_cost()
    fresh = rt.Scene(moved, mats)
    assert fresh.info == g.info
    assert_cost_close(rebuilt, fresh.bvh_cost(), g.info["nodes_used"])
    assert_cost_close(rebuilt, rt.bvh_cost_host(rt.build_bvh_host(moved)[0]), g.info["nodes_used"])
    print(f"sah at rest {rest['sah']:.4f}, refitted {refit['sah']:.4f}, rebuilt {rebuilt['sah']:.4f}")
    assert rebuilt["sah"] < refit["sah"]
    first = int(ids[100])
    g.splice_triangles(first, 10, [])
    spliced = g.bvh_cost()
    assert spliced["refs"] == rebuilt["refs"] - 10 == g.info["num_refs"]
    assert_cost_close(spliced, rt.bvh_cost_host(g.bvh()[0]), g.info["nodes_used"])
    # the SBVH's leaves share primitives: refs counts references
    sb = make_scene(rt, cases["sbvh"])
    c = sb.bvh_cost()
    assert c["refs"] == sb.info["num_refs"] > sb.info["num_prims"]
    assert_cost_close(c, np_cost(sb.bvh()[0]), sb.info["nodes_used"])
    # the room's plane boxes: finite in double
    room = make_scene(rt, cases["room"])
    c = room.bvh_cost()
    assert np.isfinite(c["sah"]) and c["root_area"] > 1e60
    assert_cost_close(c, np_cost(room.bvh()[0]), room.info["nodes_used"])
    for s in (g, fresh, sb, room):
        s.close()


def test_refusals(rt, torch, cases):
    g = make_scene(rt, cases["kat"])
    r = rt.Renderer(g, W, H)
    r.mode = 4
    with pytest.raises(rt.RTError) as e:
        r.tick_host(spp=1, depth=1, frame=0, reset=True)
    assert e.value.code == rt.RT_ERR_INVALID
    # the work map stays RT_MODE_PATH only, rt_trace PATH / WHITTED only
    r.mode = rt.MODE_BVH_HEAT
    with pytest.raises(rt.RTError) as e:
        r.tile_work(spp=1, depth=1, frame=0)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    with pytest.raises(rt.RTError) as e:
        g.trace(kat_rays()[:4], np.arange(1, 5, dtype=np.uint32), depth=1, mode=rt.MODE_BVH_HEAT)
    assert e.value.code == rt.RT_ERR_INVALID
    L = rt.lib()
    c = rt.BvhCost()
    assert L.rt_scene_bvh_cost(None, C.byref(c), None) == rt.RT_ERR_INVALID
    assert L.rt_scene_bvh_cost(g.h, None, None) == rt.RT_ERR_INVALID
    r.close()
    g.close()
    # a primitive box that is not finite: no cost, and the record stays as it was
    prims, mats, _, _ = cases["kat"]
    bad = list(prims) + [rt.sphere((0, 0, 5), float("inf"), 1)]
    s = rt.Scene(bad, mats)
    c = rt.BvhCost()
    c.sah, c.refs = -7.0, 12345
    assert L.rt_scene_bvh_cost(s.h, C.byref(c), None) == rt.RT_ERR_UNSUPPORTED
    assert c.sah == -7.0 and c.refs == 12345 and c.leaf_cost == 0.0
    s.close()
