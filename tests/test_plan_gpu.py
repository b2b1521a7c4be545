"""The refit schedule built on the GPU (csrc/rt_plan.h, rt_plan.hip): after Scene.prepare_updates --
on a fresh scene, after a rebuild, after a splice -- the device's list / lvl / grp equal
rt.refit_plan_host of the scene's tree word for word, by the route the tree's size implies; a second
call launches nothing; an update after the call leaves the scene of a twin updated without it; a
rebuild's stats stay the rebuild's; an SBVH scene is refused as an update refuses it.  Frames are 64 x 64."""
import numpy as np
import pytest

from refit_util import scene_cases, triangle_ids, twist, verts_of, with_verts
from test_rebuild_gpu import BUILD_WIDE, frames, soup, soup_mats
from test_refit_gpu import assert_frames_equal, random_rays, update

pytestmark = pytest.mark.gpu

CASES = ["leaf", "kat", "chain", "teapotF", "soup259", "soup20000"]


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cases(rt):
    c = scene_cases(rt)
    c["soup259"] = (soup(rt, 4 * BUILD_WIDE + 3, 5), soup_mats(rt), None)
    c["soup20000"] = (soup(rt, 20001, 6), soup_mats(rt), None)
    return c


def assert_plan_is_hosts(rt, g, what):
    info = g.update_plan_info()
    want = rt.refit_plan_host(*g.bvh())
    got = g.update_plan()
    route = "gpu_one_workgroup" if g.info["nodes_used"] <= rt.PLAN_SMALL_NODES else "gpu_launches"
    assert info["ready"] and info["route"] == route, (what, info)
    assert info["launches"] == (1 if route == "gpu_one_workgroup" else 3 * min(g.info["depth"], 64) + 7), (what, info)
    assert got["ntreelets"] == want["ntreelets"] and got["has_top"] == want["has_top"], what
    for name in ("list", "lvl", "grp"):
        assert np.array_equal(got[name], want[name]), f"{what}: {name} differs from the host's"
    assert info["top_nodes"] == len(want["list"]) - want["lvl"][want["grp"][want["ntreelets"]]], what
    return info


@pytest.mark.parametrize("name", CASES)
def test_prepared_schedule_is_the_hosts(rt, torch, cases, name):
    prims, mats, bvh = cases[name]
    g = rt.Scene(prims, mats, bvh=bvh)
    assert not g.update_plan_info()["ready"]
    with pytest.raises(rt.RTError) as e:
        g.update_plan()
    assert e.value.code == rt.RT_ERR_INVALID
    assert g.prepare_updates() > 0
    info = assert_plan_is_hosts(rt, g, "fresh")
    print(name, "fresh", info)
    assert g.prepare_updates() == 0 and g.update_plan_info()["launches"] == 0     # nothing to do
    assert g.update_plan_info()["ready"]
    g.rebuild()
    assert not g.update_plan_info()["ready"]                 # the old topology's schedule went with it
    stats = g.rebuild_stats()
    assert g.prepare_updates() > 0
    assert g.rebuild_stats() == stats
    print(name, "rebuilt", assert_plan_is_hosts(rt, g, "rebuilt"))
    if name in ("leaf", "chain"):
        return
    first = int(triangle_ids(rt, prims)[0])
    new = [rt.triangle((2.0, -0.5, 3.0), (3.0, -0.5, 3.0), (2.5, 1.0, 3.5), 1),
           rt.triangle((-2.0, 0.5, 4.0), (-3.0, 0.5, 4.0), (-2.5, 1.5, 4.5), 1)]
    g.splice_triangles(first, 1, new)
    assert not g.update_plan_info()["ready"]
    assert g.prepare_updates() > 0
    print(name, "spliced", assert_plan_is_hosts(rt, g, "spliced"))


@pytest.mark.parametrize("name", ["teapotF", "soup259"])
def test_update_after_prepare_equals_update_without(rt, torch, cases, name):
    prims, mats, bvh = cases[name]
    ids = triangle_ids(rt, prims)
    moved = with_verts(rt, prims, ids, twist(verts_of(prims, ids), 1.0))
    g, twin = rt.Scene(prims, mats, bvh=bvh), rt.Scene(prims, mats, bvh=bvh)
    g.prepare_updates()
    update(g, moved, ids)
    update(twin, moved, ids)
    # the twin's first update built its schedule itself, on the GPU too
    ti, gi = twin.update_plan_info(), g.update_plan_info()
    assert ti["ready"] and ti["route"] == "gpu_one_workgroup" and ti["launches"] == 1, ti
    assert gi["route"] == ti["route"]
    for k in ("list", "lvl", "grp"):
        assert np.array_equal(g.update_plan()[k], twin.update_plan()[k])
    assert g.bvh()[0].tobytes() == twin.bvh()[0].tobytes(), "node bytes differ from the twin's"
    rays = random_rays(4096, 11)
    assert g.intersect_host(rays).tobytes() == twin.intersect_host(rays).tobytes()
    spec = [(rt.MODE_PATH, 1, 1)]
    assert_frames_equal(frames(rt, g, spec), frames(rt, twin, spec))


def test_sbvh_scene_is_refused(rt, torch, cases):
    prims, mats, _ = cases["teapotF"]
    sb = rt.Scene(prims, mats, bvh_kind=rt.BVH_SBVH)
    with pytest.raises(rt.RTError) as e:
        sb.prepare_updates()
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    assert not sb.update_plan_info()["ready"] and sb.update_plan_info()["route"] == "none"
