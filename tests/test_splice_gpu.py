"""Scene.splice_triangles on the GPU: triangles leave and enter a live scene, and afterwards the scene
is indistinguishable from one created fresh from the spliced list -- the host builder's node and index
bytes, info, hit ids and t / u / v bits, occlusion, RGB8 frames and accumulator bits in every mode, the
wave walk's counters -- while renderers created before the splice stay valid, the new ids are what the
in-place updates address, and every refusal leaves the scene as it was.  Frames are 64 x 64."""
import numpy as np
import pytest

from anim_util import room_mats, room_prims, with_prims
from refit_util import twist, verts_of, with_verts
from test_rebuild_gpu import (H, W, all_specs, assert_same_as_twin, assert_tree_is_hosts, frames, soup, soup_mats,
                              walk_frame)
from test_refit_gpu import assert_frames_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def triangles(rt, n, seed, lo, hi, mat):
    """n small random triangles with centres in [lo, hi)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(lo, hi, (n, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-0.15, 0.15, (n, 3, 3)).astype(np.float32)).astype(np.float32)
    return [rt.triangle(t[0], t[1], t[2], mat) for t in v]


def spliced(prims, first, remove, new):
    out = list(prims)
    out[first:first + remove] = list(new)
    return out


def apply(prims, edits):
    for first, remove, new in edits:
        prims = spliced(prims, first, remove, new)
    return prims


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (primitives, materials, [(first, remove, inserted records)]), the edits of
    tests/cpp/splice_host.cpp"""
    box = ((-5, -2, 2), (5, 2, 8))
    tp, tm = rt.recipe_describe("teapotF")
    assert len(tp) == 1027 and tp[0].type != rt.TRIANGLE
    tv = verts_of(tp, range(1, len(tp))).reshape(-1, 3)
    tbox = (tv.min(axis=0), tv.max(axis=0))
    into, more = triangles(rt, 300, 45, *tbox, 1), triangles(rt, 37, 46, *tbox, 1)
    room = room_prims(rt, 0.0)
    return {
        # the root crosses kBuildWide = 64: from the one-workgroup path to the many-workgroup path
        "soup60+10": (soup(rt, 60, 41), soup_mats(rt), [(60, 0, triangles(rt, 10, 42, *box, 1))]),
        # both edits cross kBuildChunk = 256
        "soup300-50+50": (soup(rt, 300, 43), soup_mats(rt), [(120, 50, []), (1, 0, triangles(rt, 50, 44, *box, 1))]),
        # remove and insert in one call (the new triangles enter where the range left), then an append
        "teapot_one_call": (tp, tm, [(100, 300, into), (1027, 0, more)]),
        # ... and with the new triangles at 1: ids 1 .. 99 shift to 301 .. 399
        "teapot_two_calls": (tp, tm, [(100, 300, []), (1, 0, into), (1027, 0, more)]),
        # the spheres', the cube's and the planes' ids shift by 5
        "room+5": (room, room_mats(rt), [(1, 0, triangles(rt, 5, 47, (-1.0, -0.8, 1.0), (1.0, 1.0, 3.0), 3))]),
    }


def device_records(rt, torch, g, prims):
    rec, _ = rt.pack_prims(prims)
    return torch.from_numpy(rec).to(f"cuda:{g.device}")


def splice_all(rt, g, edits, torch=None):
    """the edits one after the other; torch: pass the records as device tensors"""
    for first, remove, new in edits:
        g.splice_triangles(first, remove, device_records(rt, torch, g, new) if torch is not None and new else new)


def tick(r):
    return r.tick_host(spp=1, depth=1, frame=0, reset=True).copy()


@pytest.mark.parametrize("name", ["soup60+10", "soup300-50+50", "teapot_one_call", "teapot_two_calls", "room+5"])
def test_spliced_scene_equals_a_fresh_one(rt, oracle, torch, cases, name):
    prims, mats, edits = cases[name]
    final = apply(prims, edits)
    twin = rt.Scene(final, mats)
    t = rt.Renderer(twin, W, H)
    want, want_acc = tick(t), t.accumulator().copy()
    t.close()
    for device in (False, True):                          # the records as a host list, as a device tensor
        g = rt.Scene(prims, mats)
        r = rt.Renderer(g, W, H)
        tick(r)                                           # a renderer has run on the old scene
        splice_all(rt, g, edits, torch if device else None)
        assert_tree_is_hosts(rt, g, final)
        assert g.info == twin.info and g.info["num_prims"] == len(final)
        print(name, "device" if device else "host", g.info, "stats", g.rebuild_stats())
        assert np.array_equal(tick(r), want), "the renderer created before the splice"
        assert r.accumulator().tobytes() == want_acc.tobytes()
        r.close()
        if not device:
            assert_same_as_twin(rt, oracle, g, twin, final, mats, all_specs(rt))
        g.close()


def test_prebuilt_tree_gets_the_builders(rt, torch):
    """a scene created over a caller's one-leaf tree has the builder's tree from the first splice on"""
    from refit_util import scene_cases
    prims, mats, bvh = scene_cases(rt)["leaf"]
    g = rt.Scene(prims, mats, bvh=bvh)
    assert g.info["nodes_used"] == 2
    new = [rt.triangle((2.0, -0.5, 3.0), (3.0, -0.5, 3.0), (2.5, 1.0, 3.5), 1)]
    g.splice_triangles(3, 0, new)
    assert_tree_is_hosts(rt, g, prims + new)
    assert g.info == rt.Scene(prims + new, mats).info and g.info["nodes_used"] > 2


def test_the_new_id_space_is_live(rt, torch, cases):
    """in-place updates address the new ids; a rebuild and an undoing splice follow"""
    prims, mats, edits = cases["teapot_two_calls"]
    final = apply(prims, edits)
    spec = [(rt.MODE_PATH, 1, 1), (rt.MODE_PATH, 4, 2)]
    g, twin = rt.Scene(prims, mats), rt.Scene(final, mats)
    splice_all(rt, g, edits)

    def same_as_twin_and_fresh(now):
        """the twin -- a fresh scene of the spliced list given the same update -- in tree bytes and
        frames; and a scene created fresh from the moved primitives in its depth-1 frame"""
        assert g.bvh()[0].tobytes() == twin.bvh()[0].tobytes() and np.array_equal(g.bvh()[1], twin.bvh()[1])
        assert_frames_equal(frames(rt, g, spec), frames(rt, twin, spec))
        assert_frames_equal(frames(rt, g, spec[:1]), frames(rt, rt.Scene(now, mats), spec[:1]))

    # the inserted range, ids 1 .. 300
    ids = np.arange(1, 301)
    now = with_verts(rt, final, ids, twist(verts_of(final, ids), 0.5))
    for s in (g, twin):
        s.update_triangles(1, verts_of(now, ids))
    same_as_twin_and_fresh(now)
    # old triangles 1 .. 99, now 301 .. 399, one unit up by matrix
    ids = np.arange(301, 400)
    assert verts_of(final, ids).tobytes() == verts_of(prims, ids - 300).tobytes()
    M = rt.mat4_translate(0.0, 1.0, 0.0)
    rest = verts_of(now, ids)
    for s in (g, twin):
        s.transform_triangles([(301, 99, M)], rest)
    moved = (rest.reshape(-1, 3) + np.array([0.0, 1.0, 0.0], np.float32)).astype(np.float32).reshape(-1, 9)
    now = with_verts(rt, now, ids, moved)
    same_as_twin_and_fresh(now)
    g.rebuild()
    assert_tree_is_hosts(rt, g, now)
    # undo: every triangle back where it was, the inserted ones out, the removed ones in again
    all_ids = np.arange(1, len(now))
    g.update_triangles(1, verts_of(final, all_ids))
    g.splice_triangles(1027, 37, [])
    g.splice_triangles(1, 300, [])
    g.splice_triangles(100, 0, prims[100:400])
    first = rt.Scene(prims, mats)
    assert g.info == first.info
    assert g.bvh()[0].tobytes() == first.bvh()[0].tobytes() and np.array_equal(g.bvh()[1], first.bvh()[1])
    assert_frames_equal(frames(rt, g, spec), frames(rt, first, spec))


def test_shifted_cube_moves(rt, torch, cases):
    """the room's cube, id 3 before the splice and 8 after it, at a second pose through update_prims"""
    prims, mats, edits = cases["room+5"]
    final = apply(prims, edits)
    assert final[8].type == rt.CUBE
    pose = with_prims(final, 8, [room_prims(rt, 1.3)[3]])
    g, twin = rt.Scene(prims, mats), rt.Scene(final, mats)
    splice_all(rt, g, edits)
    for s in (g, twin):
        s.update_prims(8, [pose[8]])
    assert g.bvh()[0].tobytes() == twin.bvh()[0].tobytes() and np.array_equal(g.bvh()[1], twin.bvh()[1])
    specs = all_specs(rt)
    assert_frames_equal(frames(rt, g, specs), frames(rt, twin, specs))
    assert_frames_equal(frames(rt, g, specs[:1]), frames(rt, rt.Scene(pose, mats), specs[:1]))
    g.rebuild()
    assert_tree_is_hosts(rt, g, pose)


def test_wave_walk_on_the_spliced_teapot(rt, torch, cases):
    prims, mats, edits = cases["teapot_two_calls"]
    g, twin = rt.Scene(prims, mats), rt.Scene(apply(prims, edits), mats)
    splice_all(rt, g, edits)
    a, b = walk_frame(rt, g), walk_frame(rt, twin)
    print("walk stats (spliced, fresh):", a[2], b[2])
    assert a[2] == b[2] and a[2]["walked"] > 0 and a[2]["verify_mismatch"] == 0
    assert_frames_equal([a[:2]], [b[:2]])


def test_refusals_leave_the_scene_untouched(rt, torch, cases):
    prims, mats, _ = cases["room+5"]
    g = rt.Scene(prims, mats)
    spec = [(rt.MODE_PATH, 1, 1)]
    nodes0, idx0, info0, frame0, stats0 = g.bvh()[0].copy(), g.bvh()[1].copy(), g.info, frames(rt, g, spec), g.rebuild_stats()
    ok = rt.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), 1)
    nan = rt.triangle((0, 0, 2), (1, float("nan"), 2), (0, 1, 2), 1)

    def refused(first, remove, new, code, device=False):
        with pytest.raises(rt.RTError) as e:
            g.splice_triangles(first, remove, device_records(rt, torch, g, new) if device else new)
        assert e.value.code == code, e.value
        assert g.info == info0 and g.bvh()[0].tobytes() == nodes0.tobytes() and np.array_equal(g.bvh()[1], idx0)
        assert_frames_equal(frames(rt, g, spec), frame0)

    for device in (False, True):
        refused(10, 0, [ok, rt.sphere((0, 0, 2), 0.5, 1)], rt.RT_ERR_INVALID, device)      # a record of another type
        refused(10, 0, [rt.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), 4), ok], rt.RT_ERR_INVALID, device)   # material 4 of 4
        refused(10, 1, [ok, nan], rt.RT_ERR_INVALID, device)                               # a NaN vertex
    refused(3, 1, [], rt.RT_ERR_INVALID)                  # the removed range holds the cube
    refused(0, 0, [ok], rt.RT_ERR_INVALID)                # the light stays
    refused(11, 2, [], rt.RT_ERR_INVALID)                 # past the end
    refused(13, 0, [ok], rt.RT_ERR_INVALID)               # first > num_prims
    refused(10, 0, [ok] * 300, rt.RT_ERR_UNSUPPORTED)     # one leaf of 300
    g.splice_triangles(5, 0, [])                          # an empty edit does nothing
    assert g.rebuild_stats() == stats0 and g.info == info0
    g.splice_triangles(10, 2, [ok])                       # and the scene still splices
    assert_tree_is_hosts(rt, g, spliced(prims, 10, 2, [ok]))
    tp, tm, _ = cases["teapot_one_call"]
    sb = rt.Scene(tp, tm, bvh_kind=rt.BVH_SBVH)
    with pytest.raises(rt.RTError) as e:
        sb.splice_triangles(100, 10, [])
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
