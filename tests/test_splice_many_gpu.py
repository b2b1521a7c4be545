"""Scene.splice_ranges and Scene.compact_triangles on the GPU: several edits, or a keep-mask, in one
rebuild.  Afterwards the scene is indistinguishable from one created fresh from the edited list -- the
host builder's node and index bytes, info, the RGB8 frame and accumulator bits of a renderer created
BEFORE the edit, and once per case hits, occlusion and frames in every mode -- the two routes agree
with each other and with splice_triangles, the new ids are what the in-place updates address, and every
refusal leaves the scene as it was.  Frames are 64 x 64.

Sizes.  The ranges route uploads its table of edits whole: there is no staging chunk, and the case of
280 edits has more rows than a workgroup has lanes.  The mask route's prefix count takes 256 ids per
workgroup (kMaskGroup of csrc/rt_splice.h) and one workgroup folds the workgroups' counts 256 at a time
with a running carry, so it has no capacity; 256 x 256 + 1 primitives is where that fold takes a second
pass, and TEAPOT-F's 1,027 are five workgroups with the last one partial."""
import numpy as np
import pytest

from anim_util import room_mats, room_prims
from refit_util import twist, verts_of, with_verts
from test_rebuild_gpu import H, W, all_specs, assert_same_as_twin, assert_tree_is_hosts, frames, soup, soup_mats
from test_refit_gpu import assert_frames_equal
from test_splice_gpu import spliced, triangles

pytestmark = pytest.mark.gpu

MASK_GROUP = 256      # kMaskGroup of csrc/rt_splice.h
BOX = ((-5, -2, 2), (5, 2, 8))


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def edited(prims, edits):
    """the edits, all in ids of `prims`, one at a time in descending order of first"""
    for first, remove, new in sorted(edits, key=lambda e: -e[0]):
        prims = spliced(prims, first, remove, new)
    return prims


def kept(prims, keep):
    return [p for p, k in zip(prims, keep) if k]


def as_device(rt, torch, g, edits):
    """the same edits with every record in ONE device tensor, in the caller's order"""
    recs = [p for _, _, new in edits for p in new]
    rec = torch.from_numpy(rt.pack_prims(recs)[0]).to(f"cuda:{g.device}") if recs else None
    return [(f, n, rec, len(new)) for f, n, new in edits]


def tick(r):
    return r.tick_host(spp=1, depth=1, frame=0, reset=True).copy()


def tree_bytes(g):
    return g.bvh()[0].tobytes(), g.bvh()[1].tobytes()


def check_edit(rt, oracle, prims, mats, final, do_edit, full=True):
    """do_edit(scene) on a scene of prims with a renderer that has run; compared with a fresh twin of final"""
    twin = rt.Scene(final, mats)
    t = rt.Renderer(twin, W, H)
    want, want_acc = tick(t), t.accumulator().copy()
    t.close()
    g = rt.Scene(prims, mats)
    r = rt.Renderer(g, W, H)
    tick(r)                                               # a renderer has run on the old scene
    do_edit(g)
    assert_tree_is_hosts(rt, g, final)
    assert g.info == twin.info and g.info["num_prims"] == len(final)
    assert not g.update_plan_info()["ready"]              # the next update rebuilds its schedule
    assert np.array_equal(tick(r), want), "the renderer created before the edit"
    assert r.accumulator().tobytes() == want_acc.tobytes()
    r.close()
    if full:
        assert_same_as_twin(rt, oracle, g, twin, final, mats, all_specs(rt))
    twin.close()
    return g


@pytest.fixture(scope="module")
def range_cases(rt):
    """name -> (primitives, materials, [(first, remove, inserted records)] in ids of the old scene)"""
    t = lambda n, seed, mat=1: triangles(rt, n, seed, *BOX, mat)
    s300 = soup(rt, 300, 43)
    tp, tm = rt.recipe_describe("teapotF")
    assert len(tp) == 1027 and tp[0].type != rt.TRIANGLE
    tv = verts_of(tp, range(1, len(tp))).reshape(-1, 3)
    tbox = (tv.min(axis=0), tv.max(axis=0))
    room = room_prims(rt, 0.0)
    return {
        # the records in the caller's order, whichever way the edits are sorted
        "descending": (s300, soup_mats(rt), [(200, 10, t(7, 50)), (50, 4, t(3, 51))]),
        "ascending": (s300, soup_mats(rt), [(50, 4, t(3, 51)), (200, 10, t(7, 50))]),
        # the second range starts where the first ends and the first inserts nothing: two rows, one start
        "adjacent": (s300, soup_mats(rt), [(100, 5, []), (105, 5, t(3, 51)), (110, 0, t(7, 50))]),
        "append+removal": (s300, soup_mats(rt), [(300, 0, t(9, 52)), (7, 0, []), (10, 20, [])]),
        # around id 256, the workgroup boundary, in the old and in the new id space
        "across256": (s300, soup_mats(rt), [(250, 12, t(3, 51)), (240, 0, t(9, 52)), (2, 1, t(7, 50))]),
        # the fracture: every third triangle out, 100 rows for the binary search
        "every_third": (s300, soup_mats(rt), [(i, 1, []) for i in range(299, 1, -3)]),
        # no staging chunk to exceed: 280 rows, more than a workgroup has lanes; one in, one out
        "280_edits": (soup(rt, 600, 45), soup_mats(rt), [(2 * i + 1, i & 1, t(1 - (i & 1), 100 + i)) for i in range(280)]),
        # ids shift under the later edits
        "teapot": (tp, tm, [(700, 100, []), (1, 0, triangles(rt, 40, 54, *tbox, 1)), (300, 50, triangles(rt, 25, 55, *tbox, 1)),
                            (900, 127, []), (500, 1, [])]),
        # the spheres', the cube's and the planes' ids shift
        "room": (room, room_mats(rt), [(12, 0, triangles(rt, 2, 48, (-1.0, -0.8, 1.0), (1.0, 1.0, 3.0), 3)),
                                       (1, 0, triangles(rt, 5, 47, (-1.0, -0.8, 1.0), (1.0, 1.0, 3.0), 3)), (10, 1, [])]),
    }


def test_one_edit_is_the_single_splice(rt, oracle, torch):
    prims, mats, new = soup(rt, 60, 41), soup_mats(rt), triangles(rt, 10, 42, *BOX, 1)   # test_splice_gpu's soup60+10
    g = check_edit(rt, oracle, prims, mats, spliced(prims, 60, 0, new), lambda s: s.splice_ranges([(60, 0, new)]))
    one = rt.Scene(prims, mats)
    one.splice_triangles(60, 0, new)
    assert tree_bytes(g) == tree_bytes(one) and g.info == one.info
    assert_frames_equal(frames(rt, g, all_specs(rt)), frames(rt, one, all_specs(rt)))
    assert g.rebuild_stats()[3] == one.rebuild_stats()[3] + 1        # the source words' launch


@pytest.mark.parametrize("name", ["descending", "ascending", "adjacent", "append+removal", "across256", "every_third",
                                  "280_edits", "teapot", "room"])
def test_ranges_equal_a_fresh_scene(rt, oracle, torch, range_cases, name):
    prims, mats, edits = range_cases[name]
    final = edited(prims, edits)
    device = name in ("teapot", "280_edits")              # the records as one device tensor
    g = check_edit(rt, oracle, prims, mats, final, lambda s: s.splice_ranges(as_device(rt, torch, s, edits) if device else edits))
    print(name, g.info, "stats", g.rebuild_stats())
    if name == "descending":
        other = rt.Scene(prims, mats)
        other.splice_ranges(range_cases["ascending"][2])
        assert tree_bytes(g) == tree_bytes(other)
    if name == "room":
        assert final[8].type == rt.CUBE


def big_soup(rt):
    return soup(rt, MASK_GROUP * MASK_GROUP + 1, 7)


@pytest.fixture(scope="module")
def mask_cases(rt):
    """name -> (primitives, materials, keep flags)"""
    rng = np.random.default_rng(56)
    tp, tm = rt.recipe_describe("teapotF")
    s60, s300, big = soup(rt, 60, 41), soup(rt, 300, 43), big_soup(rt)
    drop1 = np.ones(60, np.uint8)
    drop1[37] = 0
    third = np.ones(300, np.uint8)
    third[np.arange(299, 1, -3)] = 0
    half = (rng.random(len(tp)) < 0.5).astype(np.uint8) * 3      # any value but 0 keeps
    half[0] = 1
    two = np.zeros(len(tp), np.uint8)
    two[[0, 513]] = 1
    sparse = np.ones(len(big), np.uint8)
    sparse[1 + rng.choice(len(big) - 1, 5000, replace=False)] = 0
    return {"drop1": (s60, soup_mats(rt), drop1), "every_third": (s300, soup_mats(rt), third), "teapot_half": (tp, tm, half),
            "light+1": (tp, tm, two), "65537": (big, soup_mats(rt), sparse)}


@pytest.mark.parametrize("name", ["drop1", "every_third", "teapot_half", "light+1", "65537"])
def test_mask_equals_a_fresh_scene(rt, oracle, torch, mask_cases, range_cases, name):
    prims, mats, keep = mask_cases[name]
    final = kept(prims, keep)
    device = name != "drop1"                              # the mask as a device tensor, once as a numpy array
    g = check_edit(rt, oracle, prims, mats, final,
                   lambda s: s.compact_triangles(torch.from_numpy(keep).to(f"cuda:{s.device}") if device else keep.astype(bool)),
                   full=name != "65537")
    print(name, g.info, "stats", g.rebuild_stats())
    if name == "every_third":                             # the ranges route's bytes for the same edit
        other = rt.Scene(prims, mats)
        other.splice_ranges(range_cases["every_third"][2])
        assert tree_bytes(g) == tree_bytes(other) and g.info == other.info
        assert_frames_equal(frames(rt, g, all_specs(rt)[:1]), frames(rt, other, all_specs(rt)[:1]))
    if name == "light+1":
        assert g.info["num_prims"] == 2


def test_a_mask_of_ones_does_nothing(rt, torch, mask_cases):
    prims, mats, _ = mask_cases["teapot_half"]
    g = rt.Scene(prims, mats)
    g.prepare_updates()
    plan, stats, nodes = g.update_plan_info(), g.rebuild_stats(), tree_bytes(g)
    assert plan["ready"]
    g.compact_triangles(torch.ones(len(prims), dtype=torch.uint8, device=f"cuda:{g.device}"))
    g.compact_triangles(np.ones(len(prims), bool))
    after = g.update_plan_info()
    assert after["ready"] and after == plan and g.rebuild_stats() == stats and tree_bytes(g) == nodes
    g.splice_ranges([(5, 0, []), (1027, 0, [])])          # nor do empty edits
    g.splice_ranges([])
    assert g.update_plan_info() == plan and g.rebuild_stats() == stats


def test_the_new_id_space_is_live(rt, oracle, torch, range_cases):
    """in-place updates address the new ids, a rebuild follows, then a second batched edit of each route"""
    prims, mats, edits = range_cases["teapot"]
    final = edited(prims, edits)
    spec = [(rt.MODE_PATH, 1, 1), (rt.MODE_PATH, 4, 2)]
    g, twin = rt.Scene(prims, mats), rt.Scene(final, mats)
    g.splice_ranges(edits)
    ids = np.arange(1, 41)                                # the records inserted at 1
    now = with_verts(rt, final, ids, twist(verts_of(final, ids), 0.5))
    for s in (g, twin):
        s.update_triangles(1, verts_of(now, ids))
    assert tree_bytes(g) == tree_bytes(twin)
    assert_frames_equal(frames(rt, g, spec), frames(rt, twin, spec))
    assert_frames_equal(frames(rt, g, spec[:1]), frames(rt, rt.Scene(now, mats), spec[:1]))
    g.rebuild()
    assert_tree_is_hosts(rt, g, now)
    # a second batched edit on the edited scene: the inserted records out again, others in at the end
    more = triangles(rt, 12, 58, (-1, 0, -1), (1, 1, 1), 1)
    edits2 = [(len(now), 0, more), (1, 40, [])]
    now2 = edited(now, edits2)
    g.splice_ranges(edits2)
    assert_tree_is_hosts(rt, g, now2)
    assert g.info == rt.Scene(now2, mats).info
    keep = np.ones(len(now2), np.uint8)
    keep[100:400:7] = 0
    now3 = kept(now2, keep)
    g.compact_triangles(torch.from_numpy(keep).to(f"cuda:{g.device}"))
    assert_tree_is_hosts(rt, g, now3)
    fresh = rt.Scene(now3, mats)
    assert g.info == fresh.info
    assert_frames_equal(frames(rt, g, spec), frames(rt, fresh, spec))


def test_refusals_leave_the_scene_untouched(rt, torch, range_cases):
    prims, mats, _ = range_cases["room"]
    g = rt.Scene(prims, mats)
    spec = [(rt.MODE_PATH, 1, 1)]
    nodes0, info0, frame0, stats0 = tree_bytes(g), g.info, frames(rt, g, spec), g.rebuild_stats()
    ok = rt.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), 1)
    nan = rt.triangle((0, 0, 2), (1, float("nan"), 2), (0, 1, 2), 1)
    bad = rt.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), 4)                # material 4 of 4

    def refused(call, code):
        with pytest.raises(rt.RTError) as e:
            call()
        assert e.value.code == code, e.value
        assert g.info == info0 and tree_bytes(g) == nodes0 and g.rebuild_stats() == stats0
        assert_frames_equal(frames(rt, g, spec), frame0)

    for device in (False, True):
        form = (lambda e: as_device(rt, torch, g, e)) if device else (lambda e: e)
        refused(lambda: g.splice_ranges(form([(10, 1, [ok]), (12, 0, [ok, nan])])), rt.RT_ERR_INVALID)   # NaN in the last record of the last edit
        refused(lambda: g.splice_ranges(form([(10, 1, [bad]), (12, 0, [ok])])), rt.RT_ERR_INVALID)
        refused(lambda: g.splice_ranges(form([(12, 0, [ok]), (11, 0, [rt.sphere((0, 0, 2), 0.5, 1)])])), rt.RT_ERR_INVALID)
    refused(lambda: g.splice_ranges([(10, 2, []), (11, 1, [ok])]), rt.RT_ERR_INVALID)       # overlapping ranges
    refused(lambda: g.splice_ranges([(11, 0, [ok]), (11, 1, [])]), rt.RT_ERR_INVALID)       # the same first twice
    refused(lambda: g.splice_ranges([(11, 1, []), (0, 0, [])]), rt.RT_ERR_INVALID)          # first = 0, also for an empty edit
    refused(lambda: g.splice_ranges([(10, 1, []), (11, 2, [])]), rt.RT_ERR_INVALID)         # past the end
    refused(lambda: g.splice_ranges([(10, 1, []), (3, 1, [])]), rt.RT_ERR_INVALID)          # the cube
    refused(lambda: g.splice_ranges([(10, 0, [ok] * 300)]), rt.RT_ERR_UNSUPPORTED)          # one leaf of 300
    keep = np.ones(12, np.uint8)
    keep[0] = 0
    refused(lambda: g.compact_triangles(keep), rt.RT_ERR_INVALID)                           # primitive 0 stays
    keep[0], keep[3], keep[11] = 1, 0, 0
    refused(lambda: g.compact_triangles(keep), rt.RT_ERR_INVALID)                           # the cube
    refused(lambda: g.compact_triangles(torch.from_numpy(keep).to(f"cuda:{g.device}")), rt.RT_ERR_INVALID)
    g.splice_ranges([(10, 1, [ok]), (11, 1, [])])                                           # and the scene still splices
    assert_tree_is_hosts(rt, g, edited(prims, [(10, 1, [ok]), (11, 1, [])]))
    tp, tm, _ = range_cases["teapot"]
    sb = rt.Scene(tp, tm, bvh_kind=rt.BVH_SBVH)
    keep = np.ones(len(tp), np.uint8)
    keep[5] = 0
    for call in (lambda: sb.splice_ranges([(100, 10, []), (300, 1, [])]), lambda: sb.compact_triangles(keep)):
        with pytest.raises(rt.RTError) as e:
            call()
        assert e.value.code == rt.RT_ERR_UNSUPPORTED
