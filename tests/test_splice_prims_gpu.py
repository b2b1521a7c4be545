"""Scene.splice_prims, Scene.compact_prims and Scene.set_prim_materials on the GPU: primitives of any kind
leave and enter a live scene, and afterwards the scene is indistinguishable from one created fresh from
the edited list -- the host builder's node and index bytes, info, hit ids and t / u / v bits, occlusion,
RGB8 frames and accumulator bits in every mode, with whichever kernel family the new scene needs -- while
a renderer created before the edit stays valid, the new ids and side-table indices are what the in-place
updates address, and every refusal leaves the scene as it was.  Frames are 64 x 64."""
import numpy as np
import pytest

from anim_util import room_mats, room_prims
from test_rebuild_gpu import H, W, all_specs, assert_same_as_twin, assert_tree_is_hosts, frames, soup, walk_frame
from test_refit_gpu import assert_frames_equal
from test_splice_gpu import tick, triangles

pytestmark = pytest.mark.gpu

BOX = ((-5, -2, 2), (5, 2, 8))


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def mats4(rt):
    return [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.DIFFUSE, (0.8, 0.6, 0.5)),
            rt.material(rt.MIRROR, (0.9, 0.9, 0.9)), rt.material(rt.DIFFUSE, (0.3, 0.5, 0.9))]


def placed(rt, c, axis, angle):
    return rt.mat4_mul(rt.mat4_translate(float(c[0]), float(c[1]), float(c[2])), rt.mat4_rotate(axis, float(angle)))


def mixed(rt, n, seed, mat, planes=True):
    """n records of all five kinds in turn, centres in BOX (no box extreme at 0).  Planes are rare, stand
    outside the soup and are left out of the large soups: their boxes hold everything, no split separates
    them from anything, and a leaf of more than 255 primitives is refused by creation and rebuild alike."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = rng.uniform(*BOX).astype(np.float32)
        r, angle = float(rng.uniform(0.1, 0.3)), float(rng.uniform(0.0, 3.0))
        k = i % 9
        if k in (0, 5):
            out.append(rt.sphere(c, r, mat))
        elif k == 1:
            out.append(rt.cube((0, 0, 0), (r, 2 * r, r), mat, placed(rt, c, i % 3, angle)))
        elif k == 6:
            out.append(rt.cube(c, (r, r, 2 * r), mat))                    # placed by its position alone
        elif k in (3, 7):
            out.append(rt.quad(2 * r, mat, placed(rt, c, (i % 2) * 2, angle)))
        elif k == 8 and planes and i % 27 == 8:
            out.append(rt.plane((0, 1, 0), 9.0 + r, mat))
        else:
            out += triangles(rt, 1, seed * 1000 + i, *BOX, mat)
    return out


def edited(prims, edits):
    """the edits, in old ids, applied in descending order of first"""
    out = list(prims)
    for first, remove, new in sorted(edits, key=lambda e: -e[0]):
        out[first:first + remove] = list(new)
    return out


def on_device(rt, torch, g, edits):
    """the edits as (first, remove, (records, transforms) tensors, insert)"""
    allrec = [p for _, _, new in edits for p in new]
    if not allrec:
        return [(f, n, None, 0) for f, n, _ in edits]
    rec, T = rt.pack_prims(allrec)
    pair = (torch.from_numpy(rec).to(f"cuda:{g.device}"), torch.from_numpy(T).to(f"cuda:{g.device}"))
    return [(f, n, pair, len(new)) for f, n, new in edits]


def cubed_soup(rt):
    """soup(600) and the earlier edit that turns a triangle about every 40 ids into a cube or a quad"""
    base = soup(rt, 600, 61)
    rng = np.random.default_rng(62)
    edits, k, i = [], 17, 0
    while k < 600:
        c = rng.uniform(*BOX).astype(np.float32)
        new = rt.cube((0, 0, 0), (0.3, 0.2, 0.4), 3, placed(rt, c, 1, 0.7)) if i % 2 == 0 else rt.quad(0.5, 2, placed(rt, c, 0, 1.1))
        edits.append((k, 1, [new]))
        k += 37 + int(rng.integers(0, 8))
        i += 1
    assert len(edits) >= 14
    return base, edits


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (primitives, materials, [edit lists, one splice_prims call each], force the wave walk first)"""
    room = room_prims(rt, 0.0)
    up = placed(rt, (0.3, 0.4, 1.6), 0, 2.0)
    side = placed(rt, (-0.8, 0.6, 2.4), 2, 0.3)
    base, earlier = cubed_soup(rt)
    return {
        # the last cube leaves: has_cubes drops, the side table shrinks to the quad light's one entry
        "room-cube": (room, room_mats(rt), [[(3, 1, [])]], False),
        # a type change; every later cube's and quad's index shifts by one
        "room_sphere_to_cube": (room, room_mats(rt),
                                [[(1, 1, [rt.cube((0, 0, 0), (0.6, 0.7, 0.8), 2, placed(rt, (-1.4, -0.5, 2.0), 1, 0.5))])]], False),
        # all five kinds through one gather, inserted offsets in caller order
        "room_three_edits": (room, room_mats(rt),
                             [[(12, 0, [rt.quad(0.7, 1, up), rt.cube((0.1, 0.2, 0.1), 0.4, 3, side)]), (5, 1, []),
                               (1, 0, [rt.sphere((0.9, -0.6, 2.2), 0.25, 2)])]], False),
        # crosses kBuildWide = 64; ext flips on, the side table is allocated for the first time, the walk
        # policy must fall back
        "soup60+10mixed": (soup(rt, 60, 63), mats4(rt), [[(30, 0, mixed(rt, 10, 64, 2))]], True),
        # side-table ranks cross the 256-id scan groups, three groups so the top pass carries; crosses
        # kBuildChunk = 256
        "soup600": (base, mats4(rt), [earlier, [(230, 50, []), (40, 0, mixed(rt, 50, 65, 1, planes=False))]], False),
    }


def final_of(prims, calls):
    for edits in calls:
        prims = edited(prims, edits)
    return prims


def has_cube(rt, prims):
    return any(p.type == rt.CUBE for p in prims)


def check_against_twin(rt, oracle, g, r, twin, final, mats, want, want_acc, full):
    assert_tree_is_hosts(rt, g, final)
    assert g.info == twin.info and g.info["num_prims"] == len(final)
    assert np.array_equal(tick(r), want), "the renderer created before the edit"
    assert r.accumulator().tobytes() == want_acc.tobytes()
    if full:
        assert_same_as_twin(rt, oracle, g, twin, final, mats, all_specs(rt))
        if not has_cube(rt, final):
            a, b = walk_frame(rt, g), walk_frame(rt, twin)
            assert a[2] == b[2] and a[2]["verify_mismatch"] == 0
            assert_frames_equal([a[:2]], [b[:2]])


@pytest.mark.parametrize("name", ["room-cube", "room_sphere_to_cube", "room_three_edits", "soup60+10mixed", "soup600"])
def test_edited_scene_equals_a_fresh_one(rt, oracle, torch, cases, name):
    prims, mats, calls, force_wave = cases[name]
    final = final_of(prims, calls)
    twin = rt.Scene(final, mats)
    t = rt.Renderer(twin, W, H)
    want, want_acc = tick(t), t.accumulator().copy()
    t.close()
    for device in (False, True):                          # the records as host lists, as device tensors
        g = rt.Scene(prims, mats)
        if force_wave:
            g.set_camera_walk(rt.WALK_WAVE)               # ... which the first cube will rule out
        r = rt.Renderer(g, W, H)
        tick(r)                                           # a renderer has run on the old scene
        for edits in calls:
            g.splice_prims(on_device(rt, torch, g, edits) if device else edits)
        print(name, "device" if device else "host", g.info, "stats", g.rebuild_stats())
        check_against_twin(rt, oracle, g, r, twin, final, mats, want, want_acc, not device)
        if force_wave:
            with pytest.raises(rt.RTError):
                g.set_camera_walk(rt.WALK_WAVE)
        r.close()
        g.close()


def test_mask_drops_a_third_of_every_kind(rt, oracle, torch, cases):
    prims, mats, calls, _ = cases["soup600"]
    start = edited(prims, calls[0])
    keep = np.random.default_rng(66).uniform(size=len(start)) < 0.67
    keep[0] = True
    gone = [p.type for p, k in zip(start, keep) if not k]
    assert rt.CUBE in gone and rt.QUAD in gone and rt.TRIANGLE in gone
    final = [p for p, k in zip(start, keep) if k]
    twin = rt.Scene(final, mats)
    t = rt.Renderer(twin, W, H)
    want, want_acc = tick(t), t.accumulator().copy()
    t.close()
    for device in (False, True):
        g = rt.Scene(prims, mats)
        g.splice_prims(calls[0])
        r = rt.Renderer(g, W, H)
        tick(r)
        g.compact_prims(torch.from_numpy(keep.astype(np.uint8)).to(f"cuda:{g.device}") if device else keep)
        check_against_twin(rt, oracle, g, r, twin, final, mats, want, want_acc, not device)
        stats = g.rebuild_stats()
        g.compact_prims(np.ones(len(final), np.uint8))    # a mask that keeps everything does nothing
        assert g.rebuild_stats() == stats and g.info == twin.info
        r.close()
        g.close()


def moved(rt, p):
    """the record a little further on: the same type and material, as update_prims wants them"""
    d = np.array([0.1, 0.05, -0.1], np.float32)
    v = np.array(p.v[:], np.float32)
    if p.type == rt.SPHERE:
        return rt.sphere(v[:3] + d, float(v[3]), p.material)
    if p.type == rt.TRIANGLE:
        w = (v.reshape(3, 3) + d).astype(np.float32)
        return rt.triangle(w[0], w[1], w[2], p.material)
    T = rt.mat4_mul(rt.mat4_translate(*[float(x) for x in d]), np.eye(4, dtype=np.float32) if p.T is None else p.T)
    return rt.cube(v[:3], v[3:6], p.material, T) if p.type == rt.CUBE else rt.quad(float(v[0]), p.material, T)


def test_the_new_ids_and_side_table_indices_are_live(rt, torch, cases):
    """after the soup(600) edit: the schedule, then update_prims over a range holding kept and inserted
    cubes, quads, spheres and triangles"""
    prims, mats, calls, _ = cases["soup600"]
    final = final_of(prims, calls)
    g, twin = rt.Scene(prims, mats), rt.Scene(final, mats)
    for edits in calls:
        g.splice_prims(edits)
    assert not g.update_plan_info()["ready"]
    assert g.prepare_updates() > 0 and g.update_plan_info()["ready"]
    first, count = 30, 120                                # the 50 inserted at 40 .. 89, kept ones around them
    kinds = {p.type for p in final[first:first + count]}
    assert {rt.CUBE, rt.QUAD, rt.SPHERE, rt.TRIANGLE} <= kinds
    assert any(p.type == rt.CUBE for p in final[90:first + count]), "a kept cube, its index shifted by the inserted ones"
    now = list(final)
    now[first:first + count] = [moved(rt, p) for p in final[first:first + count]]
    for s in (g, twin):
        s.update_prims(first, now[first:first + count])
    assert g.bvh()[0].tobytes() == twin.bvh()[0].tobytes() and np.array_equal(g.bvh()[1], twin.bvh()[1])
    specs = all_specs(rt)
    assert_frames_equal(frames(rt, g, specs), frames(rt, twin, specs))
    assert_frames_equal(frames(rt, g, specs[:1]), frames(rt, rt.Scene(now, mats), specs[:1]))
    g.rebuild()
    assert_tree_is_hosts(rt, g, now)


def with_materials(rt, prims, first, materials):
    out = list(prims)
    for i, m in enumerate(materials):
        q = rt.Prim.from_buffer_copy(prims[first + i])
        q.material = int(m)
        q.T = getattr(prims[first + i], "T", None)
        out[first + i] = q
    return out


def test_set_prim_materials(rt, oracle, torch, cases):
    tp, tm = rt.recipe_describe("teapotF")
    tm = list(tm) + [rt.material(rt.MIRROR, (0.9, 0.9, 0.9)), rt.material(rt.DSMIX, (0.7, 0.8, 0.6), diffuse=0.6)]
    mirror, mix = len(tm) - 2, len(tm) - 1
    room, rm = room_prims(rt, 0.0), room_mats(rt)
    for prims, mats, first, steps in ((room, rm, 1, [[2] * 11, [3, 1, 2, 2, 1, 3, 1, 1, 2, 1, 3]]),
                                      (tp, tm, 400, [[mirror] * 300, [mix] * 300])):
        g = rt.Scene(prims, mats)
        g.prepare_updates()
        plan, stats = g.update_plan_info(), g.rebuild_stats()
        r = rt.Renderer(g, W, H)
        tick(r)
        for k, m in enumerate(steps):
            now = with_materials(rt, prims, first, m)
            twin = rt.Scene(now, mats)
            if k == 0:
                g.set_prim_materials(first, m)
            else:
                g.set_prim_materials(first, torch.tensor(m, dtype=torch.int32, device=f"cuda:{g.device}"))
            after = g.update_plan_info()
            assert after["ready"] and {**after, "launches": 0} == {**plan, "launches": 0} and g.rebuild_stats() == stats
            t = rt.Renderer(twin, W, H)
            assert np.array_equal(tick(r), tick(t)) and r.accumulator().tobytes() == t.accumulator().tobytes()
            t.close()
            assert_same_as_twin(rt, oracle, g, twin, now, mats, all_specs(rt))
            # update_prims checks its records against the new materials: it reads the same word
            g.update_prims(first, now[first:first + 2])
            with pytest.raises(rt.RTError):
                g.update_prims(first, prims[first:first + 2])
        g.set_prim_materials(first, [])                   # count == 0
        r.close()
        g.close()


def test_refusals_leave_the_scene_untouched(rt, torch):
    prims, mats = room_prims(rt, 0.0), room_mats(rt)
    g = rt.Scene(prims, mats)
    spec = [(rt.MODE_PATH, 1, 1)]
    nodes0, idx0, info0, frame0, stats0 = g.bvh()[0].copy(), g.bvh()[1].copy(), g.info, frames(rt, g, spec), g.rebuild_stats()
    ok = rt.sphere((0.5, 0.2, 2.0), 0.3, 1)
    inf = rt.mat4_translate(0.5, 0.2, 2.0).copy()
    inf.reshape(-1)[7] = np.inf

    def untouched():
        assert g.info == info0 and g.bvh()[0].tobytes() == nodes0.tobytes() and np.array_equal(g.bvh()[1], idx0)
        assert_frames_equal(frames(rt, g, spec), frame0)

    def refused(edits, device=False):
        with pytest.raises(rt.RTError) as e:
            g.splice_prims(on_device(rt, torch, g, edits) if device else edits)
        assert e.value.code == rt.RT_ERR_INVALID, e.value
        untouched()

    bad_type = rt.sphere((0.5, 0.2, 2.0), 0.3, 1)
    bad_type.type = 5
    for device in (False, True):
        refused([(12, 0, [ok, rt.sphere((0.5, 0.2, 2.0), float("nan"), 1)])], device)      # a NaN radius
        refused([(12, 0, [rt.sphere((0.5, 0.2, 2.0), 0.3, 4), ok])], device)               # material 4 of 4
        refused([(12, 0, [bad_type])], device)                                             # type 5
        refused([(3, 1, [rt.cube((0, 0, 0), 0.3, 1, inf)])], device)                       # an infinite transform entry for a cube
    refused([(0, 0, [ok])])                               # the light stays
    refused([(0, 1, [ok])])
    refused([(11, 2, [])])                                # past the end
    refused([(10, 2, []), (11, 1, [ok])])                 # overlap
    keep = np.ones(12, np.uint8)
    keep[0] = 0
    keep[3] = 0
    for k in (keep, torch.from_numpy(keep).to(f"cuda:{g.device}")):
        with pytest.raises(rt.RTError) as e:
            g.compact_prims(k)                            # a mask dropping id 0
        assert e.value.code == rt.RT_ERR_INVALID
        untouched()
    for first, m in ((0, [0]), (0, [1, 1]), (11, [1, 1]), (3, [1, 2, 4]), (3, [1, -1])):   # over id 0, past the end, out of range
        with pytest.raises(rt.RTError) as e:
            g.set_prim_materials(first, m)
        assert e.value.code == rt.RT_ERR_INVALID
        untouched()
    # the triangle entry points still refuse other kinds
    with pytest.raises(rt.RTError):
        g.splice_ranges([(3, 1, [])])
    with pytest.raises(rt.RTError):
        g.splice_triangles(12, 0, [ok])
    untouched()
    g.splice_prims([(5, 0, [])])                          # an empty edit does nothing
    assert g.rebuild_stats() == stats0 and g.info == info0
    g.splice_prims([(3, 1, [ok])])                        # and the scene still edits
    assert_tree_is_hosts(rt, g, edited(prims, [(3, 1, [ok])]))
    tp, tm = rt.recipe_describe("teapotF")
    sb = rt.Scene(tp, tm, bvh_kind=rt.BVH_SBVH)
    with pytest.raises(rt.RTError) as e:
        sb.splice_prims([(100, 10, [])])
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
