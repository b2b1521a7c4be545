"""Stream-ordered in-place updates: Scene.update_triangles / transform_triangles /
update_prims with wait=False enqueue on a stream and return; nothing on the host reads the check's flag.

Every case keeps a *twin* scene that receives the same edits through the blocking calls, and holds the
scene under test to it bit for bit: node bytes, closest hits (id and t / u / v bits), RGB8 frames,
accumulator bits.  The updates and the frames between them are queued without a synchronise -- one
update_sync() and one stream synchronise at the end of each queue -- so a frame that ran before the
update ahead of it, or an update that ran before the frame ahead of it, shows as a frame at the wrong
pose.  Frames are 64 x 64 unless stated."""
import numpy as np
import pytest

from anim_util import TIMES, room_mats, room_prims, split_tree, with_prims
from refit_util import scene_cases, tree_of, triangle_ids, twist, verts_of, with_verts
from test_refit_gpu import random_rays, runs

pytestmark = pytest.mark.gpu

W = H = 64
NAMES = ["kat", "leaf", "chain", "teapotF"]
KNOBS = ["RT_TILE_ORDER", "RT_PS_PIPELINE", "RT_PS_DEPTH", "RT_PT_PIPELINE", "RT_SPLIT_UNITS", "RT_SPLIT_HEAVY", "RT_WAVE_PRIMARY",
         "RT_PT_SLOTS", "RT_PT_MEM_MB"]
SERIAL = {"RT_PS_PIPELINE": "0", "RT_PT_PIPELINE": "0"}
# kind -> (environment at scene creation, frame depth, spp, result buffers once frames are in flight)
KINDS = {"serial": ({"RT_PS_PIPELINE": "0"}, 1, 1, 0),
         "in_flight_2": ({"RT_PS_PIPELINE": "1", "RT_PS_DEPTH": "2", "RT_WAVE_PRIMARY": "1", "RT_SPLIT_HEAVY": "64"}, 1, 1, 3),
         "in_flight_4": ({"RT_PS_PIPELINE": "1", "RT_PS_DEPTH": "4", "RT_WAVE_PRIMARY": "1", "RT_SPLIT_HEAVY": "64"}, 1, 1, 5),
         "path": ({"RT_PT_PIPELINE": "1"}, 3, 2, 0)}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cases(rt):
    return scene_cases(rt)


@pytest.fixture(scope="module")
def teapot(rt):
    prims, mats = rt.recipe_describe("teapotF")
    ids = triangle_ids(rt, prims)
    assert list(ids) == list(range(1, 1 + len(ids)))      # one run: the mesh, then the floor
    return prims, mats, ids


def scene_of(rt, monkeypatch, knobs, prims, mats, bvh=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return rt.Scene(prims, mats, bvh=bvh)


def dev(torch, g, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{g.device}")


def tick(torch, r, stream, frame, depth=1, spp=1):
    """one reset frame into a buffer of its own, on `stream` (a torch stream; None: the current one)"""
    out = torch.zeros(r.width * r.height, dtype=torch.int32, device=f"cuda:{r.scene.device}")
    return r.Tick(out, spp=spp, depth=depth, frame=frame, reset=True, stream=None if stream is None else stream.cuda_stream)


def hits(g, rays, stream=None):
    return [x.cpu().numpy() for x in g.IntersectBVH(rays, stream=stream)]


def assert_same_hits(got, want):
    gt, go, gu, gv = got
    wt, wo, wu, wv = want
    assert np.array_equal(go, wo), f"{(go != wo).sum()} ids differ"
    assert np.array_equal(gt.view(np.uint32), wt.view(np.uint32)), "t bits differ"
    hit = wo >= 0
    assert np.array_equal(gu[hit].view(np.uint32), wu[hit].view(np.uint32)) and np.array_equal(gv[hit].view(np.uint32), wv[hit].view(np.uint32))


def assert_same_scene(g, twin, rays):
    assert g.bvh()[0].tobytes() == twin.bvh()[0].tobytes(), "node bytes differ from the twin's"
    assert np.array_equal(g.bvh()[1], twin.bvh()[1])
    assert_same_hits(hits(g, rays), hits(twin, rays))


def assert_acc_equal(a, b):
    bad = (a.view(np.uint32) != b.view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{bad.sum()} accumulator pixels differ in their bits"


def twin_frames(rt, torch, twin, poses, first, depth=1, spp=1, frame0=0):
    """the blocking style: pose i, then its frame -- [(rgb8)] and the accumulator after the last"""
    t = rt.Renderer(twin, W, H)
    out = []
    for i, v in enumerate(poses):
        twin.update_triangles(first, v)
        out.append(tick(torch, t, None, frame0 + i, depth, spp).cpu().numpy())
    acc = t.accumulator()
    t.close()
    return out, acc


# ---- 1. same bytes

@pytest.mark.parametrize("name", NAMES)
def test_async_update_leaves_the_blocking_updates_bytes(rt, torch, cases, name):
    prims, mats, bvh = cases[name]
    ids = triangle_ids(rt, prims)
    new = with_verts(rt, prims, ids, twist(verts_of(prims, ids), 0.15))
    g, twin = rt.Scene(prims, mats, bvh=bvh), rt.Scene(prims, mats, bvh=bvh)
    before = g.bvh()[0].tobytes()
    tickets = []
    for first, count in runs(ids):
        v = verts_of(new, range(first, first + count))
        tickets.append(g.update_triangles(first, dev(torch, g, v), wait=False))
        twin.update_triangles(first, v)
    assert tickets == list(range(1, len(tickets) + 1))
    st = g.update_sync()
    assert (st["submitted"], st["applied"], st["refused"], st["first_refused"]) == (len(tickets), len(tickets), 0, 0), st
    assert st["refusal"] is None
    assert g.bvh()[0].tobytes() != before
    assert_same_scene(g, twin, random_rays(4096, 11))
    assert g.update_sync()["applied"] == len(tickets)       # nothing pending: the same counts again
    g.close()
    twin.close()


# ---- 2. no host wait between updates and frames

@pytest.mark.parametrize("kind", list(KINDS))
def test_updates_and_frames_queue_without_a_host_wait(rt, torch, monkeypatch, teapot, kind):
    prims, mats, ids = teapot
    knobs, depth, spp, buffers = KINDS[kind]
    first, rest = int(ids[0]), verts_of(prims, ids)
    poses = [twist(rest, 1.0 if i % 2 == 0 else -1.0) for i in range(6)]
    g = scene_of(rt, monkeypatch, knobs, prims, mats)
    r, big = rt.Renderer(g, W, H), rt.Renderer(g, 512, 512)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        # the renderer reaches its steady state first (tile order, frames in flight); the schedule is built
        lead = 0
        while lead < 4 or (buffers and r.device_bytes()[1] != buffers):
            assert lead < 24, ("frames in flight never formed", r.device_bytes(), r.overlap_depth())
            tick(torch, r, st, lead, depth, spp)
            lead += 1
        if buffers:
            assert r.overlap_depth()[0] == buffers - 1
        g.prepare_updates(st.cuda_stream)
        dposes = [dev(torch, g, v) for v in poses]
        torch.cuda.synchronize()
        before = g.update_sync()["submitted"]
        # a long frame first, so that the host is ahead of the GPU from here to the end
        tick(torch, big, st, 0, 10, 4)
        out = []
        for i, v in enumerate(dposes):
            assert g.update_triangles(first, v, stream=st.cuda_stream, wait=False) == before + i + 1
            out.append(tick(torch, r, st, i, depth, spp))
    status = g.update_sync()
    st.synchronize()
    assert status["applied"] == before + 6 and status["refused"] == 0
    got = [o.cpu().numpy() for o in out]
    acc = r.accumulator()
    twin = scene_of(rt, monkeypatch, SERIAL, prims, mats)
    want, wacc = twin_frames(rt, torch, twin, poses, first, depth, spp)
    assert not np.array_equal(want[0], want[1])             # a frame at the wrong pose would show
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{kind}: frame {i}: {(a != b).sum()} pixels differ from the twin's frame at pose {i}"
    assert_acc_equal(acc, wacc)
    assert_same_scene(g, twin, random_rays(4096, 12))
    for x in (r, big, g, twin):
        x.close()


# ---- 3. a refusal in the queue

def test_a_refusal_in_the_queue_leaves_the_others_alone(rt, torch, monkeypatch, teapot):
    prims, mats, ids = teapot
    first, rest = int(ids[0]), verts_of(prims, ids)
    A, B, C = twist(rest, 0.5), twist(rest, 1.0), twist(rest, -1.0)
    B[len(B) // 2, 4] = np.nan
    g = scene_of(rt, monkeypatch, {}, prims, mats)
    r = rt.Renderer(g, W, H)
    g.prepare_updates()
    st = torch.cuda.Stream()
    dA, dB, dC = (dev(torch, g, v) for v in (A, B, C))
    torch.cuda.synchronize()
    out, tickets = [], []
    with torch.cuda.stream(st):
        for i, v in enumerate((dA, dB, dC)):
            tickets.append(g.update_triangles(first, v, stream=st.cuda_stream, wait=False))
            out.append(tick(torch, r, st, i))
    status = g.update_sync()
    st.synchronize()
    assert (status["applied"], status["refused"], status["first_refused"]) == (2, 1, tickets[1]), status
    assert "NaN" in status["refusal"]
    assert g.update_sync()["first_refused"] == 0            # named once
    twin = scene_of(rt, monkeypatch, SERIAL, prims, mats)
    want, _ = twin_frames(rt, torch, twin, [A, A, C], first)    # the frame after B sees what A left
    for i, (a, b) in enumerate(zip(out, want)):
        assert np.array_equal(a.cpu().numpy(), b), f"frame {i}: {(a.cpu().numpy() != b).sum()} pixels differ"
    assert not np.array_equal(want[1], want[2])
    assert_same_scene(g, twin, random_rays(4096, 13))
    for x in (r, g, twin):
        x.close()


def test_a_refused_first_update_leaves_a_loose_tree_as_it_was(rt, torch, cases):
    """the root-leaf scene with its root box inflated by hand: a refit would tighten it, so its bytes
    surviving a refused update show that the refit launches were gated, not only the write"""
    prims, mats, bvh = cases["leaf"]
    loose = np.ascontiguousarray(bvh[0], np.uint8).copy()
    f = loose.view(np.float32).reshape(-1, 8)
    f[0, 0:3] -= np.float32(1.0)
    f[0, 3:6] += np.float32(1.0)
    g = rt.Scene(prims, mats, bvh=(loose, bvh[1]))
    assert g.bvh()[0].tobytes() == loose.tobytes() != np.ascontiguousarray(bvh[0]).tobytes()
    own = verts_of(prims, [1, 2])
    bad = own.copy()
    bad[1, 8] = np.inf
    rays = random_rays(4096, 14)
    h0 = hits(g, rays)
    assert g.update_triangles(1, dev(torch, g, bad), wait=False) == 1
    h1 = hits(g, rays)                                       # queued behind the refused update
    st = g.update_sync()
    assert (st["submitted"], st["applied"], st["refused"], st["first_refused"]) == (1, 0, 1, 1), st
    assert g.bvh()[0].tobytes() == loose.tobytes()           # downloaded from the device: the loose box survived
    assert_same_hits(h1, h0)
    assert g.update_triangles(1, dev(torch, g, own), wait=False) == 2
    st = g.update_sync()
    assert (st["applied"], st["refused"], st["first_refused"]) == (1, 1, 0), st
    assert g.bvh()[0].tobytes() == np.ascontiguousarray(bvh[0]).tobytes()   # the control: an applied update does refit
    g.close()


# ---- 4. matrices: more queued calls than the ring has slots

def test_twelve_matrix_updates_back_to_back(rt, torch, monkeypatch, teapot):
    prims, mats, ids = teapot
    n = len(ids)
    spans = [(1 + 301, n - 301), (1, 1), (1 + 1, 300)]      # out of order; one triangle, 300, the rest
    rest = np.concatenate([verts_of(prims, range(f, f + c)) for f, c in spans], axis=0)

    def ranges(k):
        a = np.float32(0.15 * (k + 1) * (-1 if k % 2 else 1))
        Ms = [rt.mat4_mul(rt.mat4_translate(0.02 * k, 0.01 * k, 0.0), rt.mat4_rotate(1, a)), rt.mat4_rotate(0, a),
              rt.mat4_mul(rt.mat4_rotate(1, a), rt.mat4_translate(0.0, 0.03 * k, 0.0))]
        return [(f, c, M) for (f, c), M in zip(spans, Ms)]

    g, twin = scene_of(rt, monkeypatch, {}, prims, mats), scene_of(rt, monkeypatch, SERIAL, prims, mats)
    r, t = rt.Renderer(g, W, H), rt.Renderer(twin, W, H)
    g.prepare_updates()
    drest = dev(torch, g, rest)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    out, want = [], []
    with torch.cuda.stream(st):
        for k in range(12):
            assert g.transform_triangles(ranges(k), drest, stream=st.cuda_stream, wait=False) == k + 1
            if k % 4 == 3:
                out.append(tick(torch, r, st, k))
    status = g.update_sync()
    st.synchronize()
    assert (status["submitted"], status["applied"], status["refused"]) == (12, 12, 0), status
    for k in range(12):
        twin.transform_triangles(ranges(k), rest)
        if k % 4 == 3:
            want.append(tick(torch, t, None, k).cpu().numpy())
    assert len(out) == 3 and not np.array_equal(want[0], want[1])
    for i, (a, b) in enumerate(zip(out, want)):
        assert np.array_equal(a.cpu().numpy(), b), f"frame {i}: {(a.cpu().numpy() != b).sum()} pixels differ"
    assert_acc_equal(r.accumulator(), t.accumulator())
    assert_same_scene(g, twin, random_rays(4096, 15))
    for x in (r, t, g, twin):
        x.close()


# ---- 5. every kind

def test_movers_of_every_kind_and_the_light_stays_with_the_blocking_call(rt, torch, monkeypatch):
    base, mats = room_prims(rt, 0.0), room_mats(rt)
    tree = split_tree(rt, base)
    g, twin = scene_of(rt, monkeypatch, {}, base, mats, tree), scene_of(rt, monkeypatch, SERIAL, base, mats, tree)
    r, t = rt.Renderer(g, W, H), rt.Renderer(twin, W, H)
    g.prepare_updates()
    st = torch.cuda.Stream()
    packed = []
    for time in TIMES[1:]:
        pose = room_prims(rt, time)
        rec, T = rt.pack_prims(pose[1:4])                    # the bouncing sphere, the corner sphere (still), the cube
        packed.append((pose, dev(torch, g, rec), dev(torch, g, T)))
    torch.cuda.synchronize()
    out, want = [], []
    with torch.cuda.stream(st):
        for k, (pose, rec, T) in enumerate(packed):
            assert g.update_prims(1, (rec, T), stream=st.cuda_stream, wait=False) == k + 1
            out.append(tick(torch, r, st, k))
        # the light's fields are the host's: refused at once, no ticket
        with pytest.raises(rt.RTError) as e:
            g.update_prims(0, (packed[0][1], packed[0][2]), stream=st.cuda_stream, wait=False)
        assert e.value.code == rt.RT_ERR_UNSUPPORTED
    status = g.update_sync()
    st.synchronize()
    assert (status["submitted"], status["applied"], status["refused"]) == (len(packed), len(packed), 0), status
    for k, (pose, rec, T) in enumerate(packed):
        twin.update_prims(1, pose[1:4])
        want.append(tick(torch, t, None, k).cpu().numpy())
    assert not np.array_equal(want[0], want[1])
    for i, (a, b) in enumerate(zip(out, want)):
        assert np.array_equal(a.cpu().numpy(), b), f"time {TIMES[1 + i]}: {(a.cpu().numpy() != b).sum()} pixels differ"
    assert_acc_equal(r.accumulator(), t.accumulator())
    assert_same_scene(g, twin, random_rays(4096, 16))
    for x in (r, t, g, twin):
        x.close()


# ---- 6. mixing the styles

@pytest.mark.parametrize("then", ["update", "rebuild", "splice", "bvh", "cost"])
def test_a_blocking_call_right_after_an_async_one(rt, torch, teapot, then):
    prims, mats, ids = teapot
    first, rest = int(ids[0]), verts_of(prims, ids)
    A, B = twist(rest, 0.4), twist(rest, -0.7)
    g, twin = rt.Scene(prims, mats), rt.Scene(prims, mats)
    g.update_triangles(first, dev(torch, g, A), wait=False)
    twin.update_triangles(first, A)
    if then == "update":
        g.update_triangles(first + 10, B[10:300])
        twin.update_triangles(first + 10, B[10:300])
    elif then == "rebuild":
        g.rebuild()
        twin.rebuild()
    elif then == "splice":
        extra = [rt.triangle((0.0, 0.2, 0.5), (0.3, 0.2, 0.5), (0.0, 0.5, 0.6), 1)]
        g.splice_triangles(first + 5, 3, extra)
        twin.splice_triangles(first + 5, 3, extra)
    elif then == "cost":
        assert g.bvh_cost() == twin.bvh_cost()
    assert_same_scene(g, twin, random_rays(4096, 17))        # "bvh": rt_scene_copy_bvh is the first call after the enqueue
    st = g.update_sync()
    assert (st["submitted"], st["applied"], st["refused"]) == (1, 1, 0), st
    g.close()
    twin.close()


# ---- 7. another stream

def test_readers_on_another_stream_see_the_update(rt, torch, monkeypatch, teapot):
    prims, mats, ids = teapot
    first, rest = int(ids[0]), verts_of(prims, ids)
    A = twist(rest, 1.0)
    g, twin = scene_of(rt, monkeypatch, {}, prims, mats), scene_of(rt, monkeypatch, SERIAL, prims, mats)
    r = rt.Renderer(g, W, H)
    g.prepare_updates()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    dA = dev(torch, g, A)
    rays = dev(torch, g, random_rays(4096, 18))
    before = tick(torch, r, None, 0).cpu().numpy()
    torch.cuda.synchronize()
    g.update_triangles(first, dA, stream=sa.cuda_stream, wait=False)
    with torch.cuda.stream(sb):                              # no event, no wait of the caller's between sa and sb
        frame = tick(torch, r, sb, 0)
        got = g.IntersectBVH(rays, stream=sb.cuda_stream)
    sb.synchronize()
    g.update_sync()
    want, _ = twin_frames(rt, torch, twin, [A], first)
    assert not np.array_equal(before, want[0])
    assert np.array_equal(frame.cpu().numpy(), want[0])
    assert_same_hits([x.cpu().numpy() for x in got], hits(twin, rays))
    for x in (r, g, twin):
        x.close()


# ---- 8. what the host refuses, it refuses at once

def test_host_side_refusals_take_no_ticket(rt, torch, teapot):
    prims, mats, ids = teapot
    first, n = int(ids[0]), len(ids)
    g = rt.Scene(prims, mats)
    v = dev(torch, g, verts_of(prims, ids))
    M = rt.mat4_translate(0.1, 0.0, 0.0)
    rec, T = (dev(torch, g, a) for a in rt.pack_prims(prims[1:3]))
    assert g.update_triangles(first, v[:4], wait=False) == 1
    submitted = g.update_sync()["submitted"]
    assert submitted == 1

    def refused(code, call):
        with pytest.raises(rt.RTError) as e:
            call()
        assert e.value.code == code, e.value

    refused(rt.RT_ERR_INVALID, lambda: g.update_triangles(0, v[:2], wait=False))                   # the light is no triangle
    refused(rt.RT_ERR_INVALID, lambda: g.update_triangles(len(prims) - 1, v[:2], wait=False))      # past the primitives
    refused(rt.RT_ERR_INVALID, lambda: g.update_triangles(first, verts_of(prims, ids), wait=False))   # a host array
    refused(rt.RT_ERR_INVALID, lambda: g.transform_triangles([(1, 300, M), (300, 10, M)], v[:310], wait=False))   # overlap
    refused(rt.RT_ERR_INVALID, lambda: g.transform_triangles([(0, 5, M)], v[:5], wait=False))
    refused(rt.RT_ERR_INVALID, lambda: g.transform_triangles([(1, 5, M)], verts_of(prims, ids)[:5], wait=False))  # a host array
    refused(rt.RT_ERR_INVALID, lambda: g.update_prims(len(prims) - 1, (rec, T), wait=False))
    refused(rt.RT_ERR_INVALID, lambda: g.update_prims(1, prims[1:3], wait=False))                  # host records
    refused(rt.RT_ERR_UNSUPPORTED, lambda: g.update_prims(0, (rec, T), wait=False))                # the light
    assert g.update_triangles(first, v[:0], wait=False) == 0                                       # count 0: RT_OK, no ticket
    assert g.transform_triangles([], v[:0], wait=False) == 0
    assert g.transform_triangles([(7, 0, M)], v[:0], wait=False) == 0
    sb = rt.Scene(prims, mats, bvh_kind=rt.BVH_SBVH)
    refused(rt.RT_ERR_UNSUPPORTED, lambda: sb.update_triangles(first, v[:4], wait=False))
    refused(rt.RT_ERR_UNSUPPORTED, lambda: sb.transform_triangles([(1, 4, M)], v[:4], wait=False))
    refused(rt.RT_ERR_UNSUPPORTED, lambda: sb.update_prims(1, (rec, T), wait=False))
    assert sb.update_sync()["submitted"] == 0
    st = g.update_sync()
    assert (st["submitted"], st["applied"], st["refused"]) == (submitted, 1, 0), st
    assert g.update_triangles(first, v[:4], wait=False) == submitted + 1                           # the next ticket follows
    g.close()
    sb.close()
