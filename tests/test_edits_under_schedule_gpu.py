"""Scene edits under renderers that carry scheduling state.

Every edit of a live scene promises two things (include/rt_amd.h): afterwards the scene is bit for bit a
fresh one, and the renderers keep their timed choices, tile orders and deals, which change speed only.  The
edit tests check the first on a renderer that has run one 64 x 64 frame, which has no such state; the
schedule tests check the second on scenes that never change.  Here a renderer is first driven into a named
scheduling state -- a measured tile order with half-tile units, decided or half-timed choices, frames in
flight on its own streams, sample-split buffers, path-state slots, a held shard or deal, Whitted orders --
the state is asserted through its accessor (tile_costs, choices, device_bytes), the scene is edited, and
every later frame is held to three references:

* the control: the same script on a scene created with RT_TILE_ORDER, RT_PS_PIPELINE, RT_PT_PIPELINE,
  RT_SPLIT_UNITS and RT_WAVE_PRIMARY all 0, whose renderer therefore has no scheduling state -- every
  frame's RGB8, the final accumulator and the ray counters, bit for bit;
* a fresh renderer on a fresh twin scene of the edited description -- the frames from the first reset
  frame after each edit, RGB8 and accumulator bits; the edited scene's tree is the host's;
* the oracle over the twin's tree -- the same frames, RGB8 and accumulator bits.

The control shares the edit code with the run under test; the twin and the oracle do not.  Frames are
200 x 120 (375 tiles): at 64 x 64 no order, split or overlap ever forms.  Frames go to device tensors on
one stream, back to back; the frames-in-flight and path-state-slot cases synchronise once, at the end."""
from collections import namedtuple

import numpy as np
import pytest

from anim_util import room_mats, room_prims, split_tree, with_prims
from refit_util import triangle_ids, twist, verts_of, with_verts
from scenes_util import oracle_scene
from test_gpu_parity import assert_acc_bits
from test_rebuild_gpu import assert_tree_is_hosts, soup
from test_refit_gpu import update
from test_splice_gpu import triangles
from test_splice_prims_gpu import edited, mats4, mixed, with_materials

pytestmark = pytest.mark.gpu

SIZE = (200, 120)
TILES_X = 25
NT = 375                  # 25 x 15 tiles of 8 x 8

PATH, WHITTED, HEAT = 0, 1, 3     # rt.MODE_PATH, rt.MODE_WHITTED, rt.MODE_BVH_HEAT

# Frames a renderer may need before its accessor reports the state, from csrc/rt_tune.h.  A two-way choice
# (start_two_way) runs 4 groups of kTuneGroup = 4 frames and decides on the frame after them: 16 + 1, and
# the camera walk one warm-up frame before them.  A group whose frames the host submitted slower than the
# GPU rendered them starts again, at most kTuneRestarts = 4 times and from at most its 4th frame: up to
# 4 x 3 more frames for each of the 4 groups.  The walk is decided first (1 + 16 + 1 + 48 = 66 frames),
# the split order after it (16 + 1 + 48 = 65), and a set without a timed walk spends two frames on its
# order (one records the costs, the next sorts them): 66 + 65 + 2 = 133.  A lead-in that reaches the cap
# fails its test.
LEAD_CAP = 133

CONTROL = {"RT_TILE_ORDER": "0", "RT_PS_PIPELINE": "0", "RT_PT_PIPELINE": "0", "RT_SPLIT_UNITS": "0", "RT_WAVE_PRIMARY": "0"}
FORCED = {"RT_TILE_ORDER": "1", "RT_SPLIT_HEAVY": "64", "RT_SPLIT_PARTS": "4", "RT_XCD_ORDER": "1", "RT_WAVE_PRIMARY": "1",
          "RT_TUNE_DELAY_MS": "0"}
TIMED = {"RT_TUNE_DELAY_MS": "0"}                        # walk AUTO, RT_SPLIT_HEAVY = -1: both timed
IN_FLIGHT = {"RT_PS_PIPELINE": "1", "RT_PS_DEPTH": "4", "RT_WAVE_PRIMARY": "1", "RT_SPLIT_HEAVY": "64", "RT_TUNE_DELAY_MS": "0"}
SAMPLE_SPLIT = {"RT_SPLIT_UNITS": "1000000", "RT_TUNE_DELAY_MS": "0"}
# launch_pt_frame: a depth-4 path holds 32 + 16 + 8 + 3 x 32 = 152 B, 24,000 pixels 3.65 MB a sample: with
# 4 MB of path state a 4 spp frame runs as four batches of one sample, one on each of the four slots
PT_SLOTS = {"RT_PT_PIPELINE": "1", "RT_PT_SLOTS": "4", "RT_PT_MEM_MB": "4", "RT_TUNE_DELAY_MS": "0"}
KNOBS = sorted(set().union(CONTROL, FORCED, TIMED, IN_FLIGHT, SAMPLE_SPLIT, PT_SLOTS))

Frame = namedtuple("Frame", "mode spp depth frame reset part", defaults=(PATH, 1, 1, 0, False, None))
# part: None the whole frame; ("shard", k, n) the interleaved shard k of n, packed; ("tiles", list) an explicit
# deal's share, packed; ("deal", tiles, off) every share of a deal one after the other, assembled to a whole frame


@pytest.fixture(scope="module")
def torch():
    """every test takes it: torch opens the device before the module's first scene does"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---- scene descriptions and the edits

class Desc:
    """primitives, materials and the tree a scene of them holds: the host builder's (tree None), or for a
    scene that was refitted the host refit of the tree it had (nodes, indices)"""

    def __init__(self, prims, mats, tree=None):
        self.prims, self.mats, self.tree = list(prims), list(mats), tree

    def host_tree(self, rt):
        if self.tree is not None:
            return self.tree
        nodes, idx, _ = rt.build_bvh_host(self.prims)
        return nodes, idx

    def refitted(self, rt, prims):
        nodes, idx = self.host_tree(rt)
        return Desc(prims, self.mats, (rt.refit_bvh_host(prims, nodes, idx), idx))


def scene_of(rt, monkeypatch, knobs, d):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return rt.Scene(d.prims, d.mats, bvh=d.tree)


def base_scene(rt, name):
    if name == "teapot":
        return Desc(*rt.recipe_describe("teapotF"))
    if name == "room":                                    # the planes in a leaf of their own: a refit moves boxes
        prims = room_prims(rt, 0.0)
        return Desc(prims, room_mats(rt), split_tree(rt, prims))
    n, seed = {"soup60": (60, 63), "soup300": (300, 71), "soup600": (600, 73)}[name]
    return Desc(soup(rt, n, seed), mats4(rt))


# An edit: (rt, torch, description before) -> (apply(scene), description after)

def edit_twist(rt, torch, d):
    """(a) update_triangles: every triangle twisted by 1 rad per unit of y, the vertices on the device"""
    ids = triangle_ids(rt, d.prims)
    new = with_verts(rt, d.prims, ids, twist(verts_of(d.prims, ids), 1.0))
    return (lambda g: update(g, new, ids, device=torch)), d.refitted(rt, new)


def edit_light(rt, torch, d):
    """(b) update_prims over [0, 2): the room's quad light and its bouncing sphere at t = 1.3"""
    new = with_prims(d.prims, 0, room_prims(rt, 1.3)[0:2])
    return (lambda g: g.update_prims(0, new[0:2])), d.refitted(rt, new)


def edit_xform(rt, torch, d):
    """(c) transform_triangles: two ranges given out of order, the vertices they have now as their rest pose"""
    spans = [(500, 200), (1, 300)]
    Ms = [rt.mat4_mul(rt.mat4_translate(0.3, 0.2, -0.1), rt.mat4_rotate(1, np.float32(0.4))), rt.mat4_translate(-0.2, 0.3, 0.1)]
    new, rest = d.prims, []
    for (first, n), M in zip(spans, Ms):
        v = verts_of(d.prims, range(first, first + n))
        world = rt.mesh_to_prims(v.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3), M, 1)
        new = with_verts(rt, new, range(first, first + n), verts_of(world, range(n)))
        rest.append(v)
    rest = np.concatenate(rest, axis=0)
    return (lambda g: g.transform_triangles([(f, n, M) for (f, n), M in zip(spans, Ms)], rest)), d.refitted(rt, new)


def edit_twist_rebuild(rt, torch, d):
    """(d) rebuild after (a)"""
    apply, moved = edit_twist(rt, torch, d)

    def both(g):
        apply(g)
        g.rebuild()
    return both, Desc(moved.prims, d.mats)


def deepest_leaf_box(nodes):
    f, u = nodes.view(np.float32).reshape(-1, 8), nodes.view(np.uint32).reshape(-1, 8)
    best, st = (-1, 0), [(0, 0)]
    while st:
        k, depth = st.pop()
        if u[k, 7]:
            best = max(best, (depth, k))
        else:
            st += [(int(u[k, 6]), depth + 1), (int(u[k, 6]) + 1, depth + 1)]
    return f[best[1], 0:3].copy(), f[best[1], 3:6].copy()


def edit_deepen(rt, torch, d):
    """(e) splice_ranges: 24 triangles a twentieth the soup's size in the middle of the deepest leaf's box, in
    two ranges (one also removes five): the builder cuts the cluster below that leaf, the tree gets deeper"""
    nodes, _, info = rt.build_bvh_host(d.prims)
    lo, hi = deepest_leaf_box(nodes)
    c = (lo + hi) * np.float32(0.5)
    tight = []
    for t in triangles(rt, 24, 72, c - np.float32(0.01), c + np.float32(0.01), 1):
        v = np.array(t.v[:9], np.float32).reshape(3, 3)
        m = v.mean(axis=0, dtype=np.float32)
        v = (m + (v - m) * np.float32(0.05)).astype(np.float32)
        tight.append(rt.triangle(v[0], v[1], v[2], 1))
    edits = [(150, 0, tight[:12]), (40, 5, tight[12:])]
    new = edited(d.prims, edits)
    assert rt.build_bvh_host(new)[2]["depth"] > info["depth"]

    def apply(g):
        before = g.info["depth"]
        g.splice_ranges(edits)
        assert g.info["depth"] > before, (before, g.info)
    return apply, Desc(new, d.mats)


def edit_drop_half(rt, torch, d):
    """(f) compact_triangles: half the triangles leave, the mask on the device"""
    keep = np.random.default_rng(74).uniform(size=len(d.prims)) < 0.5
    keep[0] = True
    new = [p for p, k in zip(d.prims, keep) if k]
    return (lambda g: g.compact_triangles(torch.from_numpy(keep.astype(np.uint8)).to(f"cuda:{g.device}"))), Desc(new, d.mats)


def has_cube(rt, prims):
    return any(p.type == rt.CUBE for p in prims)


def edit_flip_in(rt, torch, d):
    """(g) splice_prims: ten records of every kind enter soup(60), a cube among them: the scene needs the
    other kernel family and no longer admits the wave walk"""
    new = mixed(rt, 10, 64, 2)
    assert has_cube(rt, new) and not has_cube(rt, d.prims)
    edits = [(30, 0, new)]
    return (lambda g: g.splice_prims(edits)), Desc(edited(d.prims, edits), d.mats)


def edit_flip_out(rt, torch, d):
    """(g) compact_prims: they leave again, and five triangles with them: back to the first family"""
    keep = np.ones(len(d.prims), np.uint8)
    keep[30:40] = 0
    keep[50:55] = 0
    new = [p for p, k in zip(d.prims, keep) if k]
    assert has_cube(rt, d.prims) and not has_cube(rt, new)
    return (lambda g: g.compact_prims(keep)), Desc(new, d.mats)


def edit_mirror(rt, torch, d, first=100, count=100):
    """(h) set_prim_materials: a hundred diffuse triangles become mirrors; nothing is rebuilt or refitted"""
    assert all(p.material == 1 for p in d.prims[first:first + count]) and d.mats[2].kind == rt.MIRROR
    new = with_materials(rt, d.prims, first, [2] * count)
    mats = torch.full((count,), 2, dtype=torch.int32)
    return (lambda g: g.set_prim_materials(first, mats.to(f"cuda:{g.device}"))), Desc(new, d.mats, d.tree)


EDITS = {"a": ("teapot", [edit_twist]), "b": ("room", [edit_light]), "c": ("teapot", [edit_xform]),
         "d": ("teapot", [edit_twist_rebuild]), "e": ("soup300", [edit_deepen]), "f": ("soup600", [edit_drop_half]),
         "g": ("soup60", [edit_flip_in, edit_flip_out]), "h": ("soup300", [edit_mirror])}


# ---- frames

def tiles_of(part):
    if part is None or part[0] == "deal":
        return np.arange(NT, dtype=np.uint32)
    if part[0] == "shard":
        return np.arange(part[1], NT, part[2], dtype=np.uint32)
    return np.asarray(part[1], np.uint32)


def pixels_of(part):
    """the pixels a frame covers, in the order of its output: row-major, or packed [tile][64]"""
    W, H = SIZE
    if part is None or part[0] == "deal":
        return np.arange(W * H)
    t = tiles_of(part).astype(np.int64)[:, None]
    lane = np.arange(64)[None, :]
    return ((t % TILES_X) * 8 + (lane & 7) + ((t // TILES_X) * 8 + (lane >> 3)) * W).reshape(-1)


def same_pixels(a, b):
    whole = lambda p: p is None or p[0] == "deal"
    return (whole(a) and whole(b)) or (not whole(a) and not whole(b) and np.array_equal(tiles_of(a), tiles_of(b)))


def submit(torch, r, f, stream):
    """one frame of renderer r into a new device tensor, on `stream`"""
    W, H = SIZE
    dev = f"cuda:{r.scene.device}"
    kw = dict(spp=f.spp, depth=f.depth, frame=f.frame, reset=f.reset, stream=stream)
    r.mode = f.mode
    if f.part is None:
        return r.Tick(torch.zeros(W * H, dtype=torch.int32, device=dev), **kw)
    if f.part[0] == "shard":
        return r.render_shard(torch.zeros(r.shard_capacity(f.part[2]), dtype=torch.int32, device=dev), f.part[1], f.part[2], **kw)
    if f.part[0] == "tiles":
        return r.render_shard_tiles(torch.zeros(64 * len(f.part[1]), dtype=torch.int32, device=dev), f.part[1], **kw)
    tiles, off = f.part[1:]
    stride = 64 * int(np.diff(off).max())
    bufs = torch.zeros((len(off) - 1) * stride, dtype=torch.int32, device=dev)
    for k in range(len(off) - 1):
        r.render_shard_tiles(bufs[k * stride:(k + 1) * stride], tiles[off[k]:off[k + 1]], **kw)
    return r.assemble_tiles(bufs, stride, tiles, off, torch.zeros(W * H, dtype=torch.int32, device=dev), stream=stream)


class Run:
    """One pass of a script: one scene, one renderer created before any edit, one stream.  The run under
    test finds the lengths of the lead-ins; the control replays them."""

    def __init__(self, rt, torch, scene, control, shared):
        self.rt, self.torch, self.g, self.control, self.shared = rt, torch, scene, control, shared
        self.r = rt.Renderer(scene, *SIZE)
        self.st = torch.cuda.Stream()
        self.out, self.spec, self.acc, self.checks = [], [], {}, []
        self.nlead = 0
        self.c0 = self.r.counters()

    def frame(self, f):
        with self.torch.cuda.stream(self.st):
            self.out.append(submit(self.torch, self.r, f, self.st.cuda_stream))
        self.spec.append(f)
        return len(self.out) - 1

    def frames(self, fs):
        return [self.frame(f) for f in fs]

    def lead_in(self, until, f=Frame(), at_least=0):
        """frames 0, 1, ... of f's parameter set until the accessor reports the state (at_least: where the
        previous set's state could pass for it); never past LEAD_CAP"""
        if self.control:
            n = self.shared["leads"][self.nlead]
        else:
            n = 0
            while n < at_least or not until(self.r):
                if n >= LEAD_CAP:
                    pytest.fail(f"the state was not reached within {LEAD_CAP} frames: choices {self.r.choices()}, "
                                f"{len(self.r.tile_costs())} tile costs, device bytes {self.r.device_bytes()}")
                self.frame(f._replace(frame=n))
                n += 1
            self.shared["leads"].append(n)
        if self.control:
            self.frames([f._replace(frame=k) for k in range(n)])
        self.nlead += 1
        return n

    def reached(self, what, check):
        """the state's assertion, on the run under test"""
        if not self.control:
            assert check(self.r), (what, self.r.choices(), len(self.r.tile_costs()), self.r.device_bytes())

    def read_acc(self):
        """the accumulator after the last frame submitted (synchronises the device)"""
        self.acc[len(self.out) - 1] = self.r.accumulator()

    def edit(self, apply, d):
        apply(self.g)
        if self.control:
            return
        assert self.g.info["num_prims"] == len(d.prims)
        if d.tree is None:
            assert_tree_is_hosts(self.rt, self.g, d.prims)
        else:
            nodes, idx = self.g.bvh()
            assert nodes.tobytes() == d.tree[0].tobytes(), "node bytes differ from the host refit's"
            assert np.array_equal(idx, d.tree[1])

    def segment(self, fs, d, acc):
        """the frames after an edit, the first with reset: later held to the twin and the oracle.  acc: "now"
        reads the accumulator after the first and the last of them, "end" takes the one read at the end of
        the run (they are the script's last frames), None compares RGB8 alone"""
        assert fs[0].reset
        first = self.frame(fs[0])
        if acc == "now":
            self.read_acc()
        idx = [first] + self.frames(fs[1:])
        if acc == "now":
            self.read_acc()
        self.checks.append((idx, d, acc))
        return idx

    def finish(self):
        self.torch.cuda.synchronize()
        self.host = [o.cpu().numpy() for o in self.out]
        self.acc[len(self.out) - 1] = self.r.accumulator()
        c = self.r.counters()
        self.counted = {k: c[k] - self.c0[k] for k in c}

    def close(self):
        self.r.close()
        self.g.close()


def assert_runs_equal(test, ctrl):
    assert len(test.host) == len(ctrl.host)
    c = ctrl.r                                            # the control never had any of the state
    assert len(c.tile_costs()) == 0 and c.device_bytes()[1] == 0 and c.overlap_depth()[0] == 1 and c.choices()["walk"] == 0
    for i, (a, b) in enumerate(zip(test.host, ctrl.host)):
        assert np.array_equal(a, b), f"frame {i} {test.spec[i][:5]}: {(a != b).sum()} pixels differ from the control's"
    last = len(test.out) - 1
    assert_acc_bits(test.acc[last], ctrl.acc[last])
    assert test.counted == ctrl.counted, (test.counted, ctrl.counted)


def oracle_frames(o, fs, acc=None):
    """[(rgb8 of the whole frame, accumulator after it) or None for a heat frame] -- the oracle ticks whole
    frames, so the pixels a frame covers must have been covered by every frame since the last reset"""
    W, H = SIZE
    acc = np.zeros((W * H, 4), np.float32) if acc is None else acc
    out = []
    for i, f in enumerate(fs):
        assert f.reset or i == 0 or same_pixels(f.part, fs[i - 1].part)
        if f.mode == HEAT:                                # not the oracle's: the next frame starts over
            assert f.reset and (i + 1 == len(fs) or fs[i + 1].reset)
            out.append(None)
            continue
        if f.reset:
            acc[:] = 0
        o.set_integrator(f.mode)
        rgb, _ = o.tick(W, H, acc, spp=f.spp, depth=f.depth, frame=f.frame)
        out.append((rgb, acc.copy()))
    o.set_integrator(0)
    return out


def assert_fresh(rt, oracle, torch, monkeypatch, run, end_work=False):
    """every segment of the run under test against a fresh renderer on a fresh twin scene, and the oracle"""
    last = len(run.out) - 1
    for c, (idx, d, acc) in enumerate(run.checks):
        fs = [run.spec[i] for i in idx]
        twin = scene_of(rt, monkeypatch, CONTROL, d)
        t = rt.Renderer(twin, *SIZE)
        o = oracle_scene(rt, oracle, d.prims, d.mats, bvh=twin.bvh())
        want = oracle_frames(o, fs)
        for k, (i, f) in enumerate(zip(idx, fs)):
            px = pixels_of(f.part)
            # a deal's shares assemble to the whole frame: the twin renders that
            tf = f._replace(part=None) if f.part is not None and f.part[0] == "deal" else f
            rgb = submit(torch, t, tf, None).cpu().numpy()
            got = run.host[i]
            assert np.array_equal(got, rgb), f"frame {i} {f[:5]}: {(got != rgb).sum()} pixels differ from the fresh twin's"
            gacc = run.acc.get(i) if (acc == "now" or (acc == "end" and i == last)) else None
            if gacc is not None:
                assert_acc_bits(gacc[px], t.accumulator()[px])
            if want[k] is None:
                continue
            orgb, oacc = want[k]
            assert np.array_equal(got[:len(px)], orgb[px]), f"frame {i} {f[:5]}: {(got[:len(px)] != orgb[px]).sum()} pixels differ from the oracle's"
            if gacc is not None:
                assert_acc_bits(gacc[px], oacc[px])
        if end_work and c == len(run.checks) - 1:   # the dry-run work map of the renderer that saw the edit
            assert np.array_equal(run.r.tile_work(spp=1, depth=1, frame=0), t.tile_work(spp=1, depth=1, frame=0))
        t.close()
        twin.close()


# ---- the states: lead(run, k) brings the renderer into the state before edit k and asserts it;
# after(k, last) gives the frames that follow edit k and how their accumulator is read

def ordered_split(n=NT):
    return lambda r: len(r.tile_costs()) == n and r.choices()["split"] == 1


class Forced:
    """1: a measured order with the 64 costliest tiles in quarters, XCD-grouped, the wave walk forced"""
    knobs = FORCED
    part = None

    def lead(self, run, k):
        f = Frame(part=self.part)
        n = run.lead_in(ordered_split(len(tiles_of(self.part))), f)
        run.reached("order and split", ordered_split(len(tiles_of(self.part))))
        run.frames([f._replace(frame=n + j) for j in range(3)])

    def after(self, k, last):
        p = self.part
        fs = [Frame(frame=0, reset=True, part=p), Frame(frame=1, part=p), Frame(frame=2, part=p)]
        if p is None:
            fs.append(Frame(PATH, 1, 4, 3))               # depth 4 samples the light
        return fs, "now"

    def tail(self, run):
        pass


class ForcedEighth(Forced):
    """... with RT_SPLIT_PARTS=8 on shard 1 of 8: every one of its 47 tiles in eighths, an order of 9 x 47"""
    knobs = dict(FORCED, RT_SPLIT_PARTS="8")
    part = ("shard", 1, 8)


def decided(r):
    c = r.choices()
    return c["walk"] in (0, 1) and c["split"] in (0, 1)


class Timed:
    """2: the camera walk and the split order timed and decided"""
    knobs = TIMED

    def lead(self, run, k):
        n = run.lead_in(decided)
        run.reached("walk and split decided", decided)
        run.frames([Frame(frame=n + j) for j in range(3)])

    def after(self, k, last):
        return [Frame(frame=0, reset=True)] + [Frame(frame=j) for j in range(1, 4)], "now"

    def tail(self, run):
        pass


class MidTiming(Timed):
    """3: the edit lands while the walk is being timed -- after its warm-up frame and five more frames, the
    first timed group's events recorded, nothing decided (a decision takes 18 frames at least) -- and the
    script goes on until the walk is decided"""

    def lead(self, run, k):
        if k == 0:
            run.frames([Frame(frame=j) for j in range(6)])
            run.reached("the walk's timing is running", lambda r: r.choices()["walk"] == -1)

    def tail(self, run):
        n = run.lead_in(lambda r: r.choices()["walk"] in (0, 1), Frame(frame=0))
        run.reached("the walk is decided", lambda r: r.choices()["walk"] in (0, 1))
        run.frames([Frame(frame=n + j) for j in range(3)])


class InFlight:
    """4: four frames in flight on the renderer's streams, five result buffers; eight frames before the edit
    and eight after it with no synchronisation but the edit's own"""
    knobs = IN_FLIGHT

    def lead(self, run, k):
        n = run.lead_in(lambda r: r.device_bytes()[1] == 5)
        run.reached("depth + 1 result buffers", lambda r: r.device_bytes()[1] == 5 and r.overlap_depth()[0] == 4)
        run.frames([Frame(frame=n + j) for j in range(8)])

    def after(self, k, last):
        fs = [Frame(frame=0, reset=True)] + [Frame(frame=j) for j in range(1, 8)] + [Frame(PATH, 1, 4, 8)]
        return fs, ("end" if last else None)

    def tail(self, run):
        pass


class SampleSplit:
    """5: (tile, sample chunk) units and their sample buffer: whole frames at spp 4, shard 1 of 3 at spp 8"""
    knobs = SAMPLE_SPLIT
    whole, third = Frame(PATH, 4, 1), Frame(PATH, 8, 1, part=("shard", 1, 3))

    def lead(self, run, k):
        b0 = run.r.device_bytes()[0]
        run.frame(self.whole)
        if k == 0:          # 4 samples x 375 tiles x 64 float4: the sample buffer, no result buffer of frames in flight
            run.reached("sample buffer", lambda r: r.device_bytes()[0] - b0 >= 4 * NT * 64 * 16 and r.device_bytes()[1] == 0)
        run.frames([self.whole._replace(frame=j) for j in range(1, 9)])
        run.frames([self.third._replace(frame=j, reset=j == 0) for j in range(4)])
        run.frames([self.whole._replace(frame=j, reset=j == 0) for j in range(4)])

    def after(self, k, last):
        fs = [self.whole._replace(frame=j, reset=j == 0) for j in range(3)]
        return fs + [self.third._replace(frame=3 + j, reset=j == 0) for j in range(3)], "now"

    def tail(self, run):
        pass


class PathSlots:
    """6: the pipelined wavefront path tracer, four batches a frame on four path-state slots and streams;
    frames back to back around the edit"""
    knobs = PT_SLOTS
    f = Frame(PATH, 4, 4)

    def lead(self, run, k):
        b0 = run.r.device_bytes()[0]
        run.frame(self.f)
        if k == 0:          # the slots' path state and the frame's per-sample results
            run.reached("path-state slots", lambda r: r.device_bytes()[0] - b0 >= 4 * NT * 64 * 16)
        run.frames([self.f._replace(frame=j) for j in range(1, 8)])

    def after(self, k, last):
        return [self.f._replace(frame=j, reset=j == 0) for j in range(8)], ("end" if last else None)

    def tail(self, run):
        pass


class Deals(Forced):
    """7: shard 1 of 3, then share 0 of a deal cut from the old scene's work map; after the edit the same
    deal renders the new scene, every share, assembled"""
    third = ("shard", 1, 3)

    def lead(self, run, k):
        n = run.lead_in(ordered_split(125), Frame(part=self.third))
        run.reached("the shard's order", ordered_split(125))
        if k == 0:
            work = run.r.tile_work(spp=1, depth=1, frame=0)
            deal = run.rt.tile_deal(*SIZE, 3, work)
            if not run.control:
                run.shared["deal"] = deal
            assert all(np.array_equal(a, b) for a, b in zip(deal, run.shared["deal"]))
        tiles, off = run.shared["deal"]
        share = ("tiles", tiles[off[0]:off[1]])
        n = run.lead_in(ordered_split(int(off[1] - off[0])), Frame(part=share), at_least=2)   # one records, the next sorts
        run.reached("the share's order", ordered_split(int(off[1] - off[0])))
        run.frames([Frame(frame=n + j, part=share) for j in range(2)])
        self.deal = ("deal", tiles, off)

    def after(self, k, last):
        fs = [Frame(frame=0, reset=True, part=self.deal), Frame(frame=1, part=self.deal)]
        return fs + [Frame(frame=2, reset=True, part=self.third), Frame(frame=3, part=self.third)], "now"


class WhittedHeat(Forced):
    """8: Whitted frames (whole-tile orders of their own set) and heat frames (their depth is the tree's)
    between path frames"""
    w = Frame(WHITTED, 1, 4)

    def lead(self, run, k):
        Forced.lead(self, run, k)
        order = lambda r: len(r.tile_costs()) == NT and r.choices()["split"] == 0
        n = run.lead_in(order, self.w)
        run.reached("the Whitted set's order", order)
        run.frame(self.w._replace(frame=n))

    def after(self, k, last):
        heat = Frame(HEAT, 1, 1, reset=True)
        return [self.w._replace(frame=0, reset=True), self.w._replace(frame=1), heat._replace(frame=2),
                Frame(frame=3, reset=True), Frame(frame=4), heat._replace(frame=5), self.w._replace(frame=6, reset=True)], "now"


STATES = {"forced": Forced, "forced_eighth": ForcedEighth, "timed": Timed, "mid_timing": MidTiming, "in_flight": InFlight,
          "sample_split": SampleSplit, "path_slots": PathSlots, "deals": Deals, "whitted_heat": WhittedHeat}

# every edit under states 1 and 4; everywhere else a refit, a rebuild that changes the count, the family flip
CASES = ([("forced", e) for e in "abcdefgh"] + [("forced_eighth", "e")] + [("timed", e) for e in "afg"] +
         [("mid_timing", e) for e in "ag"] + [("in_flight", e) for e in "abcdefgh"] + [("sample_split", e) for e in "afg"] +
         [("path_slots", e) for e in "beg"] + [("deals", e) for e in "afg"] + [("whitted_heat", e) for e in "aeg"])


def play(run, state, steps):
    for k, (apply, d) in enumerate(steps):
        state.lead(run, k)
        run.edit(apply, d)
        fs, acc = state.after(k, k == len(steps) - 1)
        run.segment(fs, d, acc)
    state.tail(run)
    run.finish()


@pytest.mark.parametrize("state,edit", CASES, ids=[f"{s}-{e}" for s, e in CASES])
def test_edit_under_scheduling_state(rt, oracle, torch, monkeypatch, state, edit):
    assert (rt.MODE_PATH, rt.MODE_WHITTED, rt.MODE_BVH_HEAT) == (PATH, WHITTED, HEAT)
    scene, makers = EDITS[edit]
    d0 = base_scene(rt, scene)
    steps, d = [], d0
    for make in makers:
        apply, d = make(rt, torch, d)
        steps.append((apply, d))
    shared = {"leads": []}
    runs = []
    for control in (False, True):
        st = STATES[state]()
        run = Run(rt, torch, scene_of(rt, monkeypatch, CONTROL if control else st.knobs, d0), control, shared)
        play(run, st, steps)
        runs.append(run)
    test, ctrl = runs
    print(f"{state}-{edit}: lead-ins {shared['leads']}, {len(test.out)} frames, choices {test.r.choices()}, "
          f"frames in flight {test.r.overlap_depth()[0]}, device bytes {test.r.device_bytes()}")
    assert_runs_equal(test, ctrl)
    assert_fresh(rt, oracle, torch, monkeypatch, test, end_work=state == "deals")
    for run in runs:
        run.close()


def test_edit_without_a_reset_keeps_averaging(rt, oracle, torch, monkeypatch):
    """A splice or a material change followed by reset = 0 is a legal call: the accumulator goes on
    averaging.  State 1; three frames, compact_triangles and set_prim_materials, three more frames, no reset
    anywhere: one accumulator ticked three times by the oracle of the old scene and three times by the
    oracle of the new one, and the control."""
    d0 = base_scene(rt, "soup600")
    drop, d1 = edit_drop_half(rt, torch, d0)
    ids = [i for i, p in enumerate(d1.prims) if p.material == 1][:100]
    first = ids[0]
    assert ids == list(range(first, first + 100))
    mirror, d2 = edit_mirror(rt, torch, d1, first, 100)
    before, after = [Frame(frame=j) for j in range(3)], [Frame(frame=j) for j in range(3, 6)]
    runs = []
    for control in (False, True):
        run = Run(rt, torch, scene_of(rt, monkeypatch, CONTROL if control else FORCED, d0), control, {})
        run.frames(before)
        run.reached("order and split", ordered_split())
        run.edit(drop, d1)
        run.edit(mirror, d2)
        run.frames(after)
        run.finish()
        runs.append(run)
    test, ctrl = runs
    assert_runs_equal(test, ctrl)
    W, H = SIZE
    acc = np.zeros((W * H, 4), np.float32)
    want = oracle_frames(oracle_scene(rt, oracle, d0.prims, d0.mats, bvh=d0.host_tree(rt)), before, acc)
    want += oracle_frames(oracle_scene(rt, oracle, d2.prims, d2.mats, bvh=d2.host_tree(rt)), after, acc)
    for i, (rgb, _) in enumerate(want):
        assert np.array_equal(test.host[i], rgb), f"frame {i}: {(test.host[i] != rgb).sum()} pixels differ from the oracle's"
    assert_acc_bits(test.acc[5], want[-1][1])
    for run in runs:
        run.close()
