"""The first-hit G-buffer (rt_render_gbuffer, rt_gbuffer_pixels) on the GPU, bit for bit.

Reference, per pixel of a frame (oracle frame index sample + spp * frame, the seed of that sample):
  ray      or_camera_rays                       7 floats
  hit      or_primary_hits                      obj equal, t / u / v bits equal
  normal   tests/gbuffer_model.py on the oracle's hits; material = the description's
  albedo   solid kinds: the material table's bits (a Dielectric: 1, 1, 1); Checkerboard / Texture: the
           model; sky and light pixels: or_trace_rays at depth 1 on the oracle's rays (lastSpecular set:
           Trace returns skyColor(D) / the light's colour there and draws nothing)
Frames are 44x20 (6x3 tiles, off-image lanes on both sides) and 40x24 (whole tiles).  Scene A: recipe
teapotF (the core build); B: the animated room at 0.3 (quad light, cube: the extension build); C: a
Checkerboard plane, a TextureMaterial cube, a Dielectric sphere, a Mirror triangle under a 64x32
non-constant sky.  Each reference is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_model as gm
from anim_util import room_mats, room_prims
from scenes_util import _cam, grazing_cameras, oracle_scene

pytestmark = pytest.mark.gpu

SIZES = [(44, 20), (40, 24)]
PARAMS = [(1, 0, 0), (1, 0, 3), (4, 2, 1)]          # (spp, sample, frame)
ALL = ("ray", "hit", "normal", "albedo")
f32 = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---------------------------------------------------------------- scenes (descriptions need no GPU)
def scene_c(rt):
    """prims, mats, sky [32, 64], textures"""
    rng = np.random.default_rng(5)
    sky = rng.integers(0, 1 << 24, (32, 64)).astype(np.uint32)
    tex = rng.integers(0, 1 << 24, (4, 8)).astype(np.uint32)
    mats = [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.CHECKERBOARD, (0.9, 0.1, 0.2), (0.05, 0.3, 0.7)),
            rt.material(rt.TEXTURE, (1, 1, 1), texture=0), rt.material(rt.DIELECTRIC, (0.2, 0.4, 0.1), ior=1.5),
            rt.material(rt.MIRROR, (0.9, 0.8, 0.7))]
    T = rt.mat4_mul(rt.mat4_rotate(1, 0.6), rt.mat4_rotate(0, 0.3))
    prims = [rt.sphere((0.0, 1.1, 2.0), 0.35, 0), rt.plane((0, 1, 0), 1.0, 1), rt.cube((-1.2, -0.3, 1.9), 1.2, 2, T),
             rt.sphere((1.1, -0.4, 1.6), 0.55, 3), rt.triangle((-0.9, -0.5, 3.0), (1.0, -0.4, 2.9), (0.1, 1.0, 3.1), 4)]
    return prims, mats, sky, [tex]


def description(rt, name):
    """(prims, mats, sky, textures) of scene A / B / C"""
    if name == "A":
        prims, mats = rt.recipe_describe("teapotF")
        return prims, mats, None, []
    if name == "B":
        return room_prims(rt, 0.3), room_mats(rt), None, []
    return scene_c(rt)


# what each scene must show in every frame tested, so that no class passes by being absent
CLASSES = {"A": ("sky", "checkerboard", "solid"), "B": ("light", "solid", "cube"),
           "C": ("sky", "light", "checkerboard", "texture", "dielectric", "solid", "cube")}


class Case:
    """A scene on the GPU, in the oracle, and as its description"""

    def __init__(self, rt, oracle, name, prims=None, bvh=None):
        self.name = name
        d_prims, self.mats, self.sky, self.textures = description(rt, name)
        self.prims = d_prims if prims is None else prims
        if name == "A" and prims is None:
            self.g, self.o = rt.Scene.recipe("teapotF"), oracle.Scene("teapotF", rt.DATA_DIR)
        else:
            self.g = rt.Scene(self.prims, self.mats, sky=self.sky, textures=self.textures, bvh=bvh)
            self.o = oracle_scene(rt, oracle, self.prims, self.mats, sky=self.sky, textures=self.textures, bvh=bvh)
        self.refs = {}

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def cases(rt, oracle, torch):
    out = {n: Case(rt, oracle, n) for n in "ABC"}
    yield out
    for c in out.values():
        c.close()


# ---------------------------------------------------------------- the reference
def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def reference(rt, case, W, H, spp=1, sample=0, frame=0, cam=None, camkey="default"):
    """The four planes of the whole frame as uint32 bit arrays [W*H, k], from the oracle and the model,
    and the pixel classes; cached per case."""
    key = (W, H, spp, sample, frame, camkey)
    if key in case.refs:
        return case.refs[key]
    o, n = case.o, W * H
    fprime = sample + spp * frame
    px = np.arange(n, dtype=np.int32)
    c = o.camera_from(W, H, rt.Camera.default(W, H) if cam is None else cam)
    rays = np.empty((n, 7), f32)
    o.L.or_camera_rays(C.byref(c), W, H, fprime, _p(px, C.c_int32), n, _p(rays, C.c_float))
    t, obj, u, v = np.empty(n, f32), np.empty(n, np.int32), np.empty(n, f32), np.empty(n, f32)
    o.L.or_primary_hits(o.h, C.byref(c), W, H, fprime, _p(px, C.c_int32), n, _p(t, C.c_float), _p(obj, C.c_int32),
                        _p(u, C.c_float), _p(v, C.c_float))
    hit = obj >= 0
    pmat = np.array([p.material for p in case.prims], np.int32)
    ptype = np.array([p.type for p in case.prims], np.int32)
    mkind = np.array([m.kind for m in case.mats], np.int32)
    material = np.where(hit, pmat[np.maximum(obj, 0)], -1).astype(np.int32)
    kind = np.where(hit, mkind[np.maximum(material, 0)], -1).astype(np.int32)
    # normals: the model on the oracle's hits
    N = np.zeros((n, 3), f32)
    N[hit] = gm.normals(case.prims, obj[hit], rays[hit, 0:3], rays[hit, 3:6], t[hit])
    # albedo
    trace, _, _ = o.trace_rays(rays, np.ones(n, np.uint32), depth=1, flags=np.ones(n, np.uint8))
    I = gm.hit_point(rays[:, 0:3], rays[:, 3:6], t)
    rgb = np.zeros((n, 3), f32)
    cls = np.full(n, "", dtype=object)
    for i in np.unique(material):
        m = material == i
        if i < 0:
            rgb[m], cls[m] = trace[m], "sky"
            continue
        mat = case.mats[int(i)]
        if mat.kind == rt.LIGHT:
            rgb[m], cls[m] = trace[m], "light"
        elif mat.kind == rt.DIELECTRIC:
            rgb[m], cls[m] = f32([1, 1, 1]), "dielectric"
        elif mat.kind == rt.CHECKERBOARD:
            rgb[m], cls[m] = gm.checkerboard_color(I[m], list(mat.color), list(mat.color2)), "checkerboard"
        elif mat.kind == rt.TEXTURE:
            rgb[m], cls[m] = gm.texture_color(case.textures[mat.texture], u[m], v[m]), "texture"
        else:
            rgb[m], cls[m] = f32(list(mat.color)), "solid"
    is_cube = hit & (ptype[np.maximum(obj, 0)] == rt.CUBE)
    ref = {"ray": rays.view(np.uint32),
           "hit": np.stack([t.view(np.uint32), obj.view(np.uint32), u.view(np.uint32), v.view(np.uint32)], 1),
           "normal": np.concatenate([N.view(np.uint32), material.view(np.uint32)[:, None]], 1),
           "albedo": np.concatenate([rgb.view(np.uint32), kind.view(np.uint32)[:, None]], 1),
           "class": cls, "cube": is_cube, "hitmask": hit}
    case.refs[key] = ref
    return ref


def classes_present(ref):
    out = set(np.unique(ref["class"]).tolist())
    if ref["cube"].any():
        out.add("cube")
    return out


def bits(planes):
    """{plane: torch tensor [..., k]} -> {plane: uint32 [n, k]}"""
    return {k: np.ascontiguousarray(t.cpu().numpy()).view(np.uint32).reshape(-1, t.shape[-1]) for k, t in planes.items()}


def host_bits(planes):
    """{plane: structured array} -> {plane: uint32 [n, k]}"""
    return {k: np.ascontiguousarray(a).reshape(-1).view(np.uint32).reshape(a.size, -1) for k, a in planes.items()}


def assert_planes(got, ref, what, rows=None, names=ALL):
    """hit: u, v of a sky pixel are not compared beyond what the oracle leaves (0, 0 on both sides)"""
    for k in names:
        want = ref[k] if rows is None else ref[k][rows]
        bad = np.nonzero((got[k] != want).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: plane {k}: {len(bad)} of {len(want)} pixels differ, first at {bad[:4].tolist()}: " \
                              f"{got[k][bad[0]].tolist()} != {want[bad[0]].tolist()}"


def crop(W, x0, y0, w, h):
    """row-major pixel indices of a rectangle"""
    return ((y0 + np.arange(h))[:, None] * W + x0 + np.arange(w)[None, :]).reshape(-1)


# ---------------------------------------------------------------- 1. rays and hits, 3. normals and albedo
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", list("ABC"))
def test_all_planes_equal_the_oracle_and_the_model(rt, cases, name, W, H):
    case = cases[name]
    r = rt.Renderer(case.g, W, H)
    for spp, sample, frame in PARAMS:
        ref = reference(rt, case, W, H, spp, sample, frame)
        got = bits(r.gbuffer(ALL, sample=sample, spp=spp, frame=frame))
        counts = {c: int((ref["class"] == c).sum()) for c in classes_present(ref) - {"cube"}}
        print(name, W, H, spp, sample, frame, counts, "cube", int(ref["cube"].sum()))
        assert_planes(got, ref, f"scene {name} {W}x{H} spp {spp} sample {sample} frame {frame}")
        missing = set(CLASSES[name]) - classes_present(ref)
        assert not missing, f"scene {name} {W}x{H} frame {frame}: no pixel of class {sorted(missing)}"
    assert r.frame == 0
    r.close()


@pytest.mark.parametrize("name", list("ABC"))
def test_moved_camera(rt, cases, name):
    W, H = 44, 20
    case = cases[name]
    cam = _cam(rt, W, H, (0.4, 0.3, -1.2), (-0.1, -0.05, 0.99), (0.99, 0.0, 0.1), (0.0, 1.0, 0.05))
    r = rt.Renderer(case.g, W, H)
    r.camera = cam
    ref = reference(rt, case, W, H, 4, 2, 1, cam=cam, camkey="moved")
    assert_planes(bits(r.gbuffer(ALL, sample=2, spp=4, frame=1)), ref, f"scene {name} moved camera")
    r.close()


def test_core_build_light_pixels(rt, cases):
    """TEAPOT-F's light sphere is out of the default camera's view: a camera below it, looking up at it"""
    W, H = 40, 24
    case = cases["A"]
    c = [float(x) for x in list(case.prims[0].v)[:3]]
    cam = _cam(rt, W, H, (c[0], c[1] - 3.0, c[2]), (0, 1, 0), (1, 0, 0), (0, 0, 1))
    r = rt.Renderer(case.g, W, H)
    r.camera = cam
    ref = reference(rt, case, W, H, cam=cam, camkey="light")
    assert (ref["class"] == "light").sum() >= 8 and (ref["class"] == "sky").sum() >= 8
    assert_planes(bits(r.gbuffer(ALL)), ref, "scene A looking at its light")
    r.close()


# ---------------------------------------------------------------- 2. both walks
def test_lane_and_wave_walk_give_the_same_planes(rt, oracle, cases):
    case = cases["A"]
    g = rt.Scene.recipe("teapotF")
    frames = [(W, H, None, "default") for W, H in SIZES]
    name, cam = grazing_cameras(rt, 44, 20)["teapotF_floor_skim"]
    assert name == "teapotF"
    frames.append((44, 20, cam, "floor_skim"))
    for W, H, cam, camkey in frames:
        ref = reference(rt, case, W, H, cam=cam, camkey=camkey)
        r = rt.Renderer(g, W, H)
        if cam is not None:
            r.camera = cam
        got = {}
        stack = 4 * 256 * rt_stack_entries(rt, g)         # the lane stacks: entries x 256 lanes x 4 B
        for walk in (rt.WALK_LANE, rt.WALK_WAVE):
            g.set_camera_walk(walk)
            # what the launch is made with, read where the launch reads it: the wave walk and its word stack
            # (4 waves x stack entries x 4 B past the lane stacks) under WAVE only, and never for a list
            info, linfo = r.gbuffer_walk(), r.gbuffer_walk(pixels=True)
            assert info["wave"] == (walk == rt.WALK_WAVE) and not linfo["wave"], (walk, info, linfo)
            assert linfo["lds_bytes"] == stack and info["lds_bytes"] == stack + (stack // 64 if walk == rt.WALK_WAVE else 0), (info, linfo, stack)
            got[walk] = bits(r.gbuffer(ALL))
            assert_planes(got[walk], ref, f"walk {walk} {W}x{H} {camkey}")
            ws = r.walk_stats()
            assert ws["walked"] == 0 and ws["retraced"] == 0, ws      # the query counts nothing
        for k in ALL:
            assert np.array_equal(got[rt.WALK_LANE][k], got[rt.WALK_WAVE][k])
        r.close()
    g.close()


def rt_stack_entries(rt, g):
    """LDS stack entries per lane of a scene's launches, from the one launch whose LDS is its lane stacks
    alone: the list form's"""
    r = rt.Renderer(g, 8, 8)
    n = r.gbuffer_walk(pixels=True)["lds_bytes"] // (4 * 256)
    r.close()
    assert n >= g.info["depth"] > 0
    return n


def test_auto_walk_follows_what_the_frames_settled_on(rt, cases):
    """RT_WALK_AUTO (TEAPOT-F's default): the lane walk while the renderer's frames have settled nothing, then
    whatever they settle on; the query itself settles nothing, however often it runs."""
    W, H = 40, 24
    g = rt.Scene.recipe("teapotF")
    r = rt.Renderer(g, W, H)
    ref = reference(rt, cases["A"], W, H)
    assert r.choices()["walk"] == -1 and not r.gbuffer_walk()["wave"]
    for _ in range(40):
        r.gbuffer(("hit",))
    assert r.choices()["walk"] == -1 and not r.gbuffer_walk()["wave"]
    for k in range(64):                                 # 1 warm-up + 4 groups of 4 timed frames, and restarts
        r.Tick(depth=1)
        if r.choices()["walk"] >= 0:
            break
    settled = r.choices()["walk"]
    assert settled in (0, 1), r.choices()
    assert r.gbuffer_walk()["wave"] == (settled == 1) and not r.gbuffer_walk(pixels=True)["wave"]
    assert_planes(bits(r.gbuffer(ALL, frame=0)), ref, f"AUTO settled on walk {settled}")   # (r.frame has moved on)
    r.close()
    g.close()


def test_cube_scene_refuses_the_wave_walk_and_takes_the_lane_walk(rt, cases):
    case = cases["B"]
    with pytest.raises(rt.RTError) as e:
        case.g.set_camera_walk(rt.WALK_WAVE)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED
    W, H = 44, 20
    r = rt.Renderer(case.g, W, H)
    assert not r.gbuffer_walk()["wave"]
    assert_planes(bits(r.gbuffer(ALL)), reference(rt, case, W, H), "scene B after the refused walk")
    r.close()


# ---------------------------------------------------------------- 4. rectangles
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["A", "C"])
def test_rectangles_equal_the_crop_and_leave_a_guard_band(rt, torch, cases, name, W, H):
    case = cases[name]
    ref = reference(rt, case, W, H)
    r = rt.Renderer(case.g, W, H)
    L, guard = rt.lib(), 64
    for rect in [(5, 3, 17, 9), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W - 3, 0, 1, H), (0, H - 1, W, 1), (8, 8, 8, 8)]:
        x0, y0, w, h = rect
        rows = crop(W, *rect)
        assert_planes(bits(r.gbuffer(ALL, rect=rect)), ref, f"scene {name} {W}x{H} rect {rect}", rows=rows)
        # straight through the C ABI into buffers with a band of 0xA5 bytes on both sides of each plane
        bufs, g = {}, rt.GBuffer()
        for k, words in (("ray", 7), ("hit", 4), ("normal", 4), ("albedo", 4)):
            bufs[k] = torch.full((guard + w * h * words + guard,), -1515870811, dtype=torch.int32, device="cuda:0")   # 0xA5A5A5A5
            setattr(g, k, bufs[k].data_ptr() + 4 * guard)
        p = rt.FrameParams(W, H, 1, 1, 0, rt.MODE_PATH, 0)
        rc = L.rt_render_gbuffer(r.h, C.byref(r.camera), C.byref(p), 0, x0, y0, w, h, C.byref(g),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == rt.RT_OK, L.rt_last_error()
        for k, b in bufs.items():
            a = b.cpu().numpy().view(np.uint32)
            assert (a[:guard] == 0xA5A5A5A5).all() and (a[-guard:] == 0xA5A5A5A5).all(), f"rect {rect}: plane {k} wrote outside"
            assert np.array_equal(a[guard:-guard].reshape(w * h, -1), ref[k][rows]), f"rect {rect}: plane {k}"
    r.close()


# ---------------------------------------------------------------- 5. pixel lists
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pixel_lists(rt, torch, cases, name, W, H):
    case = cases[name]
    ref = reference(rt, case, W, H, 4, 2, 1)
    r = rt.Renderer(case.g, W, H)
    rng = np.random.default_rng(W)
    px = rng.integers(0, W * H, 200)
    px[150:] = px[:50]                               # duplicates
    px = rng.permutation(px)
    kw = dict(sample=2, spp=4, frame=1)
    assert_planes(bits(r.pick(px, ALL, **kw)), ref, f"scene {name} {W}x{H} list", rows=px)
    assert_planes(bits(r.pick(torch.from_numpy(px.astype(np.int32)).cuda(), ALL, **kw)), ref, "a device list", rows=px)
    assert_planes(host_bits(r.pick_host(px, ALL, **kw)), ref, "the _host form", rows=px)
    xy = np.stack([px % W, px // W], 1)
    assert_planes(bits(r.pick(xy, ("hit",), **kw)), ref, "(x, y) pairs", rows=px, names=("hit",))
    # n = 1 through the C ABI's _host form equals Renderer.pick_host
    one = np.array([px[7]], np.uint32)
    hit = np.zeros(1, rt.HIT_DTYPE)
    p = rt.FrameParams(W, H, 4, 1, 1, rt.MODE_PATH, 0)
    g = rt.GBuffer(hit=hit.ctypes.data)
    assert rt.lib().rt_gbuffer_pixels_host(r.h, C.byref(r.camera), C.byref(p), 2, one.ctypes.data_as(C.c_void_p), 1, C.byref(g)) == rt.RT_OK
    assert hit.tobytes() == r.pick_host(one, **kw)["hit"].tobytes()
    assert np.array_equal(hit.view(np.uint32).reshape(1, 4), ref["hit"][one])
    # a device list is read on the GPU only: an index outside the frame leaves its list position of every
    # plane as it was, and its neighbours are written
    lst = px[:9].astype(np.int64)
    lst[[0, 4, 8]] = [W * H, 0xffffffff, W * H + 12345]
    good = np.array([1, 2, 3, 5, 6, 7])
    dlist = torch.from_numpy(lst.astype(np.uint32).view(np.int32)).cuda()
    bufs, gb = {}, rt.GBuffer()
    for k, words in (("ray", 7), ("hit", 4), ("normal", 4), ("albedo", 4)):
        bufs[k] = torch.full((9, words), -1515870811, dtype=torch.int32, device="cuda:0")   # 0xA5A5A5A5
        setattr(gb, k, bufs[k].data_ptr())
    assert rt.lib().rt_gbuffer_pixels(r.h, C.byref(r.camera), C.byref(p), 2, C.c_void_p(dlist.data_ptr()), 9, C.byref(gb),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)) == rt.RT_OK
    for k, b in bufs.items():
        a = b.cpu().numpy().view(np.uint32)
        assert (a[[0, 4, 8]] == 0xA5A5A5A5).all(), f"plane {k}: a position with an index outside the frame was written"
        assert np.array_equal(a[good], ref[k][lst[good]]), f"plane {k}: the neighbours of a bad index"
    # an empty list: RT_OK, nothing launched, empty planes
    assert r.pick([], ALL)["hit"].shape == (0, 4) and r.pick_host([])["hit"].shape == (0,)
    r.close()


# ---------------------------------------------------------------- 6. plane subsets
@pytest.mark.parametrize("name", ["A", "C"])
def test_plane_subsets(rt, cases, name):
    W, H = 44, 20
    case = cases[name]
    ref = reference(rt, case, W, H)
    r = rt.Renderer(case.g, W, H)
    for subset in [("ray",), ("hit",), ("normal",), ("albedo",), ("hit", "albedo")]:
        got = r.gbuffer(subset)
        assert tuple(got) == subset
        assert_planes(bits(got), ref, f"scene {name} planes {subset}", names=subset)
        assert_planes(host_bits(r.gbuffer_host(subset, rect=(5, 3, 17, 9))), ref, f"host planes {subset}", rows=crop(W, 5, 3, 17, 9),
                      names=subset)
        assert_planes(bits(r.pick(np.arange(W * H), subset)), ref, f"list planes {subset}", names=subset)
    r.close()


# ---------------------------------------------------------------- 7. no side effects
def test_queries_change_no_frame_state(rt, cases):
    """Frames 0-2 at depth 1 and one at depth 4 in two renderers, the second with G-buffer and pick calls
    between every two frames: same RGB8 frames, accumulator bits, counters, choices and walk statistics;
    and around each query the second renderer's own counters, choices and statistics stand still."""
    W, H = 44, 20
    g = cases["A"].g

    def state(r):
        return r.counters(), r.choices(), r.walk_stats()

    def queries(r):
        before = state(r)
        r.gbuffer(ALL)
        r.gbuffer_host(("hit",), rect=(5, 3, 17, 9), sample=1, spp=2)
        r.pick([0, 17, W * H - 1])
        r.pick_host([[3, 4]], ALL)
        assert state(r) == before and r.frame == before[0]["frames"]

    a, b = rt.Renderer(g, W, H), rt.Renderer(g, W, H)
    queries(b)
    for depth, frames in ((1, 3), (4, 1)):
        for _ in range(frames):
            fa, fb = a.tick_host(depth=depth), b.tick_host(depth=depth)
            queries(b)
            assert np.array_equal(fa, fb)
            assert a.accumulator().tobytes() == b.accumulator().tobytes()
            assert state(a) == state(b)
    assert a.frame == b.frame == 4 and a.counters()["frames"] == 4
    a.close()
    b.close()


# ---------------------------------------------------------------- 8. behind stream-ordered updates
def test_gbuffer_runs_behind_an_async_update(rt, oracle, torch):
    """update_prims(wait=False) to time 0.8, then gbuffer on the same stream with no synchronise.  An
    in-place update keeps the tree's topology and refits its boxes, so the reference is the
    oracle holding the 0.8 description over the host-refitted tree, as tests/test_update_prims_gpu.py
    holds every updated scene."""
    W, H = 44, 20
    base, new = room_prims(rt, 0.3), room_prims(rt, 0.8)
    moved = base[:1] + new[1:4] + base[4:]                       # the light stays: its fields are the host's
    nodes, idx = rt.build_bvh_host(base)[:2]
    before = Case(rt, oracle, "B", prims=base, bvh=(nodes, idx))
    after = Case(rt, oracle, "B", prims=moved, bvh=(rt.refit_bvh_host(moved, nodes, idx), idx))
    g = before.g
    r = rt.Renderer(g, W, H)
    rec, T = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in rt.pack_prims(new[1:4]))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    # the raw stream handle alone, torch's current stream left as it is: the queries allocate and upload on `st`
    first = r.gbuffer(ALL, stream=st.cuda_stream)
    assert g.update_prims(1, (rec, T), stream=st.cuda_stream, wait=False) == 1
    second = r.gbuffer(ALL, stream=st.cuda_stream)
    picked = r.pick(np.arange(W * H), ALL, stream=st.cuda_stream)
    assert torch.cuda.current_stream() != st
    status = g.update_sync()
    st.synchronize()
    assert (status["submitted"], status["applied"], status["refused"]) == (1, 1, 0), status
    ref0, ref1 = reference(rt, before, W, H), reference(rt, after, W, H)
    assert not np.array_equal(ref0["hit"], ref1["hit"])
    assert_planes(bits(first), ref0, "before the update")
    assert_planes(bits(second), ref1, "behind the update")
    assert_planes(bits(picked), ref1, "the list form behind the update")
    r.close()
    before.close()
    after.close()


# ---------------------------------------------------------------- 9. refusals on the device
def test_refusals_with_a_renderer(rt, torch, cases):
    W, H = 44, 20
    r = rt.Renderer(cases["A"].g, W, H)
    L = rt.lib()
    before = r.counters()

    def refused(fn, text):
        with pytest.raises(rt.RTError) as e:
            fn()
        assert e.value.code == rt.RT_ERR_INVALID and text in str(e.value), str(e.value)

    refused(lambda: r.gbuffer(sample=1), "sample outside")
    refused(lambda: r.gbuffer(sample=4, spp=4), "sample outside")
    refused(lambda: r.gbuffer(sample=1, spp=0), "sample outside")
    refused(lambda: r.gbuffer(rect=(0, 0, 0, 4)), "empty rectangle")
    refused(lambda: r.gbuffer(rect=(0, 0, W, 0)), "empty rectangle")
    refused(lambda: r.gbuffer(rect=(1, 0, W, H)), "leaves the frame")
    refused(lambda: r.gbuffer(rect=(0, H, 1, 1)), "leaves the frame")
    refused(lambda: r.gbuffer_host(rect=(W - 2, H - 2, 3, 2)), "leaves the frame")
    refused(lambda: r.pick_host([W * H]), "outside the frame")
    refused(lambda: r.pick([W * H]), "outside the frame")
    # a frame size that is not the renderer's, and no plane at all: through the C ABI
    hit = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda:0")
    one = rt.GBuffer(hit=hit.data_ptr())
    host_hit = np.zeros(W * H, rt.HIT_DTYPE)
    host_one = rt.GBuffer(hit=host_hit.ctypes.data)
    px = np.zeros(1, np.uint32)
    dpx = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    for p in (rt.FrameParams(W + 4, H, 1, 1, 0, 0, 0), rt.FrameParams(W, H - 4, 1, 1, 0, 0, 0)):
        w, h = min(p.width, W), min(p.height, H)
        calls = [lambda: L.rt_render_gbuffer(r.h, C.byref(r.camera), C.byref(p), 0, 0, 0, w, h, C.byref(one), None),
                 lambda: L.rt_render_gbuffer_host(r.h, C.byref(r.camera), C.byref(p), 0, 0, 0, w, h, C.byref(host_one)),
                 lambda: L.rt_gbuffer_pixels(r.h, C.byref(r.camera), C.byref(p), 0, C.c_void_p(dpx.data_ptr()), 1, C.byref(one), None),
                 lambda: L.rt_gbuffer_pixels_host(r.h, C.byref(r.camera), C.byref(p), 0, px.ctypes.data_as(C.c_void_p), 1, C.byref(host_one))]
        for call in calls:
            assert call() == rt.RT_ERR_INVALID and b"frame size differs" in L.rt_last_error()
    p = rt.FrameParams(W, H, 1, 1, 0, 0, 0)
    none = rt.GBuffer()
    assert L.rt_render_gbuffer(r.h, C.byref(r.camera), C.byref(p), 0, 0, 0, W, H, C.byref(none), None) == rt.RT_ERR_INVALID
    assert L.rt_gbuffer_pixels(r.h, C.byref(r.camera), C.byref(p), 0, C.c_void_p(dpx.data_ptr()), 1, C.byref(none), None) == rt.RT_ERR_INVALID
    assert L.rt_gbuffer_pixels(r.h, C.byref(r.camera), C.byref(p), 0, None, 1, C.byref(one), None) == rt.RT_ERR_INVALID
    assert L.rt_gbuffer_pixels(r.h, C.byref(r.camera), C.byref(p), 0, None, 0, C.byref(one), None) == rt.RT_OK   # n = 0
    bad = np.array([0, W * H], np.uint32)
    assert L.rt_gbuffer_pixels_host(r.h, C.byref(r.camera), C.byref(p), 0, bad.ctypes.data_as(C.c_void_p), 2,
                                    C.byref(host_one)) == rt.RT_ERR_INVALID and b"pixel 1 lies outside the frame" in L.rt_last_error()
    torch.cuda.synchronize()
    assert float(hit.abs().sum()) == 0.0 and not host_hit.view(np.uint32).any(), "a refused call wrote a plane"
    assert r.counters() == before
    r.close()
