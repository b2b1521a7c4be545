"""Every build of the frame kernel and of rt_trace that the host's kernel selection can reach
(csrc/rt_variants.h), in both kernel families -- the core build on the TEAPOT-F recipe, the
extension build on the cube / quad / texture scene of test_gpu_parity -- each under a constant and
under a textured sky: RGB8, accumulator bits and the shadow-ray count against the oracle, and
rt_frame_kernel_name's answer for the frame.  A mis-routed launch (a larger MAXD class, the plain
build where the single-sample one was meant) renders the same frame, so this file pins what every
route computes; tests/test_variants_host.py pins the routes themselves.

40x24 frames: 15 tiles, three full workgroups of four waves and a ragged one of three."""
import numpy as np
import pytest

from scenes_util import oracle_scene
from test_gpu_parity import assert_acc_bits, shapes_scene
from test_gpu_trace import check_trace, trace_rays

pytestmark = pytest.mark.gpu

W, H = 40, 24
PATH, WHITTED, PACKET = 0, 1, 2
ONE_KERNEL = {"RT_PT_WAVEFRONT": "0"}   # path-traced frames in the k_render builds, not the wavefront's

# id: mode, depth, spp, environment at scene creation, walk check (None: the walk is not forced), kernel name
FRAMES = {
    "path1-single-sample": (PATH, 1, 1, {}, None, "k_render<path,1>"),
    "path1-plain": (PATH, 1, 1, {"RT_FRAME_WAVES": "7"}, None, "k_render<path,1>"),
    "path1-spp2": (PATH, 1, 2, {}, None, "k_render<path,1>"),
    "path1-walk-count": (PATH, 1, 1, {}, "WALK_CHECK_COUNT", "k_render<path,1>"),
    "path1-walk-verify": (PATH, 1, 1, {}, "WALK_CHECK_VERIFY", "k_render<path,1>"),
    "path3": (PATH, 3, 1, ONE_KERNEL, None, "k_render<path,4>"),
    "path7": (PATH, 7, 1, ONE_KERNEL, None, "k_render<path,10>"),
    "path20": (PATH, 20, 1, ONE_KERNEL, None, "k_render<path,32>"),
    "whitted5": (WHITTED, 5, 1, {}, None, "k_render<whitted,1>"),
    "packet0": (PACKET, 0, 1, {}, None, "k_render<packet,1>"),
    "packet1": (PACKET, 1, 1, {}, None, "k_render<packet,1>"),
    "packet3": (PACKET, 3, 1, {}, None, "k_render<packet,10>"),
    "packet7": (PACKET, 7, 1, {}, None, "k_render<packet,10>"),
    "packet20": (PACKET, 20, 1, {}, None, "k_render<packet,32>"),
}
FAMILIES = ["core", "ext"]
SKIES = ["const", "tex"]
# the wave walk (and so its check build) is the core family's: cubes rule it out
FRAME_CASES = [(fam, sky, f) for fam in FAMILIES for sky in SKIES for f in FRAMES
               if fam == "core" or FRAMES[f][4] is None]
TRACES = [(PATH, 1), (PATH, 3), (PATH, 7), (PATH, 20), (WHITTED, 5)]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def worlds(rt, oracle, torch):
    """(family, sky) -> (make, oracle scene): make() builds the device scene under the environment
    of the moment, the oracle scene is built once; oracle frames are computed once per
    (family, sky, mode, depth, spp) and handed out as copies."""
    sky = np.random.default_rng(17).integers(0, 1 << 24, size=(32, 64), dtype=np.uint32)
    made, frames = {}, {}

    def world(fam, sk):
        if (fam, sk) not in made:
            s = sky if sk == "tex" else None
            if fam == "core":
                prims, mats = rt.recipe_describe("teapotF")
                o = oracle_scene(rt, oracle, prims, mats, sky=s)
                made[fam, sk] = (lambda: rt.Scene(prims, mats, sky=s)), o
            else:
                with_sky = lambda rt_, oracle_, prims, mats, textures: (prims, mats, textures)
                prims, mats, tex = shapes_scene(rt, oracle, make=with_sky)
                o = oracle_scene(rt, oracle, prims, mats, sky=s, textures=tex)
                made[fam, sk] = (lambda: rt.Scene(prims, mats, sky=s, textures=tex)), o
        return made[fam, sk]

    def oracle_frame(fam, sk, mode, depth, spp):
        key = (fam, sk, mode, depth, spp)
        if key not in frames:
            o = world(fam, sk)[1]
            o.set_integrator(mode)
            acc = np.zeros((W * H, 4), np.float32)
            want, st = o.tick(W, H, acc, spp=spp, depth=depth, frame=0)
            o.set_integrator(PATH)
            frames[key] = (want, acc, st)
        want, acc, st = frames[key]
        return want.copy(), acc.copy(), dict(st)

    return world, oracle_frame


@pytest.mark.parametrize("fam,sky,frame", FRAME_CASES)
def test_frame_variant_against_oracle(rt, worlds, monkeypatch, fam, sky, frame):
    mode, depth, spp, env, check, name = FRAMES[frame]
    world, oracle_frame = worlds
    for k in ("RT_FRAME_WAVES", "RT_PT_WAVEFRONT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = world(fam, sky)[0]()
    if check is not None:
        g.set_camera_walk(rt.WALK_WAVE)
    r = rt.Renderer(g, W, H)
    r.mode = mode
    if check is not None:
        r.set_walk_check(getattr(rt, check))
    assert r.kernel_name(spp=spp, depth=depth) == name
    got = r.tick_host(spp=spp, depth=depth, frame=0)
    want, acc, st = oracle_frame(fam, sky, mode, depth, spp)
    assert np.array_equal(got, want), f"{(got != want).sum()} RGB8 mismatches"
    assert_acc_bits(np.ascontiguousarray(r.accumulator(), np.float32).reshape(-1, 4), acc)
    c = r.counters()
    assert c["shadow"] == st["shadow"], (c, st)
    if check is not None:   # the check build ran: the walk's counters moved, no walked lane differed
        ws = r.walk_stats()
        assert 0 < ws["walked"] <= W * H and ws["verify_mismatch"] == 0, ws
    r.close()
    g.close()


@pytest.mark.parametrize("mode,depth", TRACES)
@pytest.mark.parametrize("sky", SKIES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_trace_variant_against_oracle(rt, worlds, fam, sky, mode, depth):
    make, o = worlds[0](fam, sky)
    g = make()
    rays, seeds, flags = trace_rays(o, W, H, n_random=200)   # 138 camera rays + 200 random ones
    check_trace(g, o, rays, seeds, flags, depth, mode)
    g.close()
