"""The primary+shadow frame kernel's batched reads: the single-sample build requests
the pixel's accumulator before the rays (only on frames that accumulate in the kernel, only on lanes
that write the pixel) and fetches the hit's shade record and material whole, with NEE's light fields
before the shadow ray.  None of it changes a float operation, so small frames -- 44x20: 6x3 tiles
with off-image lanes on both sides, 40x24: whole tiles -- equal the oracle's ticks bit for bit: RGB8
frame, accumulator, ray counters (the oracle's isect / occl statistics)."""
import numpy as np
import pytest

from scenes_util import oracle_scene
from test_frame_fixed_cost import acc_bits_equal, check_packed, packed_pixels

pytestmark = pytest.mark.gpu

SIZES = [(44, 20), (40, 24)]
# accumulate, reset, accumulate: the early accumulator read, the skipped read, and frames dispatched
# in the measured tile order (costs recorded on the third frame of a parameter set, used from the fourth)
TICKS = [(0, False), (1, False), (2, False), (3, True), (4, False), (5, False), (6, False)]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def teapot_oracle(rt, oracle):
    return oracle.Scene("teapotF", rt.DATA_DIR)


def counters_equal(r, stats, npix, what):
    """shadow rays = the oracle's IsOccluded calls; primary + bounce rays = its IntersectBVH calls."""
    c = r.counters()
    isect, occl = sum(s["isect"] for s in stats), sum(s["occl"] for s in stats)
    assert c["shadow"] == occl == sum(s["shadow"] for s in stats), f"{what}: shadow {c} vs {stats}"
    assert c["primary"] == npix * len(stats) and c["primary"] + c["bounce"] == isect, f"{what}: {c} vs isect {isect}"
    assert occl > 0


def run_ticks(rt, g, o, W, H, ticks, what, depth=1, setup=None):
    """ticks: (frame, reset) per Tick at spp 1; every frame and the accumulator after it, then the counters."""
    r = rt.Renderer(g, W, H)
    if setup:
        setup(r)
    what = f"{what} {W}x{H} depth {depth} [{r.kernel_name(1, depth)}]"
    acc = np.zeros((W * H, 4), np.float32)
    stats = []
    for frame, reset in ticks:
        got = r.tick_host(spp=1, depth=depth, frame=frame, reset=reset)
        if reset:
            acc[:] = 0
        want, st = o.tick(W, H, acc, spp=1, depth=depth, frame=frame)
        stats.append(st)
        assert np.array_equal(got, want), f"{what} frame {frame}: {(got != want).sum()} RGB8 mismatches"
        acc_bits_equal(r.accumulator(), acc, f"{what} frame {frame}")
    counters_equal(r, stats, W * H, what)
    return r


def ntiles(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


@pytest.mark.parametrize("walk", ["0", "1"])   # the lane walk / the wave walk for camera rays, neither timed
@pytest.mark.parametrize("W,H", SIZES)
def test_accumulate_reset_accumulate_in_measured_order(rt, teapot_oracle, torch, monkeypatch, W, H, walk):
    monkeypatch.setenv("RT_WAVE_PRIMARY", walk)
    g = rt.Scene.recipe("teapotF")
    r = run_ticks(rt, g, teapot_oracle, W, H, TICKS, f"walk {walk}")
    assert len(r.tile_costs()) == ntiles(W, H), "the last frames ran in the measured tile order"
    r.close()
    g.close()


@pytest.mark.parametrize("in_flight", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_forced_split_order(rt, teapot_oracle, torch, monkeypatch, W, H, in_flight):
    """The four costliest tiles run as two half-tile waves each: the early read follows the part mask.
    With overlapped frames forced the frame kernel stores samples and reads no accumulator at all;
    the finishing pass accumulates.  (Overlapped frames this small keep the plain build unless the
    single-sample one is asked for: RT_FRAME_WAVES=8.)"""
    monkeypatch.setenv("RT_WAVE_PRIMARY", "0")
    monkeypatch.setenv("RT_SPLIT_HEAVY", "4")
    monkeypatch.setenv("RT_PS_PIPELINE", "1" if in_flight else "0")
    if in_flight:
        monkeypatch.setenv("RT_PS_DEPTH", "2")
        monkeypatch.setenv("RT_FRAME_WAVES", "8")
    g = rt.Scene.recipe("teapotF")
    r = run_ticks(rt, g, teapot_oracle, W, H, TICKS, f"split order, in flight {in_flight}")
    assert len(r.tile_costs()) == ntiles(W, H) and r.choices()["split"] == 1, r.choices()
    assert (r.device_bytes()[1] > 0) == in_flight, "result buffers exist exactly when frames overlap"
    r.close()
    g.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_packed_shards_and_permuted_tile_list(rt, teapot_oracle, torch, W, H):
    """Three frames, each rendered as the interleaved shards 1, 0, 2 of 3 (packed output), then three
    more as two explicit tile lists of a permutation: the accumulator carries over throughout."""
    g, o = rt.Scene.recipe("teapotF"), teapot_oracle
    N, nt = 3, ntiles(W, H)
    perm = np.random.default_rng(11).permutation(nt).astype(np.uint32)
    lists = [perm[:5], perm[5:]]
    r = rt.Renderer(g, W, H)
    bufs = torch.zeros((N, r.shard_capacity(N)), dtype=torch.int32, device="cuda:0")
    buf = torch.zeros(nt * 64, dtype=torch.int32, device="cuda:0")
    acc = np.zeros((W * H, 4), np.float32)
    stats = []
    for f in range(6):
        want, st = o.tick(W, H, acc, spp=1, depth=1, frame=f)
        stats.append(st)
        if f < 3:
            for s in (1, 0, 2):
                r.render_shard(bufs[s], s, N, depth=1, frame=f)
                torch.cuda.synchronize()
                check_packed(bufs[s], packed_pixels(W, H, np.arange(s, nt, N)), want, f"shard {s}/{N} {W}x{H} frame {f}")
        else:
            for k, tiles in enumerate(lists):
                r.render_shard_tiles(buf, tiles, depth=1, frame=f)
                torch.cuda.synchronize()
                check_packed(buf, packed_pixels(W, H, tiles), want, f"tile list {k} {W}x{H} frame {f}")
        acc_bits_equal(r.accumulator(), acc, f"shards / lists {W}x{H} frame {f}")
    counters_equal(r, stats, W * H, f"shards / lists {W}x{H}")
    r.close()
    g.close()


def materials_scene(rt, extension):
    """The light, a glass and a mirror sphere, a diffuse triangle and a small mirror triangle over a
    checkerboard (mix) floor plane, all in the default camera's view; `extension` adds a diffuse cube,
    which takes the scene to the extension kernel build."""
    mats = [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.DIFFUSE, (0.8, 0.3, 0.3)),
            rt.material(rt.MIRROR, (0.9, 0.9, 0.9)), rt.material(rt.DIELECTRIC, (0.2, 0.05, 0.3), ior=1.5),
            rt.material(rt.CHECKERBOARD, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9), diffuse=0.5)]
    prims = [rt.sphere((0.0, 1.6, 3.0), 0.4, 0), rt.plane((0, 1, 0), 1.0, 4), rt.sphere((-1.2, -0.3, 2.5), 0.6, 3),
             rt.sphere((1.2, -0.4, 2.5), 0.55, 2), rt.triangle((-3, -1, 5), (3, -1, 5), (0, 3, 5), 1),
             rt.triangle((-0.4, -0.9, 1.5), (0.4, -0.9, 1.5), (0.0, -0.3, 2.0), 2)]
    if extension:
        prims.append(rt.cube((0.1, 0.2, 2.2), 0.5, 1, rt.mat4_rotate(1, 0.5)))
    return prims, mats


@pytest.mark.parametrize("depth", [1, 3])          # 3: the path tracer, whose level 0 shares the shading code
@pytest.mark.parametrize("extension", [False, True])
def test_every_core_material_in_view(rt, oracle, torch, extension, depth):
    W, H = 44, 20
    prims, mats = materials_scene(rt, extension)
    o = oracle_scene(rt, oracle, prims, mats)
    g = rt.Scene(prims, mats)
    obj = g.IntersectBVH(o.camera_rays(W, H, np.arange(W * H, dtype=np.int32)))[1].cpu().numpy()
    seen = {prims[i].material for i in np.unique(obj[obj >= 0])}
    assert seen == set(range(len(mats))), f"materials in view: {seen}"
    assert (obj < 0).any(), "and some sky"
    if extension:
        assert (obj == len(prims) - 1).any(), "the cube is in view"
    run_ticks(rt, g, o, W, H, TICKS[:5], f"materials, extension {extension}", depth=depth).close()
    g.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_walk_check_build(rt, teapot_oracle, torch, monkeypatch, W, H):
    """k_render_walkcheck shares render_tile (not the single-sample build's pieces): the same ticks."""
    monkeypatch.setenv("RT_WAVE_PRIMARY", "1")
    g = rt.Scene.recipe("teapotF")
    r = run_ticks(rt, g, teapot_oracle, W, H, TICKS, "walk check", setup=lambda r: r.set_walk_check(rt.WALK_CHECK_COUNT))
    ws = r.walk_stats()
    assert 0 < ws["walked"] <= len(TICKS) * W * H and ws["verify_mismatch"] == 0, ws
    r.close()
    g.close()
