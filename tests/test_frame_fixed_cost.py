"""The primary+shadow frame kernel's fixed cost per wave: the single-sample build
reads its argument records in place and counts its shadow rays by ballot; the other builds of
render_tile (sample loop, sample split, walk check) keep the summed counter.  Small frames whose
edge tiles carry off-image lanes (44x20: 6x3 tiles, neither side a multiple of 8; 40x24: whole
tiles), against the oracle's tick bit for bit: RGB8 frame, accumulator, ray counters (the
oracle's isect / occl statistics)."""
import numpy as np
import pytest

from scenes_util import oracle_scene

pytestmark = pytest.mark.gpu

SIZES = [(44, 20), (40, 24)]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def teapot(rt, oracle, torch):
    return rt.Scene.recipe("teapotF"), oracle.Scene("teapotF", rt.DATA_DIR)


def acc_bits_equal(gacc, acc, what):
    g, w = gacc.view(np.uint32), acc.view(np.uint32)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} accumulator pixels differ, first {bad[:3].tolist()}: " \
                          f"{gacc[bad[0]].tolist()} vs {acc[bad[0]].tolist()}"


def counters_equal(r, stats, what):
    """primary + bounce rays = the oracle's IntersectBVH calls, shadow rays = its IsOccluded calls."""
    c = r.counters()
    isect, occl = sum(s["isect"] for s in stats), sum(s["occl"] for s in stats)
    assert c["shadow"] == occl == sum(s["shadow"] for s in stats), f"{what}: shadow {c} vs {stats}"
    assert c["bounce"] == 0 and c["primary"] == isect, f"{what}: {c} vs isect {isect}"
    assert occl > 0


def run_ticks(rt, g, o, W, H, spp, ticks, what, setup=None):
    """ticks: (frame, reset) per Tick; each frame, the accumulator after each and the counters."""
    r = rt.Renderer(g, W, H)
    if setup:
        setup(r)
    what = f"{what} {W}x{H} spp {spp} [{r.kernel_name(spp, 1)}]"
    acc = np.zeros((W * H, 4), np.float32)
    stats = []
    for frame, reset in ticks:
        got = r.tick_host(spp=spp, depth=1, frame=frame, reset=reset)
        if reset:
            acc[:] = 0
        want, st = o.tick(W, H, acc, spp=spp, depth=1, frame=frame)
        stats.append(st)
        assert np.array_equal(got, want), f"{what} frame {frame}: {(got != want).sum()} RGB8 mismatches"
        acc_bits_equal(r.accumulator(), acc, f"{what} frame {frame}")
    counters_equal(r, stats, what)
    return r


@pytest.mark.parametrize("W,H", SIZES)
def test_single_sample_frames_and_reset(rt, teapot, W, H):
    g, o = teapot
    run_ticks(rt, g, o, W, H, 1, [(0, False), (1, False), (2, True)], "Tick").close()


@pytest.mark.parametrize("spp", [2, 8])   # the plain build's sample loop; the sample split where the renderer picks it
@pytest.mark.parametrize("W,H", SIZES)
def test_multi_sample_frames(rt, teapot, W, H, spp):
    g, o = teapot
    run_ticks(rt, g, o, W, H, spp, [(0, False), (1, False)], "Tick").close()


def packed_pixels(W, H, tiles):
    """Pixel index of every packed slot [i][64] of the listed global tiles, -1 off the image."""
    tx = (W + 7) // 8
    t = np.asarray(tiles, np.int64)[:, None]
    lane = np.arange(64)[None, :]
    x, y = (t % tx) * 8 + (lane & 7), (t // tx) * 8 + (lane >> 3)
    return np.where((x < W) & (y < H), x + y * W, -1).reshape(-1)


def check_packed(buf, px, want, what):
    got = buf.cpu().numpy().view(np.uint32)[:len(px)]
    ok = px >= 0
    assert np.array_equal(got[ok], want[px[ok]]), f"{what}: {(got[ok] != want[px[ok]]).sum()} RGB8 mismatches"


@pytest.mark.parametrize("W,H", SIZES)
def test_interleaved_shards_packed_output(rt, teapot, torch, W, H):
    """Shard 1 of 3 (and, for the frame's totals, shards 0 and 2) of the interleaved deal."""
    g, o = teapot
    N = 3
    ntiles = ((W + 7) // 8) * ((H + 7) // 8)
    r = rt.Renderer(g, W, H)
    bufs = torch.zeros((N, r.shard_capacity(N)), dtype=torch.int32, device="cuda:0")
    acc = np.zeros((W * H, 4), np.float32)
    stats = []
    for f in range(2):
        want, st = o.tick(W, H, acc, spp=1, depth=1, frame=f)
        stats.append(st)
        for s in (1, 0, 2):
            r.render_shard(bufs[s], s, N, depth=1, frame=f)
            torch.cuda.synchronize()
            check_packed(bufs[s], packed_pixels(W, H, np.arange(s, ntiles, N)), want, f"shard {s}/{N} {W}x{H} frame {f}")
    acc_bits_equal(r.accumulator(), acc, f"shards {W}x{H}")
    counters_equal(r, stats, f"shards {W}x{H}")
    r.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_explicit_permuted_tile_lists(rt, teapot, torch, W, H):
    g, o = teapot
    ntiles = ((W + 7) // 8) * ((H + 7) // 8)
    perm = np.random.default_rng(7).permutation(ntiles).astype(np.uint32)
    lists = [perm[:7], perm[7:]]
    r = rt.Renderer(g, W, H)
    buf = torch.zeros(ntiles * 64, dtype=torch.int32, device="cuda:0")
    acc = np.zeros((W * H, 4), np.float32)
    stats = []
    for f in range(2):
        want, st = o.tick(W, H, acc, spp=1, depth=1, frame=f)
        stats.append(st)
        for k, tiles in enumerate(lists):
            r.render_shard_tiles(buf, tiles, depth=1, frame=f)
            torch.cuda.synchronize()
            check_packed(buf, packed_pixels(W, H, tiles), want, f"tile list {k} {W}x{H} frame {f}")
    acc_bits_equal(r.accumulator(), acc, f"tile lists {W}x{H}")
    counters_equal(r, stats, f"tile lists {W}x{H}")
    r.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_walk_check_build_same_frames(rt, oracle, torch, W, H):
    """k_render_walkcheck shares render_tile: the oracle's frames, and the wave walk's counters run."""
    g = rt.Scene.recipe("teapotF")
    g.set_camera_walk(rt.WALK_WAVE)
    o = oracle.Scene("teapotF", rt.DATA_DIR)
    r = run_ticks(rt, g, o, W, H, 1, [(0, False), (1, False)], "walk check",
                  setup=lambda r: r.set_walk_check(rt.WALK_CHECK_COUNT))
    ws = r.walk_stats()
    assert 0 < ws["walked"] <= 2 * W * H and ws["verify_mismatch"] == 0, ws
    r.close()
    g.close()


def test_pack_rgb8_slow_path_negative_and_huge_channels(rt, oracle, torch):
    """A light of colour (-2.5, 1e12, 0.5) in direct view over a diffuse plane: lit floor pixels and
    the light's own pixels carry negative red (the int64 wrap of pack_rgb8's conversion) beside
    clamped green, next to sky tiles whose channels are ordinary."""
    W, H = 40, 24
    mats = [rt.material(rt.LIGHT, (-2.5, 1e12, 0.5)), rt.material(rt.DIFFUSE, (0.8, 0.8, 0.8))]
    prims = [rt.sphere((0.0, 0.6, 2.0), 0.5, 0), rt.plane((0, 1, 0), 1.0, 1)]
    o = oracle_scene(rt, oracle, prims, mats)
    g = rt.Scene(prims, mats)
    r = run_ticks(rt, g, o, W, H, 1, [(0, False), (1, False)], "negative light")
    a = r.accumulator()
    assert (a[:, 0] < 0).sum() > 64 and (a[:, 0] >= 0).sum() > 64, "the scene must hold negative and ordinary channels"
    r.close()
    g.close()
