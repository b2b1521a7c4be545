"""The renderer's growable device buffers (DevBuf, ResultRing: csrc/rt_refit.h, csrc/rt_device.hip).

* rt_renderer_device_bytes is the sum of what is allocated: the plain and the split order with room for
  every tile in eighths (9 n words) and one cost map per camera walk (2 n), and the work map of a dry run.
* Every buffer along its grow path -- the tile list of a deal that gets longer and shorter again, the orders
  and cost maps that follow its length, the sample buffer of sample-split frames, the path-state slots, the
  per-sample results and the running sum of path-traced frames -- on a frame with partial edge tiles: the
  frames are those of a renderer without any of it, and the renderer may outlive its scene's handle.

Small frames: what can go wrong here is bookkeeping, which 40 tiles show as well as 32,400."""
import numpy as np
import pytest

from test_edits_under_schedule_gpu import CONTROL, KNOBS, LEAD_CAP
from test_rebuild_gpu import soup
from test_splice_prims_gpu import mats4

pytestmark = pytest.mark.gpu

PATH = 0   # rt.MODE_PATH


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def scene_of(rt, monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return rt.Scene(soup(rt, 60, 63), mats4(rt))


def test_device_bytes_are_what_is_allocated(rt, torch, monkeypatch):
    W, H, NT = 64, 40, 40
    g = scene_of(rt, monkeypatch, {"RT_TILE_ORDER": "1", "RT_SPLIT_HEAVY": "4", "RT_PS_PIPELINE": "0", "RT_SPLIT_UNITS": "0",
                                   "RT_TUNE_DELAY_MS": "0"})
    r = rt.Renderer(g, W, H)
    assert r.mode == PATH
    out = torch.zeros(W * H, dtype=torch.int32, device=f"cuda:{g.device}")
    b0 = r.device_bytes()[0]
    for f in range(3):
        r.Tick(out, spp=1, depth=1, frame=f)
    torch.cuda.synchronize()
    b1 = r.device_bytes()[0]
    print(f"orders and cost maps: {b1 - b0} bytes")
    assert b1 - b0 == 11 * NT * 4, (b0, b1)               # plain | split order 9 n words, two cost maps 2 n
    r.tile_work(spp=1, depth=1, frame=0)
    b2 = r.device_bytes()[0]
    print(f"work map: {b2 - b1} bytes")
    assert b2 - b1 == NT * 4, (b1, b2)
    assert r.device_bytes()[1] == 0
    r.close()
    g.close()


W, H, TILES_X, NT = 60, 36, 8, 40         # the last column of tiles is 4 pixels wide, the last row 4 high


def pixels_in(tiles):
    """the frame's pixels inside the listed tiles, counted one pixel at a time"""
    inside = np.zeros(NT, bool)
    inside[np.asarray(tiles)] = True
    y, x = np.mgrid[0:H, 0:W]
    return int(inside[(y // 8) * TILES_X + x // 8].sum())


def test_grow_paths_render_the_control_frames(rt, torch, monkeypatch):
    five = np.array([39, 3, 15, 33, 18], np.uint32)       # the corner tile (4 x 4 pixels), one of each partial edge
    rest = np.setdiff1d(np.arange(NT, dtype=np.uint32), five)
    twelve = np.random.default_rng(91).permutation(rest)[:12]
    assert pixels_in([39]) == 16 and pixels_in(five) == 16 + 64 + 32 + 32 + 64
    knobs = {"RT_TILE_ORDER": "1", "RT_SPLIT_HEAVY": "64", "RT_SPLIT_PARTS": "8", "RT_SPLIT_UNITS": "1000000",
             "RT_TUNE_DELAY_MS": "0"}                     # (the suite's default, conftest.py: scene_of clears every knob)
    runs, leads = [], []
    for control in (False, True):
        g = scene_of(rt, monkeypatch, CONTROL if control else knobs)
        r = rt.Renderer(g, W, H)
        dev = f"cuda:{g.device}"
        outs, primary, lead = [], 0, 0
        c0 = r.counters()["primary"]

        def frame(tiles, spp, depth, f):
            nonlocal primary
            outs.append(r.render_shard_tiles(torch.zeros(64 * len(tiles), dtype=torch.int32, device=dev), tiles,
                                             spp=spp, depth=depth, frame=f, reset=f == 0))
            primary += pixels_in(tiles) * spp

        for tiles in (five, twelve, five):
            # until the list's order is active with every tile in eighths (9 n entries); the control replays the count
            n = 0
            while (n < leads[lead] if control else not (len(r.tile_costs()) == len(tiles) and r.choices()["split"] == 1)):
                assert n < LEAD_CAP, (r.choices(), len(r.tile_costs()))
                frame(tiles, 1, 1, n)
                n += 1
            if not control:
                leads.append(n)
            lead += 1
            for f in range(n, n + 3):
                frame(tiles, 1, 1, f)
        before = r.device_bytes()[0]
        for spp in (2, 4):                                # (tile, sample chunk) units: d_samples appears, then grows
            for f in range(2):
                frame(five, spp, 1, f)
            if not control:
                assert r.device_bytes()[0] - before >= spp * 5 * 64 * 16
        before = r.device_bytes()[0]
        for f in range(2):                                # the wavefront tracer: path-state slots, results, d_sum
            frame(five, 4, 3, f)
        assert r.device_bytes()[0] - before >= NT * 64 * 16 + 5 * 64 * (32 + 16 + 2 * 32)
        torch.cuda.synchronize()
        host = [o.cpu().numpy() for o in outs]
        assert r.counters()["primary"] - c0 == primary
        runs.append(host)
        g.close()                                         # the scene's handle first: the renderer frees its buffers
        r.close()                                         # on the device it remembered
    test, ctrl = runs
    print(f"lead-ins {leads}, {len(test)} frames")
    assert len(test) == len(ctrl)
    for i, (a, b) in enumerate(zip(test, ctrl)):
        assert a.tobytes() == b.tobytes(), f"frame {i}: {(a != b).sum()} words differ from the control's"
