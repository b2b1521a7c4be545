"""The renderer's timed choices (camera walk, half-tile split order, frames in flight) time groups
of frames submitted back to back.  A group in which the GPU ran dry between two frames (the caller
synchronised) is timed again, at most kTuneRestarts times per group (csrc/rt_tune.h), so a
caller that synchronises after EVERY frame still gets a decision; frames are the same whatever is
decided."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def test_choices_decided_when_the_caller_syncs_every_frame(rt, torch):
    g = rt.Scene.recipe("mig16")            # walk timed, tail-bound: split order and deep frames in flight
    W, H = 480, 270
    r = rt.Renderer(g, W, H)
    g_ref = rt.Scene.recipe("mig16")
    g_ref.set_camera_walk(rt.WALK_LANE)
    ref = rt.Renderer(g_ref, W, H)
    for f in range(700):                     # tick_host: a host synchronisation after every frame
        a = r.tick_host(spp=1, depth=1, frame=f)
        if f % 50 == 0 or f > 680:
            b = ref.tick_host(spp=1, depth=1, frame=f)
            assert np.array_equal(a, b), f"frame {f}"
        else:
            ref.tick_host(spp=1, depth=1, frame=f)
    ch = r.choices()
    assert ch["walk"] in (0, 1) and ch["split"] in (0, 1), ch
    assert r.overlap_depth()[0] in (1, 2, 4, 6)
    assert np.array_equal(r.accumulator().view(np.uint32), ref.accumulator().view(np.uint32))
    r.close()
    ref.close()


def test_decisions_fall_on_fixed_frames_when_every_frame_stalls(rt, torch):
    """A caller that synchronises after every frame makes every timed group use all its restarts,
    so the frame on which each choice is first reported is fixed by the group scheduler
    (csrc/rt_tune.h) alone.  Counts are 1-based calls:
      walk   1 warm-up + 4 groups x (1 + 4 + 3) frames, decided on the next call        -> 34
      split  the order is built on call 34 and its first timed frame runs there; 32
             timed frames, decided on the next call                                     -> 66
      depth  frames in flight start on call 66 (deep shape: 240 tiles are less than one
             round of waves); 8 groups x (1 + 4 + 31) frames, decided on the next call  -> 354"""
    g = rt.Scene.recipe("mig16")
    W, H = 160, 96
    r = rt.Renderer(g, W, H)
    g_ref = rt.Scene.recipe("mig16")
    g_ref.set_camera_walk(rt.WALK_LANE)
    ref = rt.Renderer(g_ref, W, H)
    first = {}
    for f in range(360):
        a = r.tick_host(spp=1, depth=1, frame=f)
        b = ref.tick_host(spp=1, depth=1, frame=f)
        if f % 50 == 0:
            assert np.array_equal(a, b), f"frame {f}"
        ch = r.choices()
        seen = {"walk": ch["walk"] >= 0, "split": ch["split"] >= 0, "depth": r.overlap_depth()[0] >= 0}
        for k, v in seen.items():
            if v:
                first.setdefault(k, f + 1)
    print("first decided on call:", first)
    assert first == {"walk": 34, "split": 66, "depth": 354}, first
    assert np.array_equal(r.accumulator().view(np.uint32), ref.accumulator().view(np.uint32))
    r.close()
    ref.close()


def test_choices_decided_back_to_back(rt, torch):
    """The usual caller: frames queued on a stream, an occasional synchronisation (every 100
    frames, as bench.py's multi-GPU clock ramp does)."""
    g = rt.Scene.recipe("teapotF")
    W, H = 640, 360
    r = rt.Renderer(g, W, H)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream()
    for f in range(600):
        r.Tick(out, spp=1, depth=1, frame=f, stream=st.cuda_stream)
        if f % 100 == 99:
            st.synchronize()
    torch.cuda.synchronize()
    ch = r.choices()
    assert ch["walk"] in (0, 1) and ch["split"] in (0, 1), ch
    assert r.overlap_depth()[0] in (1, 2, 4, 6)
    r.close()
