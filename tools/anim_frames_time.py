#!/usr/bin/env python3
"""What one frame of an animated scene costs, the update included: the loop "update, then frame with
reset = 1", in the blocking style (Scene.update_* / transform_triangles block, so every frame starts
from an empty queue) and in the stream-ordered style (wait=False: update and frame are enqueued on one
stream and the host runs ahead), beside the static frame time of the same renderer.

1080p primary+shadow frames (spp 1, depth 1).  Per scene, after a clock ramp during which the renderer's
timed choices settle, every loop is timed as a window of --frames frames on the host clock, ending in a
device synchronise (the async window also ends in its update_sync), --reps windows each, median and
min / max; the styles are measured alternately, twice each in one session:
  teapotF  full    Scene.update_triangles over every triangle, two poses alternating;
  mig16    xform   ONE Scene.transform_triangles call moving all 16 aircraft, two poses alternating;
  mig16    full    Scene.update_triangles over every triangle.
static_ms is the same window of reset frames without any update.

usage: python tools/anim_frames_time.py [--frames 100] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import advancedgraphicsraytracer_amd as rt  # noqa: E402
from anim_time import aircraft_matrices  # noqa: E402
from refit_time import PRIM_DTYPE, W, H, create, twist  # noqa: E402


def windows(fn, frames, reps):
    """reps windows of `frames` calls of fn(k), each ending in fn.end() and a device synchronise: ms per frame"""
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(frames):
            fn(k)
        fn.end()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / frames)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


class Loop:
    def __init__(self, g, r, out, st, update):
        self.g, self.r, self.out, self.st, self.update = g, r, out, st, update
        self.n = 0

    def frame(self):
        self.r.Tick(self.out, spp=1, depth=1, frame=self.n, reset=True, stream=self.st.cuda_stream)
        self.n += 1


class Static(Loop):
    def __call__(self, k):
        self.frame()

    def end(self):
        pass


class Blocking(Loop):
    def __call__(self, k):
        self.update(k, True, self.st.cuda_stream)
        self.frame()

    def end(self):
        pass


class Async(Loop):
    def __call__(self, k):
        self.update(k, False, self.st.cuda_stream)
        self.frame()

    def end(self):
        st = self.g.update_sync()
        assert st["refused"] == 0, st


def measure(name, g, updates, frames, reps):
    r = rt.Renderer(g, W, H)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream()
    g.prepare_updates()
    static = Static(g, r, out, st, None)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.4 or static.n < 160:      # clock ramp; the timed choices settle
        for k in range(8):
            static(k)
        torch.cuda.synchronize()
    res = {"scene": name, "triangles": None, "static_ms": [], "loops": {}}
    for key, upd in updates.items():
        for style in (Blocking, Async):                          # warm-up of both routes
            loop = style(g, r, out, st, upd)
            for k in range(8):
                loop(k)
            loop.end()
        res["loops"][key] = {"blocking_ms": [], "async_ms": []}
    torch.cuda.synchronize()
    for _ in range(2):                                           # alternately, twice
        res["static_ms"].append(windows(static, frames, reps))
        for key, upd in updates.items():
            res["loops"][key]["blocking_ms"].append(windows(Blocking(g, r, out, st, upd), frames, reps))
            res["loops"][key]["async_ms"].append(windows(Async(g, r, out, st, upd), frames, reps))
    for key, v in res["loops"].items():
        b, a = v["blocking_ms"], v["async_ms"]
        spread = max(x["max"] for x in b) - min(x["min"] for x in b)
        gain = float(np.mean([x["median"] for x in b]) - np.mean([x["median"] for x in a]))
        v["blocking_spread_ms"], v["gain_ms"] = round(spread, 4), round(gain, 4)
        v["async_faster_beyond_spread"] = bool(gain > spread)
    res["overlap_depth"] = r.overlap_depth()[0]
    r.close()
    return res


def teapot(frames, reps):
    prims, mats = rt.recipe_describe("teapotF")
    parr, marr = (rt.Prim * len(prims))(*prims), (rt.Material * len(mats))(*mats)
    view = np.frombuffer(parr, dtype=PRIM_DTYPE)
    tri = np.flatnonzero(view["type"] == rt.TRIANGLE)
    first, v0 = int(tri[0]), view["v"][tri].copy()
    dev = [torch.from_numpy(twist(v0, a)).cuda() for a in (0.15, -0.15)]
    g = create(parr, marr)

    def full(k, wait, stream):
        g.update_triangles(first, dev[k % 2], stream=stream, wait=wait)
    res = measure("teapotF", g, {"full": full}, frames, reps)
    res["triangles"] = len(tri)
    g.close()
    return res


def mig16(frames, reps):
    V, F = rt.load_mesh(os.path.join(rt.DATA_DIR, "mig29.rtmesh"))
    nt = len(F)
    prims, mats = rt.recipe_describe("mig16")
    parr, marr = (rt.Prim * len(prims))(*prims), (rt.Material * len(mats))(*mats)
    g = create(parr, marr)
    rest = torch.from_numpy(np.tile(V[F].reshape(nt, 9).astype(np.float32), (16, 1))).cuda()
    ranges = [[(1 + i * nt, nt, M) for i, M in enumerate(aircraft_matrices(p))] for p in (0.0, 0.2)]
    world = [torch.from_numpy(world_vertices(rg, V, F)).cuda() for rg in ranges]   # the poses as vertices, for the full update

    def xform(k, wait, stream):
        g.transform_triangles(ranges[k % 2], rest, stream=stream, wait=wait)

    def full(k, wait, stream):
        g.update_triangles(1, world[k % 2], stream=stream, wait=wait)
    res = measure("mig16", g, {"xform": xform, "full": full}, frames, reps)
    res["triangles"], res["ranges"] = 16 * nt, 16
    g.close()
    return res


def world_vertices(ranges, V, F):
    """world vertices of the 16 aircraft as rt_mesh_to_prims places them ([16 nt, 9] float32)"""
    out = []
    for _, _, M in ranges:
        p = rt.mesh_to_prims(V, F, M, 1)
        out.append(np.frombuffer((rt.Prim * len(p))(*p), dtype=PRIM_DTYPE)["v"].copy())
    return np.concatenate(out, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("anim_frames_time.py needs a GPU: nothing is measured without one")
    out = {"tool": "tools/anim_frames_time.py", "frame": f"{W}x{H} spp 1 depth 1, reset = 1", "frames_per_window": a.frames,
           "reps": a.reps, "scenes": [teapot(a.frames, a.reps), mig16(a.frames, a.reps)]}
    print(json.dumps(out, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
