#!/usr/bin/env python3
"""What an animated mesh costs per change: Scene.update_triangles (in-place vertex update + GPU BVH
refit) against destroying and re-creating the scene, and how far the refitted tree's quality decays.

Per scene (teapotF, mig16), after a clock ramp and warm-up updates:
  full_update_ms       median wall time of update_triangles over every triangle (device vertices;
                       the call blocks, so the host clock around it ends in a device synchronise);
  full_update_host_ms  the same with the vertices in host memory (staged by the library);
  range_update_ms      the same for the first 1/16 of the triangles (one aircraft of mig16);
  first_update_ms      the scene's first update, which also builds the refit plan;
  recreate_ms          median of rt_scene_destroy + rt_scene_create from a ready description (host
                       binned-SAH build + upload) -- the only route without update_triangles;
  frames               primary+shadow 1080p time per frame (config 2 / config 4; HIP events around a
                       run of frames) on the refitted tree after a modest and a large twist, beside
                       a fresh build of the same geometry, measured alternately twice.

usage: python tools/refit_time.py [--scenes teapotF,mig16] [--reps 20] [--frames 400] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import advancedgraphicsraytracer_amd as rt  # noqa: E402

PRIM_DTYPE = np.dtype([("type", "<i4"), ("material", "<i4"), ("v", "<f4", 9)])
W, H = 1920, 1080
TWISTS = {"modest": 0.15, "large": 1.0}


def twist(verts, k):
    """twist about y by k radians per unit of y, per vertex ([n, 9] float32 in and out)"""
    v = verts.reshape(-1, 3).astype(np.float64)
    a = k * v[:, 1]
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], 1).astype(np.float32).reshape(-1, 9)


def create(parr, marr):
    d = rt.SceneDesc()
    d.prims, d.num_prims = parr, len(parr)
    d.materials, d.num_materials = marr, len(marr)
    h = C.c_void_p()
    rt._check(rt.lib().rt_scene_create(C.byref(d), C.byref(h)))
    return rt.Scene(device=0, _handle=h)


def frame_ms(scene, frames, warm=40):
    r = rt.Renderer(scene, W, H)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream()
    nf, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 0.3 or nf < warm:   # clock ramp; the renderer's timed choices settle
        for _ in range(8):
            r.Tick(out, spp=1, depth=1, frame=nf, stream=st.cuda_stream)
            nf += 1
        torch.cuda.synchronize()
    # frames may overlap (several in flight on the renderer's streams), so one event pair spans the
    # whole run: throughput per frame, as bench.py's ms_per_step
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        a.record(st)
        for k in range(frames):
            r.Tick(out, spp=1, depth=1, frame=nf + k, stream=st.cuda_stream)
        b.record(st)
    torch.cuda.synchronize()
    r.close()
    return round(a.elapsed_time(b) / frames, 4)


def timed(fn, reps):
    ms = []
    for k in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


def run(name, reps, frames):
    prims, mats = rt.recipe_describe(name)
    parr, marr = (rt.Prim * len(prims))(*prims), (rt.Material * len(mats))(*mats)
    view = np.frombuffer(parr, dtype=PRIM_DTYPE)
    tri = np.flatnonzero(view["type"] == rt.TRIANGLE)
    first, n = int(tri[0]), len(tri)
    assert np.array_equal(tri, np.arange(first, first + n))
    v0 = view["v"][tri].copy()
    sets = {k: twist(v0, a) for k, a in TWISTS.items()}
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(sets, rest=v0).items()}
    g = create(parr, marr)
    info = g.info
    frame_ms(g, 8)                                            # clock ramp before anything is timed
    t0 = time.perf_counter()
    g.update_triangles(first, dev["modest"])
    res = {"scene": name, "triangles": n, "nodes": info["nodes_used"],
           "first_update_ms": round((time.perf_counter() - t0) * 1e3, 4)}
    for k in range(3):
        g.update_triangles(first, dev["rest" if k % 2 == 0 else "modest"])
    order = ["modest", "rest"]
    res["full_update_ms"], res["full_update_min_ms"] = timed(lambda k: g.update_triangles(first, dev[order[k % 2]]), reps)
    host = [sets["modest"], v0]
    res["full_update_host_ms"], _ = timed(lambda k: g.update_triangles(first, host[k % 2]), reps)
    part = n // 16
    pdev = [dev["modest"][:part].contiguous(), dev["rest"][:part].contiguous()]
    res["range_triangles"] = part
    res["range_update_ms"], res["range_update_min_ms"] = timed(lambda k: g.update_triangles(first, pdev[k % 2]), reps)
    g.update_triangles(first, dev["rest"])
    holder = [create(parr, marr)]

    def recreate(_):
        holder[0].close()
        holder[0] = create(parr, marr)
    res["recreate_ms"], res["recreate_min_ms"] = timed(recreate, max(3, reps // 4))
    holder[0].close()
    res["frames"] = {"untouched_ms": frame_ms(g, frames)}
    for k in TWISTS:
        view["v"][tri] = sets[k]
        fresh = create(parr, marr)
        g.update_triangles(first, dev[k])
        pair = {"refit_ms": [], "fresh_ms": []}
        for _ in range(2):
            pair["refit_ms"].append(frame_ms(g, frames))
            pair["fresh_ms"].append(frame_ms(fresh, frames))
        fresh.close()
        res["frames"][k] = dict(pair, twist_rad_per_unit=TWISTS[k])
    view["v"][tri] = v0
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="teapotF,mig16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refit_time.py needs a GPU: nothing is measured without one")
    out = {"tool": "tools/refit_time.py", "frame": f"{W}x{H} spp 1 depth 1", "reps": a.reps,
           "scenes": [run(s, a.reps, a.frames) for s in a.scenes.split(",") if s]}
    print(json.dumps(out, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
