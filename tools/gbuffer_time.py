#!/usr/bin/env python3
"""What the first-hit G-buffer costs, at 1920 x 1080 on TEAPOT-F and mig29 x16.

Per scene, after a clock ramp of depth-1 frames (which also lets the renderer's timed choices settle,
so the G-buffer's RT_WALK_AUTO walk is the one its frames run):
  gbuffer_all_ms    rt_render_gbuffer, all four planes (ray, hit, normal, albedo)
  gbuffer_hit_ms    rt_render_gbuffer, the hit plane alone (no shade or material record read)
  frame_ms          the same renderer's depth-1 path frame (camera ray + shading + shadow ray + accumulate), as
                    the renderer runs it: its measured tile order, and several frames in flight where it chose so
  frame_serial_ms   the depth-1 frame of a second scene created with RT_PS_PIPELINE=0: one frame at a time, as
                    a query is one launch at a time
  frame_plain_ms    ... and of a third created with RT_PS_PIPELINE=0 and RT_TILE_ORDER=0: one frame at a time with its
                    tiles in their plain order -- the frame launched the way a query is
  intersect_ms      rt_intersect over the ray plane the G-buffer wrote: the traversal floor, one lane per ray
  pick_host_ms      Renderer.pick_host of one pixel (stage, launch, copy back, synchronise): host clock

The four device routes are timed as one event pair around --inner launches on one stream, the routes
alternating within each of --reps rounds of one session; the figures are medians over the rounds (and
the minimum).  pick_host is the median of --reps blocking calls under the host clock.

usage: python tools/gbuffer_time.py [--scenes teapotF,mig16] [--reps 20] [--inner 50] [--json out.json]
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

W, H = 1920, 1080


def run(name, reps, inner):
    L = rt.lib()
    g = rt.Scene.recipe(name)
    r = rt.Renderer(g, W, H)
    os.environ["RT_PS_PIPELINE"] = "0"        # (read when a scene is created)
    g1 = rt.Scene.recipe(name)
    del os.environ["RT_PS_PIPELINE"]
    r1 = rt.Renderer(g1, W, H)
    os.environ["RT_PS_PIPELINE"], os.environ["RT_TILE_ORDER"] = "0", "0"
    g2 = rt.Scene.recipe(name)
    del os.environ["RT_PS_PIPELINE"], os.environ["RT_TILE_ORDER"]
    r2 = rt.Renderer(g2, W, H)
    dev = "cuda:0"
    st = torch.cuda.Stream()
    s = C.c_void_p(st.cuda_stream)
    out = torch.zeros(W * H, dtype=torch.int32, device=dev)
    planes = {k: torch.zeros((W * H, 7 if k == "ray" else 4), dtype=torch.float32, device=dev) for k in rt.GBUFFER_PLANES}
    g_all = rt.GBuffer(**{k: t.data_ptr() for k, t in planes.items()})
    g_hit = rt.GBuffer(hit=planes["hit"].data_ptr())
    hits = torch.zeros((W * H, 4), dtype=torch.float32, device=dev)
    cam = r.camera
    out1 = torch.zeros(W * H, dtype=torch.int32, device=dev)
    state = {"frame": 0, "frame1": 0, "frame2": 0}

    def frame():
        r.Tick(out, spp=1, depth=1, frame=state["frame"], stream=st.cuda_stream)
        state["frame"] += 1

    def frame_serial():
        r1.Tick(out1, spp=1, depth=1, frame=state["frame1"], stream=st.cuda_stream)
        state["frame1"] += 1

    def frame_plain():
        r2.Tick(out1, spp=1, depth=1, frame=state["frame2"], stream=st.cuda_stream)
        state["frame2"] += 1

    def gbuffer(which):
        p = rt.FrameParams(W, H, 1, 1, max(state["frame"] - 1, 0), rt.MODE_PATH, 0)
        rt._check(L.rt_render_gbuffer(r.h, C.byref(cam), C.byref(p), 0, 0, 0, W, H, C.byref(which), s))

    def intersect():
        rt._check(L.rt_intersect(g.h, C.c_void_p(planes["ray"].data_ptr()), C.c_void_p(hits.data_ptr()), W * H, s))

    routes = {"gbuffer_all_ms": lambda: gbuffer(g_all), "gbuffer_hit_ms": lambda: gbuffer(g_hit), "frame_ms": frame,
              "frame_serial_ms": frame_serial, "frame_plain_ms": frame_plain,
              "intersect_ms": intersect}
    # clock ramp: at least 0.3 s and 64 frames of the heaviest route, then every route once
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3 or state["frame"] < 64:
        for _ in range(8):
            frame()
            frame_serial()
            frame_plain()
        torch.cuda.synchronize()
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                a.record(st)
                for _ in range(inner):
                    fn()
                b.record(st)
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    res = {"scene": name, "primitives": g.info["num_prims"], "nodes": g.info["nodes_used"], "walk": r.choices()["walk"],
           "frame_kernel": r.kernel_name(1, 1), "frames_in_flight": r.overlap_depth()[0], "serial_walk": r1.choices()["walk"],
           "plain_walk": r2.choices()["walk"]}
    for k, v in ms.items():
        res[k] = round(float(np.median(v)), 4)
        res[k.replace("_ms", "_min_ms")] = round(float(min(v)), 4)
    # the traversal floor traced the G-buffer's own rays: the same hits
    gbuffer(g_all)
    intersect()
    torch.cuda.synchronize()
    res["intersect_equals_hit_plane"] = bool(torch.equal(hits.view(torch.int32), planes["hit"].view(torch.int32)))
    pick = []
    for k in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.pick_host([(k * 7919) % (W * H)], frame=0)
        pick.append((time.perf_counter() - t0) * 1e3)
    res["pick_host_ms"] = round(float(np.median(pick[3:])), 4)
    res["pick_host_min_ms"] = round(float(min(pick[3:])), 4)
    r.close()
    r1.close()
    r2.close()
    g.close()
    g1.close()
    g2.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="teapotF,mig16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gbuffer_time.py needs a GPU: nothing is measured without one")
    out = {"tool": "tools/gbuffer_time.py", "frame": f"{W}x{H} spp 1", "reps": a.reps, "inner": a.inner,
           "scenes": [run(s, a.reps, a.inner) for s in a.scenes.split(",") if s]}
    print(json.dumps(out, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
