#!/usr/bin/env python3
"""Per-phase wave cycles of the primary+shadow frame kernel, from a diagnostic build's stamps
(tools/build_variant.sh NAME -DRT_FRAME_PHASES; rt_kernels.inc frame_phase): the first active lane of
each wave stores s_memtime at wave start, head done, camera traversal done, shading done, shadow traversal
done and wave end.  Renders serial TEAPOT-F frames (no tile order, no frames in flight, so a wave is
a whole tile in launch order), reads the last frame's stamps and prints mean, median and the 10 / 90
percentiles of each phase, for sky waves (no lane shaded a diffuse hit: no shadow stamps) and
shadow-casting waves apart.  The table is in s_memtime ticks (the counter the tile costs use).

usage: frame_phases.py LIB [--scene teapotF] [--w 1920] [--h 1080] [--frames 40] [--json OUT]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ["head", "camera traversal", "shading", "shadow traversal", "tail"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--scene", default="teapotF")
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.environ["RTAMD_LIB"] = os.path.abspath(a.lib)
    for k in ("RT_TILE_ORDER", "RT_PS_PIPELINE", "RT_WAVE_PRIMARY"):   # plain order, serial frames, lane walk
        os.environ[k] = "0"
    sys.path.insert(0, ROOT)
    import advancedgraphicsraytracer_amd as rt
    L = rt.lib()
    L.rt_debug_frame_phases.argtypes = [C.c_void_p, C.c_size_t]
    g = rt.Scene.recipe(a.scene)
    r = rt.Renderer(g, a.w, a.h)
    for f in range(a.frames - 1):
        r.tick_host(spp=1, depth=1, frame=f)
    assert L.rt_debug_frame_phases_clear() == 0
    r.tick_host(spp=1, depth=1, frame=a.frames - 1)
    nwaves = ((a.w + 7) // 8) * ((a.h + 7) // 8)
    buf = np.zeros((nwaves, 8), np.uint64)
    assert L.rt_debug_frame_phases(buf.ctypes.data_as(C.c_void_p), buf.size) == 0
    t = buf[:, :6].astype(np.int64)
    assert (t[:, 0] > 0).all() and (t[:, 5] >= t[:, 0]).all(), "every wave stamps its start and end"
    shadow = t[:, 3] > 0                      # some lane set up a shadow ray
    hit = t[:, 2] > 0                         # (every wave with a lane on the image traces camera rays)
    out = {"lib": os.path.basename(a.lib), "scene": a.scene, "w": a.w, "h": a.h, "waves": int(nwaves)}
    for name, sel in (("sky", hit & ~shadow), ("shadow", shadow)):
        x = t[sel]
        d = np.stack([x[:, 1] - x[:, 0], x[:, 2] - x[:, 1],
                      np.where(x[:, 3] > 0, x[:, 3] - x[:, 2], 0), np.where(x[:, 4] > 0, x[:, 4] - x[:, 3], 0),
                      x[:, 5] - np.maximum(x[:, 4], x[:, 2])], axis=1)
        total = x[:, 5] - x[:, 0]
        rows = {}
        print(f"{out['lib']}: {name} waves {len(x)} of {nwaves}, mean residency {total.mean():.1f} ticks")
        for k, ph in enumerate(PHASES):
            c = d[:, k]
            rows[ph] = {"mean": round(float(c.mean()), 2), "median": float(np.median(c)), "p10": float(np.percentile(c, 10)),
                        "p90": float(np.percentile(c, 90)), "share": round(float(c.sum() / max(1, total.sum())), 4)}
            print(f"  {ph:17s} mean {rows[ph]['mean']:8.2f}  median {rows[ph]['median']:6.0f}  p10 {rows[ph]['p10']:6.0f}  "
                  f"p90 {rows[ph]['p90']:6.0f}  share {100 * rows[ph]['share']:5.1f} %")
        out[name] = {"waves": int(len(x)), "mean_total": round(float(total.mean()), 2), "phases": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    r.close()
    g.close()


if __name__ == "__main__":
    main()
