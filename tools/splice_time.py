#!/usr/bin/env python3
"""What a mesh entering and leaving a live scene costs: Scene.splice_triangles against
destroying and re-creating the scene, with Scene.rebuild of the same session as the yardstick.

The method is tools/rebuild_time.py's: a clock ramp, warm-up calls, the median of --reps blocking calls
under the host clock (every call ends in a device synchronise), the routes run alternately twice in
one session.  Per scene (teapotF: 300 triangles; mig16: one aircraft's share of the sixteen):
  splice_ms             (a) one call that removes the mesh-sized range [1, 1 + m) and inserts m triangles
                            that lie elsewhere (the same mesh shifted, two places alternately), records
                            in device memory;
  remove_ms, append_ms      the same edit as two calls: the range out, then m triangles appended;
  update_after_ms       (b) the first in-place update after a splice (it downloads the new topology
                            and rebuilds the refit schedule on the host);
  update_ms                 a later update of the same triangles, for comparison;
  rebuild_ms                Scene.rebuild of the same scene in the same session;
  recreate_ms           (c) rt_scene_destroy + rt_scene_create of the spliced description.

usage: python tools/splice_time.py [--scenes teapotF,mig16] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refit_time import PRIM_DTYPE, W, H, create, frame_ms, timed  # noqa: E402

import advancedgraphicsraytracer_amd as rt  # noqa: E402

MESH = {"teapotF": 300}          # triangles of the edit; mig16: (n - 1) / 16
SHIFT = (0.0, 0.75, 0.0)         # where the mesh re-enters, every other call


def run(name, reps):
    prims, mats = rt.recipe_describe(name)
    parr, marr = (rt.Prim * len(prims))(*prims), (rt.Material * len(mats))(*mats)
    view = np.frombuffer(parr, dtype=PRIM_DTYPE)
    n = len(view)
    assert (view["type"][1:] == rt.TRIANGLE).all()
    m = MESH.get(name, (n - 1) // 16)
    # the mesh at its place and shifted: records for the splice, vertices for the update after it
    recs = [view[1:1 + m].copy(), view[1:1 + m].copy()]
    recs[1]["v"] = (recs[1]["v"].reshape(-1, 3, 3) + np.array(SHIFT, np.float32)).reshape(-1, 9)
    drec = [torch.from_numpy(r.view(np.int32).reshape(m, 11).copy()).cuda() for r in recs]
    dver = [torch.from_numpy(r["v"].copy()).cuda() for r in recs]
    shifted = view.copy()
    shifted[1:1 + m] = recs[1]
    sarr = (rt.Prim * n).from_buffer_copy(shifted.tobytes())
    g = create(parr, marr)
    res = {"scene": name, "primitives": n, "edit_triangles": m, "nodes": g.info["nodes_used"]}
    frame_ms(g, 8)                                            # clock ramp before anything is timed
    for k in range(3):                                        # warm-up: every kernel has run once
        g.splice_triangles(1, m, drec[k % 2])
        g.update_triangles(1, dver[k % 2])
        g.rebuild()
        g.splice_triangles(1, m, [])
        g.splice_triangles(n - m, 0, drec[k % 2])
        g.splice_triangles(n - m, m, [])
        g.splice_triangles(1, 0, drec[k % 2])
    assert g.info["num_prims"] == n
    res["splice_stats"] = g.rebuild_stats()
    holder = [create(parr, marr)]

    def recreate(k):
        holder[0].close()
        holder[0] = create(sarr if k % 2 else parr, marr)

    def cycle(reps):
        """each call timed on its own within one cycle; the scene has n primitives again at its end"""
        ms = {"splice": [], "after": [], "later": [], "rebuild": [], "remove": [], "append": []}
        for k in range(reps):
            a, b = drec[(k + 1) % 2], drec[k % 2]
            for key, fn in (("splice", lambda: g.splice_triangles(1, m, a)),
                            ("after", lambda: g.update_triangles(1, dver[k % 2])),
                            ("later", lambda: g.update_triangles(1, dver[(k + 1) % 2])),
                            ("rebuild", g.rebuild),
                            ("remove", lambda: g.splice_triangles(1, m, [])),
                            ("append", lambda: g.splice_triangles(n - m, 0, b))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ms[key].append((time.perf_counter() - t0) * 1e3)
            g.splice_triangles(n - m, m, [])                  # untimed: the mesh back to the front
            g.splice_triangles(1, 0, b)
        return {k: [round(float(np.median(v)), 4), round(float(min(v)), 4)] for k, v in ms.items()}

    rounds = []
    for _ in range(2):                                        # the routes alternately, twice
        c = cycle(reps)
        rec = timed(recreate, max(4, reps // 4))
        rounds.append({"splice_ms": c["splice"][0], "splice_min_ms": c["splice"][1], "update_after_ms": c["after"][0],
                       "update_ms": c["later"][0], "rebuild_ms": c["rebuild"][0], "rebuild_min_ms": c["rebuild"][1],
                       "remove_ms": c["remove"][0], "append_ms": c["append"][0],
                       "recreate_ms": rec[0], "recreate_min_ms": rec[1]})
    holder[0].close()
    res["rounds"] = rounds
    for key in ("splice_ms", "update_after_ms", "update_ms", "rebuild_ms", "remove_ms", "append_ms", "recreate_ms"):
        res[key] = round(float(np.mean([r[key] for r in rounds])), 4)
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="teapotF,mig16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("splice_time.py needs a GPU: nothing is measured without one")
    out = {"tool": "tools/splice_time.py", "clock_ramp_frame": f"{W}x{H} spp 1 depth 1", "reps": a.reps,
           "scenes": [run(s, a.reps) for s in a.scenes.split(",") if s]}
    print(json.dumps(out, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
