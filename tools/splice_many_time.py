#!/usr/bin/env python3
"""What several edits in one rebuild cost: Scene.splice_ranges and Scene.compact_triangles
against the same edits as one Scene.splice_triangles call each, with one single-range splice and
Scene.rebuild of the same session as the yardsticks.

The method is tools/splice_time.py's: a clock ramp, warm-up calls, the median of --reps blocking calls
under the host clock (every call ends in a device synchronise), the routes run alternately twice in one
session.  After every timed edit the removed triangles are put back, untimed, by one splice_ranges call.
  mig16     three aircraft leave (three ranges of (n - 1) / 16 triangles):
  teapotF   100 scattered single triangles leave (every tenth from id 10 on):
    ranges_ms    one splice_ranges call, the edits in host memory;
    singles_ms   one splice_triangles call per range, descending (mig16 only: 100 rebuilds tell nothing new);
    mask_ms      one compact_triangles call, the keep-mask in device memory;
    one_ms       one single-range splice_triangles call removing the first range (mig16) or 100
                 consecutive triangles (teapotF) -- the requirement is relative to this;
    one_spread_ms    its run-to-run spread within the session: |difference| of the two rounds' medians
                     and the larger (median - minimum) of a round;
    rebuild_ms   Scene.rebuild.

usage: python tools/splice_many_time.py [--scenes teapotF,mig16] [--reps 20] [--json profiles/splice/splice_many_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refit_time import PRIM_DTYPE, W, H, create, frame_ms  # noqa: E402

import advancedgraphicsraytracer_amd as rt  # noqa: E402


def ranges_of(name, n):
    """the old-id ranges that leave, ascending, and the single range of the yardstick"""
    if name == "teapotF":
        return [(i, 1) for i in range(10, 1010, 10)], (10, 100)
    m = (n - 1) // 16
    r = [(1 + k * m, m) for k in (2, 7, 12)]
    return r, r[0]


def run(name, reps):
    prims, mats = rt.recipe_describe(name)
    parr, marr = (rt.Prim * len(prims))(*prims), (rt.Material * len(mats))(*mats)
    view = np.frombuffer(parr, dtype=PRIM_DTYPE)
    n = len(view)
    assert (view["type"][1:] == rt.TRIANGLE).all()
    ranges, one = ranges_of(name, n)
    dev = lambda a: torch.from_numpy(a.view(np.int32).reshape(-1, 11).copy()).cuda()
    # what leaves, for putting it back: the records of all ranges back to back, and where they return
    # in the id space without them
    gone = dev(np.concatenate([view[f:f + m] for f, m in ranges]))
    back, shift = [], 0
    for f, m in ranges:
        back.append((f - shift, 0, gone if not back else None, m))
        shift += m
    one_gone = dev(view[one[0]:one[0] + one[1]].copy())
    keep = torch.ones(n, dtype=torch.uint8, device="cuda")
    for f, m in ranges:
        keep[f:f + m] = 0
    out_edits = [(f, m, []) for f, m in ranges]
    g = create(parr, marr)
    nodes0 = g.bvh()[0].tobytes()
    res = {"scene": name, "primitives": n, "ranges": len(ranges), "triangles_leaving": shift, "nodes": g.info["nodes_used"]}
    singles = name != "teapotF"

    def routes():
        r = [("ranges", lambda: g.splice_ranges(out_edits), lambda: g.splice_ranges(back)),
             ("mask", lambda: g.compact_triangles(keep), lambda: g.splice_ranges(back)),
             ("one", lambda: g.splice_triangles(one[0], one[1], []), lambda: g.splice_triangles(one[0], 0, one_gone)),
             ("rebuild", g.rebuild, None)]
        if singles:
            r.insert(1, ("singles", lambda: [g.splice_triangles(f, m, []) for f, m in reversed(ranges)], lambda: g.splice_ranges(back)))
        return r

    frame_ms(g, 8)                                            # clock ramp before anything is timed
    for _ in range(3):                                        # warm-up: every kernel has run once
        for _, fn, undo in routes():
            fn()
            if undo:
                undo()
    assert g.info["num_prims"] == n and g.bvh()[0].tobytes() == nodes0   # every edit was undone
    g.splice_ranges(out_edits)
    res["ranges_stats"] = g.rebuild_stats()
    g.splice_ranges(back)
    g.compact_triangles(keep)
    res["mask_stats"] = g.rebuild_stats()
    g.splice_ranges(back)

    def cycle():
        ms = {key: [] for key, _, _ in routes()}
        for _ in range(reps):
            for key, fn, undo in routes():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ms[key].append((time.perf_counter() - t0) * 1e3)
                if undo:
                    undo()
        return {k: [round(float(np.median(v)), 4), round(float(min(v)), 4)] for k, v in ms.items()}

    rounds = [cycle() for _ in range(2)]                      # the routes alternately, twice
    res["rounds"] = [{f"{k}_ms": v[0] for k, v in c.items()} | {f"{k}_min_ms": v[1] for k, v in c.items()} for c in rounds]
    for key in rounds[0]:
        res[f"{key}_ms"] = round(float(np.mean([c[key][0] for c in rounds])), 4)
    res["one_spread_ms"] = round(max(abs(rounds[0]["one"][0] - rounds[1]["one"][0]), *[c["one"][0] - c["one"][1] for c in rounds]), 4)
    assert g.info["num_prims"] == n and g.bvh()[0].tobytes() == nodes0
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="teapotF,mig16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("splice_many_time.py needs a GPU: nothing is measured without one")
    out = {"tool": "tools/splice_many_time.py", "clock_ramp_frame": f"{W}x{H} spp 1 depth 1", "reps": a.reps,
           "scenes": [run(s, a.reps) for s in a.scenes.split(",") if s]}
    print(json.dumps(out, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
