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

With --kinds the any-kind routes of DESIGN 4.14 are measured the same way instead:
  mig16        one aircraft removed and re-inserted in one call, through Scene.splice_triangles and through
               Scene.splice_prims alternately: the difference is the rank scan and the side-table pass on a
               scene without a side table; and Scene.set_prim_materials over the aircraft against the
               splice that would otherwise change its material;
  room         16 crates (cubes) entering and leaving the room through Scene.splice_prims, against
               rt_scene_destroy + rt_scene_create of either description.

usage: python tools/splice_time.py [--scenes teapotF,mig16] [--reps 20] [--json out.json] [--kinds]
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


def med(ms):
    return [round(float(np.median(ms)), 4), round(float(min(ms)), 4)]


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def run_kinds_mig(reps):
    """mig16: the triangle route and the any-kind route on the same edit, and the material change"""
    prims, mats = rt.recipe_describe("mig16")
    parr, marr = (rt.Prim * len(prims))(*prims), (rt.Material * len(mats))(*mats)
    view = np.frombuffer(parr, dtype=PRIM_DTYPE)
    n = len(view)
    m = (n - 1) // 16
    recs = [view[1:1 + m].copy(), view[1:1 + m].copy()]
    recs[1]["v"] = (recs[1]["v"].reshape(-1, 3, 3) + np.array(SHIFT, np.float32)).reshape(-1, 9)
    drec = [torch.from_numpy(r.view(np.int32).reshape(m, 11).copy()).cuda() for r in recs]
    other = (int(view["material"][1]) + 1) % len(mats) or 1          # another material, not the light's
    remat = [r.copy() for r in recs]
    for r in remat:
        r["material"] = other
    dremat = [torch.from_numpy(r.view(np.int32).reshape(m, 11).copy()).cuda() for r in remat]
    dmat = [torch.full((m,), int(view["material"][1]), dtype=torch.int32, device="cuda"),
            torch.full((m,), other, dtype=torch.int32, device="cuda")]
    g = create(parr, marr)
    res = {"scene": "mig16", "primitives": n, "edit_triangles": m}
    frame_ms(g, 8)                                            # clock ramp before anything is timed
    for k in range(3):                                        # warm-up: every kernel has run once
        g.splice_triangles(1, m, drec[k % 2])
        g.splice_prims([(1, m, (drec[k % 2], None), m)])
        g.set_prim_materials(1, dmat[k % 2])
    rounds = []
    for _ in range(2):                                        # the routes alternately, twice
        ms = {"triangles": [], "prims": [], "materials": [], "material_splice": []}
        for k in range(reps):
            a = drec[(k + 1) % 2]
            ms["triangles"].append(clock(lambda: g.splice_triangles(1, m, a)))
            ms["prims"].append(clock(lambda: g.splice_prims([(1, m, (a, None), m)])))
            ms["materials"].append(clock(lambda: g.set_prim_materials(1, dmat[(k + 1) % 2])))
            ms["material_splice"].append(clock(lambda: g.splice_prims([(1, m, (dremat[k % 2], None), m)])))
            g.set_prim_materials(1, dmat[0])
        rounds.append({k + "_ms": med(v)[0] for k, v in ms.items()} | {k + "_min_ms": med(v)[1] for k, v in ms.items()})
    res["launches_prims"] = g.rebuild_stats()[3]
    g.splice_triangles(1, m, drec[0])
    res["launches_triangles"] = g.rebuild_stats()[3]
    res["rounds"] = rounds
    for key in ("triangles_ms", "prims_ms", "materials_ms", "material_splice_ms"):
        res[key] = round(float(np.mean([r[key] for r in rounds])), 4)
    res["prims_minus_triangles_ms"] = round(res["prims_ms"] - res["triangles_ms"], 4)
    g.close()
    return res


def run_kinds_room(reps):
    """the room: 16 crates enter behind the last primitive and leave again"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from anim_util import room_mats, room_prims
    room, mats = room_prims(rt, 0.0), room_mats(rt)
    rng = np.random.default_rng(7)
    crates = [rt.cube((0, 0, 0), 0.3, 3, rt.mat4_mul(rt.mat4_translate(*[float(x) for x in rng.uniform((-2, -0.8, 0.5), (2, 1.5, 3.5))]),
                                                      rt.mat4_rotate(1, float(rng.uniform(0, 3))))) for _ in range(16)]
    rec, T = rt.pack_prims(crates)
    pair = (torch.from_numpy(rec).cuda(), torch.from_numpy(T).cuda())
    n = len(room)
    g = rt.Scene(room, mats)
    res = {"scene": "room", "primitives": n, "crates": len(crates)}
    frame_ms(g, 8)
    for _ in range(3):
        g.splice_prims([(n, 0, pair, 16)])
        g.splice_prims([(n, 16, None, 0)])
    holder = [rt.Scene(room, mats)]

    def recreate(k):
        holder[0].close()
        holder[0] = rt.Scene(room + crates if k % 2 == 0 else room, mats)

    rounds = []
    for _ in range(2):
        enter, leave = [], []
        for k in range(reps):
            enter.append(clock(lambda: g.splice_prims([(n, 0, pair, 16)])))
            leave.append(clock(lambda: g.splice_prims([(n, 16, None, 0)])))
        rec_ms = timed(recreate, max(4, reps // 2))
        rounds.append({"enter_ms": med(enter)[0], "leave_ms": med(leave)[0], "recreate_ms": rec_ms[0], "recreate_min_ms": rec_ms[1]})
    holder[0].close()
    res["rounds"] = rounds
    for key in ("enter_ms", "leave_ms", "recreate_ms"):
        res[key] = round(float(np.mean([r[key] for r in rounds])), 4)
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="teapotF,mig16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--kinds", action="store_true", help="the any-kind routes of DESIGN 4.14 instead of --scenes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("splice_time.py needs a GPU: nothing is measured without one")
    out = {"tool": "tools/splice_time.py", "clock_ramp_frame": f"{W}x{H} spp 1 depth 1", "reps": a.reps,
           "scenes": [run_kinds_mig(a.reps), run_kinds_room(a.reps)] if a.kinds else [run(s, a.reps) for s in a.scenes.split(",") if s]}
    print(json.dumps(out, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
