"""Helpers of the BVH analysis tests (test_bvh_heat_host.py, test_bvh_heat_gpu.py): a numpy float32
model of Scene::BVHVisualization (template/scene.h:244-283), the heat frame's colour, accumulator and
RGB8 from its counts, the tree cost in numpy float64, and the scenes and rays both files use.

The model is vectorised over rays and iterated until no ray is live.  Its box test mirrors the oracle's
intersect_aabb (oracle/rt_oracle.c:723): the slab products in float32, min / max as the selects of
std::min / std::max -- (b < a) ? b : a and (a < b) ? b : a -- so a NaN product (0 * inf) resolves the
way the reference's does; test_bvh_heat_host.py pins it to the oracle's own traversal counters."""
import math

import numpy as np

from anim_util import room_mats, room_prims
from refit_util import scene_cases, tree_of

W, H = 36, 20          # a 5 x 3 tile grid with a partial tile on both edges
BATCHES = (1, 63, 65, 257)
F32 = np.float32
# refit_util.twist's rate in the refit-or-rebuild scenario: the smallest of 1, 1.5, 2 rad / unit at
# which TEAPOT-F's refitted tree costs more than a fresh build of the twisted mesh (sah, numpy: 1.0
# 3.193 < 3.421, 1.5 3.453 < 3.639, 2.0 3.515 > 3.255)
TWIST = 2.0


def smin(a, b):
    return np.where(b < a, b, a)


def smax(a, b):
    return np.where(a < b, b, a)


def _box_dist(f, k, O, rD, t):
    """IntersectAABB of node k[i] for ray i (template/scene.h:432-450), float32 throughout"""
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = f[k, 0:3], f[k, 3:6]
        t1, t2 = (lo - O) * rD, (hi - O) * rD
        tmn, tmx = smin(t1[:, 0], t2[:, 0]), smax(t1[:, 0], t2[:, 0])
        for c in (1, 2):
            tmn = smax(tmn, smin(t1[:, c], t2[:, c]))
            tmx = smin(tmx, smax(t1[:, c], t2[:, c]))
        ok = (tmx >= tmn) & (tmn < t) & (tmx > 0)
    return np.where(ok, tmn, F32(1e30)).astype(F32)


def np_visualize(nodes, rays):
    """uint32 [n, 2]: nodeTraversals, intersections per ray"""
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32)
    f, u = nodes.view(F32).reshape(-1, 8), nodes.view(np.uint32).reshape(-1, 8)
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 7)
    n = len(rays)
    O = rays[:, 0:3]
    with np.errstate(divide="ignore"):
        rD = (F32(1) / rays[:, 3:6]).astype(F32)
    t = rays[:, 6]
    stack = np.zeros((n, 64), np.int64)
    sp = np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    out = np.zeros((n, 2), np.uint32)
    far = F32(1e30)
    while live.any():
        idx = np.nonzero(live)[0]
        out[idx, 0] += 1
        leaf = u[node[idx], 7] > 0
        li = idx[leaf]
        out[li, 1] += 1
        ii = idx[~leaf]
        c1 = u[node[ii], 6].astype(np.int64)
        c2 = c1 + 1
        d1 = _box_dist(f, c1, O[ii], rD[ii], t[ii])
        d2 = _box_dist(f, c2, O[ii], rD[ii], t[ii])
        sw = d1 > d2
        d1, d2, c1, c2 = np.where(sw, d2, d1), np.where(sw, d1, d2), np.where(sw, c2, c1), np.where(sw, c1, c2)
        miss = d1 == far
        go = ii[~miss]
        node[go] = c1[~miss]
        push = ~miss & (d2 != far)
        pi = ii[push]
        stack[pi, sp[pi]] = c2[push]
        sp[pi] += 1
        # leaves and interior nodes whose children both missed take the next stack entry, or end
        pop = np.concatenate([li, ii[miss]])
        done = sp[pop] == 0
        live[pop[done]] = False
        pp = pop[~done]
        sp[pp] -= 1
        node[pp] = stack[pp, sp[pp]]
    return out


def heat_colour(counts, depth):
    """the sample's value (template/scene.h:282) in float32: [n, 3]"""
    c = np.zeros((len(counts), 3), F32)
    c[:, 0] = counts[:, 1].astype(F32) / F32(depth)
    c[:, 1] = (F32(0.25) * counts[:, 0].astype(F32)) / F32(depth)
    return c


def pack_rgb8(acc):
    """RGBF32_to_RGB8 (template/precomp.h:441-444): trunc(255 * min(1, c)) per channel, 0x00RRGGBB"""
    ch = (F32(255) * np.minimum(F32(1), acc[:, 0:3].astype(F32))).astype(F32)
    q = np.trunc(ch).astype(np.uint32)
    return (q[:, 0] << 16) + (q[:, 1] << 8) + q[:, 2]


def heat_frames(counts0, counts1, depth):
    """The three checked frames from the counts of the frame-0 and frame-1 camera rays:
    name -> (accumulator [n, 4] float32, RGB8 [n] uint32).
    reset0: frame 0, reset, spp 1 -- the colour itself; avg1: frame 1 after it, no reset -- w = 2,
    a + 0.5f * (c - a); spp2: one spp-2 frame 0, reset -- (1 / 2) * ((0 + c0) + c1)."""
    c0, c1 = heat_colour(counts0, depth), heat_colour(counts1, depth)
    n = len(c0)
    out = {}

    def acc_of(rgb, w):
        a = np.zeros((n, 4), F32)
        a[:, 0:3], a[:, 3] = rgb, F32(w)
        return a

    out["reset0"] = acc_of(c0, 1)
    out["avg1"] = acc_of((c0 + F32(0.5) * (c1 - c0)).astype(F32), 2)
    out["spp2"] = acc_of((F32(1.0) / F32(2.0)) * ((c0 + c1).astype(F32)), 1)
    return {k: (a, pack_rgb8(a)) for k, a in out.items()}


def np_areas(nodes):
    """per node: ex*ey + ey*ez + ez*ex in float64 from the float32 bounds, left to right"""
    f = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32).view(F32).reshape(-1, 8)
    e = f[:, 3:6].astype(np.float64) - f[:, 0:3].astype(np.float64)
    return (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]


def np_cost(nodes):
    """rt_bvh_cost restated: the double sums through math.fsum (exactly rounded)"""
    u = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32).view(np.uint32).reshape(-1, 8)
    area = np_areas(nodes)
    keep = np.arange(len(u)) != 1
    cnt = u[:, 7]
    leaf, inner = keep & (cnt > 0), keep & (cnt == 0)
    c = {"interior_area": math.fsum(area[inner]), "leaf_area": math.fsum(area[leaf]),
         "leaf_cost": math.fsum(cnt[leaf].astype(np.float64) * area[leaf]), "root_area": float(area[0]),
         "interiors": int(inner.sum()), "leaves": int(leaf.sum()), "refs": int(cnt[leaf].sum()),
         "max_leaf": int(cnt[leaf].max()) if leaf.any() else 0}
    c["sah"] = 0.0 if c["root_area"] == 0 else (c["interior_area"] + c["leaf_cost"]) / c["root_area"]
    return c


INT_FIELDS = ("interiors", "leaves", "refs", "max_leaf")
SUM_FIELDS = ("interior_area", "leaf_area", "leaf_cost")


def assert_cost_close(got, want, nodes_used):
    """integers exact; each double sum within nodes_used * 2^-53 relative -- the terms are non-negative,
    so that is the worst case of any summation order against the exact sum; sah = (interior_area +
    leaf_cost) / root_area is one such sum (same bound: its terms are non-negative too) through one more
    addition and one division on each side, four roundings of 2^-53 in all"""
    for k in INT_FIELDS:
        assert got[k] == want[k], (k, got[k], want[k])
    rel = nodes_used * 2.0 ** -53
    for k in SUM_FIELDS:
        assert abs(got[k] - want[k]) <= rel * abs(want[k]), (k, got[k], want[k])
    assert got["root_area"] == want["root_area"]
    assert abs(got["sah"] - want["sah"]) <= (rel + 2.0 ** -51) * abs(want["sah"]), (got["sah"], want["sah"])


def tree_cases(rt):
    """name -> (prims, materials, prebuilt (nodes, indices) or None, bvh_kind): the four cases of
    refit_util.scene_cases, an SBVH of the teapot, and the animated room (a cube, a quad, planes)"""
    out = {k: (p, m, b, rt.BVH_PLAIN) for k, (p, m, b) in scene_cases(rt).items()}
    tp, tm, _, _ = out["teapotF"]
    out["sbvh"] = (tp, tm, None, rt.BVH_SBVH)
    out["room"] = (room_prims(rt, 0.7), room_mats(rt), None, rt.BVH_PLAIN)
    return out


def host_nodes(rt, case):
    prims, _, bvh, kind = case
    if kind == rt.BVH_SBVH:
        return rt.build_sbvh_host(prims)[0]
    return tree_of(rt, prims, bvh)[0]


def probe_rays(nodes, cam_rays, kat):
    """The camera rays, the known-answer rays, and rays made for this tree's root box: axis-parallel
    ones with zero direction components (infinite rD, and 0 * inf = NaN where the origin lies on a slab
    plane), rays starting inside the root box, and rays whose tmax ends inside the tree so that
    tmin < ray.t decides.  Shuffled with a fixed seed, so every leading batch mixes the kinds."""
    f = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32).view(F32).reshape(-1, 8)
    lo, hi = np.clip(f[0, 0:3], -8, 8).astype(F32), np.clip(f[0, 3:6], -8, 8).astype(F32)
    mid, ext = ((lo + hi) * F32(0.5)).astype(F32), (hi - lo).astype(F32)
    R = []
    for ax in range(3):
        for sgn in (1.0, -1.0):
            d = np.zeros(3, F32)
            d[ax] = sgn
            for o in (mid, lo, hi, mid + F32(0.25) * ext):     # through the middle, along slab planes
                o = np.array(o, F32)
                o[ax] = mid[ax] - F32(sgn) * (ext[ax] + F32(1))
                R.append(np.concatenate([o, d, [F32(1e34)]]))
            d2 = d.copy()
            d2[ax] = -0.0 if sgn < 0 else 0.0                  # +-0 in one component, the others alive
            d2[(ax + 1) % 3], d2[(ax + 2) % 3] = 0.6, 0.8
            R.append(np.concatenate([lo, d2, [F32(1e34)]]))
    rng = np.random.default_rng(77)
    D = rng.normal(size=(24, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F32)
    inside = mid + (rng.uniform(-0.45, 0.45, (24, 3)) * ext).astype(F32)
    R += [np.concatenate([o, d, [F32(1e34)]]) for o, d in zip(inside, D)]
    special = np.array(R, F32)
    short = cam_rays[::5].copy()
    short[:, 6] = rng.uniform(0.5, 8.0, len(short)).astype(F32)
    kshort = kat[::40].copy()
    kshort[:, 6] = rng.uniform(0.0, 9.0, len(kshort)).astype(F32)
    rays = np.concatenate([special, cam_rays, short, kat, kshort], 0).astype(F32)
    return np.ascontiguousarray(rays[np.random.default_rng(5).permutation(len(rays))])
