"""Scene.update_triangles on the GPU: in-place triangle updates with a bottom-up BVH refit.

A refit keeps the topology and recomputes boxes as min / max of floats, so nothing rounds: the
refitted node array must equal rt_bvh_refit_host's and the numpy restatement byte for byte, and an
updated scene must equal the oracle holding the same primitives over the same tree bit for bit --
hit ids, t / u / v bits, occlusion, RGB8 frames and accumulator bits, no tie allowance.  Scenes:
the KAT scene (smaller than one treelet), a light and two triangles (the root is a leaf), the
64-level chain (64 heights, one leaf per level) and TEAPOT-F (many treelets plus nodes above the cut)."""
import numpy as np
import pytest

from refit_util import (mixed_leaves, numpy_refit, scene_cases, tree_of, triangle_ids, twist, verts_of, with_verts)
from scenes_util import kat_rays, oracle_scene, sticky_prims

pytestmark = pytest.mark.gpu

W, H = 160, 96
NAMES = ["kat", "leaf", "chain", "teapotF"]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cases(rt):
    return scene_cases(rt)


@pytest.fixture(scope="module")
def specs(rt):
    """(mode, depth, spp): primary + shadow, Whitted depth 4, path depth 4 x 2 spp"""
    return [(rt.MODE_PATH, 1, 1), (rt.MODE_WHITTED, 4, 1), (rt.MODE_PATH, 4, 2)]


def runs(ids):
    """contiguous runs [(first, count)] of a sorted id list"""
    out = []
    for i in ids:
        if out and out[-1][0] + out[-1][1] == i:
            out[-1][1] += 1
        else:
            out.append([int(i), 1])
    return [(a, b) for a, b in out]


def update(g, prims, ids, device=None):
    """new vertices for the listed triangles, one call per contiguous run; device: a torch module to
    pass device tensors, else numpy arrays"""
    for first, count in runs(ids):
        v = verts_of(prims, range(first, first + count))
        if device is not None:
            v = device.from_numpy(v).to(f"cuda:{g.device}")
        g.update_triangles(first, v)


def gpu_frames(rt, g, specs, renderers=None):
    """[(rgb8, accumulator)] per spec, frame 0 with reset; renderers: reuse these (one per spec)"""
    out = []
    for k, (mode, depth, spp) in enumerate(specs):
        r = renderers[k] if renderers else rt.Renderer(g, W, H)
        r.mode = mode
        rgb = r.tick_host(spp=spp, depth=depth, frame=0, reset=True)
        out.append((rgb.copy(), r.accumulator().copy()))
        if not renderers:
            r.close()
    return out


def oracle_frames(o, specs):
    out = []
    for mode, depth, spp in specs:
        o.set_integrator(mode)
        acc = np.zeros((W * H, 4), np.float32)
        rgb, _ = o.tick(W, H, acc, spp=spp, depth=depth, frame=0)
        out.append((rgb, acc))
    o.set_integrator(0)
    return out


def assert_frames_equal(got, want):
    for k, ((grgb, gacc), (wrgb, wacc)) in enumerate(zip(got, want)):
        assert np.array_equal(grgb, wrgb), f"spec {k}: {(grgb != wrgb).sum()} RGB8 pixels differ"
        bad = (gacc.reshape(-1, 4).view(np.uint32) != wacc.reshape(-1, 4).view(np.uint32)).any(axis=1)
        assert not bad.any(), f"spec {k}: {bad.sum()} accumulator pixels differ in their bits"


def assert_hits_equal(g, o, rays):
    gt, go, gu, gv = (x.cpu().numpy() for x in g.IntersectBVH(rays))
    ot, oo, ou, ov = o.intersect(rays)
    assert np.array_equal(go, oo), f"{(go != oo).sum()} ids differ"
    assert np.array_equal(gt.view(np.uint32), ot.view(np.uint32)), "t bits differ"
    hit = oo >= 0
    assert np.array_equal(gu[hit].view(np.uint32), ou[hit].view(np.uint32))
    assert np.array_equal(gv[hit].view(np.uint32), ov[hit].view(np.uint32))


def random_rays(n, seed):
    rng = np.random.default_rng(seed)
    O = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    D[: n // 16, 1] = 0.0
    return np.concatenate([O, D, np.full((n, 1), 1e34, np.float32)], axis=1).astype(np.float32)


def assert_rays_equal(g, o, extra=()):
    """camera rays, 20k random rays, the KAT rays (+ extra): closest hits and occlusion"""
    cam = o.camera_rays(W, H, np.arange(W * H, dtype=np.int32))
    for k, rays in enumerate((cam, random_rays(20000, 5), kat_rays()) + tuple(extra)):
        assert_hits_equal(g, o, rays)
        short = rays.copy()
        short[:, 6] = np.random.default_rng(9 + k).uniform(0.0, 8.0, len(rays)).astype(np.float32)
        assert np.array_equal(g.IsOccluded(short).cpu().numpy(), o.occluded(short).astype(bool))


@pytest.mark.parametrize("name", NAMES)
def test_update_with_own_vertices_changes_nothing(rt, torch, cases, specs, name):
    prims, mats, bvh = cases[name]
    nodes, idx = tree_of(rt, prims, bvh)
    g, twin = rt.Scene(prims, mats, bvh=bvh), rt.Scene(prims, mats, bvh=bvh)
    rs = [rt.Renderer(g, W, H) for _ in specs]
    gpu_frames(rt, g, specs, rs)                     # the renderers have run before the update
    update(g, prims, triangle_ids(rt, prims), device=torch)
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    assert np.array_equal(g.bvh()[1], idx)
    assert_frames_equal(gpu_frames(rt, g, specs, rs), gpu_frames(rt, twin, specs))
    for r in rs:
        r.close()


@pytest.mark.parametrize("name", NAMES)
def test_full_deformation_equals_oracle_on_the_refitted_tree(rt, oracle, torch, cases, specs, name):
    prims, mats, bvh = cases[name]
    nodes, idx = tree_of(rt, prims, bvh)
    ids = triangle_ids(rt, prims)
    moved = with_verts(rt, prims, ids, twist(verts_of(prims, ids), 0.6))
    g = rt.Scene(prims, mats, bvh=bvh)
    update(g, moved, ids, device=torch)
    host = rt.refit_bvh_host(moved, nodes, idx)
    assert host.tobytes() != nodes.tobytes()
    assert g.bvh()[0].tobytes() == host.tobytes()
    assert host.tobytes() == numpy_refit(rt, moved, nodes, idx).tobytes()
    o = oracle_scene(rt, oracle, moved, mats, bvh=(host, idx))
    assert_rays_equal(g, o)
    assert_frames_equal(gpu_frames(rt, g, specs), oracle_frames(o, specs))


def leaf_mates(nodes, idx):
    """primitive id -> the ids sharing its leaf"""
    u = nodes.view(np.uint32).reshape(-1, 8)
    out, st = {}, [0]
    while st:
        k = st.pop()
        if u[k, 7] == 0:
            st += [int(u[k, 6]), int(u[k, 6]) + 1]
            continue
        members = [int(i) for i in idx[int(u[k, 6]):int(u[k, 6]) + int(u[k, 7])]]
        for i in members:
            out[i] = members
    return out


def aimed_rays(verts):
    """one ray per triangle ([n, 9] vertices): from 0.05 in front of its centroid, along its normal"""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    ctr = v.mean(axis=1)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ok = np.linalg.norm(nrm, axis=1) > 0             # a mesh may hold degenerate triangles
    v, ctr, nrm = v[ok], ctr[ok], nrm[ok]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([ctr - 0.05 * nrm, nrm, np.full((len(v), 1), 1e34)], axis=1).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
def test_partial_range(rt, oracle, cases, name):
    """A range that starts and ends inside leaves (where the tree has leaves of several triangles) and,
    on TEAPOT-F, spans more triangles than a treelet has nodes: the updated scene equals the oracle
    on (moved range + untouched rest) over the refitted tree, also for rays aimed at the untouched
    triangles."""
    prims, mats, bvh = cases[name]
    nodes, idx = tree_of(rt, prims, bvh)
    tri = triangle_ids(rt, prims)
    lo, hi = int(tri[0]), int(tri[-1]) + 1
    assert np.array_equal(tri, np.arange(lo, hi))
    first, end = {"kat": (2, 4), "leaf": (2, 3), "chain": (10, 40)}.get(name, (lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3))
    if name == "teapotF":
        mates = leaf_mates(nodes, idx)
        while not any(lo <= m < first for m in mates[first]):
            first += 1
        while not any(end <= m < hi for m in mates[end - 1]):
            end += 1
        assert end - first > 256 and first > lo and end < hi
    ids = np.arange(first, end)
    if name in ("leaf", "teapotF"):
        assert mixed_leaves(nodes, idx, ids) >= (1 if name == "leaf" else 2)
    moved = with_verts(rt, prims, ids, twist(verts_of(prims, ids), -0.8))
    g = rt.Scene(prims, mats, bvh=bvh)
    update(g, moved, ids)                            # numpy vertices: the staged path
    host = rt.refit_bvh_host(moved, nodes, idx)
    assert g.bvh()[0].tobytes() == host.tobytes()
    o = oracle_scene(rt, oracle, moved, mats, bvh=(host, idx))
    rest = np.setdiff1d(tri, ids)[:3000]
    aimed = aimed_rays(verts_of(moved, rest))
    assert_rays_equal(g, o, extra=(aimed,))
    _, obj, _, _ = o.intersect(aimed)
    assert np.isin(obj, rest).mean() > 0.9           # the answers are the untouched triangles
    assert_frames_equal(gpu_frames(rt, g, [(rt.MODE_PATH, 1, 1)]), oracle_frames(o, [(rt.MODE_PATH, 1, 1)]))


def test_sticky_boxes_are_recomputed(rt, cases):
    """One TEAPOT-F triangle squashed into a sliver (sine under 2^-8), another squashed and then
    restored: the wave walk's counters (rays walked, boxes entered through the cull margin, lanes
    re-traced) equal those of a scene created fresh from the same primitives over the same refitted
    tree, no verified lane differs, and the frames are equal."""
    prims, mats, _ = cases["teapotF"]
    nodes, idx, _ = rt.build_bvh_host(prims)
    tri = triangle_ids(rt, prims)
    x, y = int(tri[len(tri) // 4]), int(tri[(3 * len(tri)) // 4])

    def squash(i):
        v = verts_of(prims, [i]).reshape(3, 3)
        mid = (v[0] + v[1]) * np.float32(0.5)
        v[2] = mid + (v[2] - mid) * np.float32(1e-4)
        return v.reshape(1, 9)

    both = with_verts(rt, with_verts(rt, prims, [x], squash(x)), [y], squash(y))
    final = with_verts(rt, prims, [x], squash(x))
    assert not sticky_prims(rt, prims)[[x, y]].any()
    assert sticky_prims(rt, both)[[x, y]].all()
    st = sticky_prims(rt, final)
    assert st[x] and not st[y]
    g = rt.Scene(prims, mats)
    update(g, both, [x, y])
    update(g, final, [y])
    refit = rt.refit_bvh_host(final, nodes, idx)
    assert g.bvh()[0].tobytes() == refit.tobytes()
    fresh = rt.Scene(final, mats, bvh=(refit, idx))
    res = []
    for s in (g, fresh):
        s.set_camera_walk(rt.WALK_WAVE)
        r = rt.Renderer(s, W, H)
        r.set_walk_check(rt.WALK_CHECK_VERIFY)
        rgb = r.tick_host(spp=1, depth=1, frame=0, reset=True)
        res.append((rgb, r.accumulator(), r.walk_stats()))
        r.close()
    (rgb0, acc0, ws0), (rgb1, acc1, ws1) = res
    print("walk stats (updated, fresh):", ws0, ws1)
    assert ws0["walked"] > 0
    assert [ws0[k] for k in ("walked", "margin_boxes", "retraced")] == [ws1[k] for k in ("walked", "margin_boxes", "retraced")]
    assert ws0["verify_mismatch"] == 0 and ws1["verify_mismatch"] == 0
    assert_frames_equal([(rgb0, acc0)], [(rgb1, acc1)])


def test_errors_leave_the_scene_untouched(rt, torch, cases):
    prims, mats, _ = cases["teapotF"]
    g = rt.Scene(prims, mats)
    tri = triangle_ids(rt, prims)
    spec = [(rt.MODE_PATH, 1, 1)]
    nodes0, frame0 = g.bvh()[0].copy(), gpu_frames(rt, g, spec)
    first = int(tri[10])
    good = twist(verts_of(prims, range(first, first + 50)), 0.5)
    for poison in (np.nan, np.inf, -np.inf):
        for dev in (False, True):
            v = good.copy()
            v[37, 4] = poison
            with pytest.raises(rt.RTError) as e:
                g.update_triangles(first, torch.from_numpy(v).to(f"cuda:{g.device}") if dev else v)
            assert e.value.code == rt.RT_ERR_INVALID
    assert g.bvh()[0].tobytes() == nodes0.tobytes()
    assert_frames_equal(gpu_frames(rt, g, spec), frame0)
    assert prims[0].type != rt.TRIANGLE
    for bad_first, count in ((0, 2), (len(prims) - 1, 2), (len(prims), 1)):
        with pytest.raises(rt.RTError) as e:         # the light in the range; a range past the end
            g.update_triangles(bad_first, np.zeros((count, 9), np.float32))
        assert e.value.code == rt.RT_ERR_INVALID
    g.update_triangles(first, np.zeros((0, 9), np.float32))      # count 0: a no-op
    g.update_triangles(first, torch.zeros((0, 9), device=f"cuda:{g.device}"))
    assert g.bvh()[0].tobytes() == nodes0.tobytes()
    assert_frames_equal(gpu_frames(rt, g, spec), frame0)
    sb = rt.Scene(prims, mats, bvh_kind=rt.BVH_SBVH)
    assert sb.info["num_refs"] != sb.info["num_prims"]
    with pytest.raises(rt.RTError) as e:
        sb.update_triangles(first, good)
    assert e.value.code == rt.RT_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", NAMES)
def test_there_and_back(rt, cases, name):
    prims, mats, bvh = cases[name]
    nodes, idx = tree_of(rt, prims, bvh)
    ids = triangle_ids(rt, prims)
    moved = with_verts(rt, prims, ids, twist(verts_of(prims, ids), 1.1))
    g = rt.Scene(prims, mats, bvh=bvh)
    spec = [(rt.MODE_PATH, 1, 1), (rt.MODE_PATH, 4, 2)]
    rs = [rt.Renderer(g, W, H) for _ in spec]
    before = gpu_frames(rt, g, spec, rs)
    update(g, moved, ids)
    assert g.bvh()[0].tobytes() == rt.refit_bvh_host(moved, nodes, idx).tobytes()
    update(g, prims, ids)
    assert g.bvh()[0].tobytes() == nodes.tobytes()
    assert_frames_equal(gpu_frames(rt, g, spec, rs), before)
    for r in rs:
        r.close()
