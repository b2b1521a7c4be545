"""Helpers of the refit tests (test_refit_host.py, test_refit_gpu.py): the scenes, a deformation
that is a pure function of a vertex's position, and the refit restated in numpy.

A refit keeps the tree's topology and recomputes boxes only: a leaf's box is the float32 min / max
over its primitives' boxes (a triangle's: min / max of its three vertices), an interior node's the
union of its children's.  min / max never round, so the library's host refit, its device refit and
this one must agree byte for byte."""
import numpy as np

from scenes_util import chain_scene, kat_scene


def scene_cases(rt):
    """name -> (prims, materials, prebuilt bvh or None): smaller than one treelet; a root that is
    a leaf; 64 heights with one leaf per level; many treelets plus nodes above the cut."""
    mats = [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.DIFFUSE, (0.8, 0.6, 0.5))]
    leaf = [rt.sphere((0, 4, -2), 0.5, 0),
            rt.triangle((-1.0, -0.5, 3.0), (1.0, -0.5, 3.0), (0.0, 1.0, 3.5), 1),
            rt.triangle((-1.5, -1.0, 4.0), (0.5, 1.5, 4.5), (1.5, -1.0, 4.0), 1)]
    kp, km = kat_scene(rt)
    cp, cm, cb = chain_scene(rt, 64)
    tp, tm = rt.recipe_describe("teapotF")
    # the builder would split these three; a prebuilt tree of one leaf (node 1 is the unused one)
    root = np.zeros((2, 32), np.uint8)
    root.view(np.uint32).reshape(-1, 8)[0, 6:8] = (0, 3)
    lidx = np.arange(3, dtype=np.uint32)
    lb = (numpy_refit(rt, leaf, root, lidx), lidx)
    return {"kat": (kp, km, None), "leaf": (leaf, mats, lb), "chain": (cp, cm, cb), "teapotF": (tp, tm, None)}


def tree_of(rt, prims, bvh):
    """(nodes [n, 32] uint8, indices) of a case: its prebuilt tree or the host builder's"""
    if bvh is not None:
        return np.ascontiguousarray(bvh[0], np.uint8), np.ascontiguousarray(bvh[1], np.uint32)
    nodes, idx, _ = rt.build_bvh_host(prims)
    return nodes, idx


def triangle_ids(rt, prims):
    return np.array([i for i, p in enumerate(prims) if p.type == rt.TRIANGLE], np.int64)


def verts_of(prims, ids):
    """[len(ids), 9] float32: A, B, C of the listed triangles"""
    return np.array([[prims[i].v[k] for k in range(9)] for i in ids], np.float32).reshape(-1, 9)


def twist(verts, k):
    """A twist about the y axis by k radians per unit of y, per vertex, rounded to float32: a pure
    function of the vertex position, so vertices shared between triangles stay shared."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    a = k * v[:, 1]
    c, s = np.cos(a), np.sin(a)
    out = np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], axis=1)
    return out.astype(np.float32).reshape(np.shape(verts))


def with_verts(rt, prims, ids, verts):
    """The primitive list with the listed triangles' vertices replaced (materials kept)."""
    out = list(prims)
    for i, v in zip(ids, np.asarray(verts, np.float32).reshape(-1, 9)):
        out[i] = rt.triangle(v[0:3], v[3:6], v[6:9], prims[i].material)
    return out


def tmin(a, b):   # the builder's fminf: a < b ? a : b (template/precomp.h:471)
    return np.where(a < b, a, b)


def tmax(a, b):
    return np.where(a > b, a, b)


def prim_box(rt, p):
    """float32 (min, max): a triangle's from its vertices, any other primitive's as the root box of
    a tree built over it alone"""
    if p.type == rt.TRIANGLE:
        v = np.array(list(p.v), np.float32).reshape(3, 3)
        return tmin(v[0], tmin(v[1], v[2])), tmax(v[0], tmax(v[1], v[2]))
    nodes, _, _ = rt.build_bvh_host([p])
    f = nodes.view(np.float32).reshape(-1, 8)
    return f[0, 0:3].copy(), f[0, 3:6].copy()


def numpy_refit(rt, prims, nodes, idx):
    out = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 32).copy()
    f, u = out.view(np.float32).reshape(-1, 8), out.view(np.uint32).reshape(-1, 8)
    order, st = [], [0]
    while st:
        k = st.pop()
        order.append(k)
        if u[k, 7] == 0:
            st += [int(u[k, 6]), int(u[k, 6]) + 1]
    for k in reversed(order):
        lf, cnt = int(u[k, 6]), int(u[k, 7])
        if cnt:
            mn, mx = np.full(3, 1e30, np.float32), np.full(3, -1e30, np.float32)
            for s in range(lf, lf + cnt):
                lo, hi = prim_box(rt, prims[int(idx[s])])
                mn, mx = tmin(mn, lo), tmax(mx, hi)
        else:
            mn, mx = tmin(f[lf, 0:3], f[lf + 1, 0:3]), tmax(f[lf, 3:6], f[lf + 1, 3:6])
        f[k, 0:3], f[k, 3:6] = mn, mx
    return out


def assert_nested(nodes):
    """every child box inside its parent's"""
    f, u = nodes.view(np.float32).reshape(-1, 8), nodes.view(np.uint32).reshape(-1, 8)
    st = [0]
    while st:
        k = st.pop()
        if u[k, 7]:
            continue
        for c in (int(u[k, 6]), int(u[k, 6]) + 1):
            assert (f[c, 0:3] >= f[k, 0:3]).all() and (f[c, 3:6] <= f[k, 3:6]).all(), (k, c)
            st.append(c)


def mixed_leaves(nodes, idx, ids):
    """leaves holding primitives both inside and outside the id set"""
    u = nodes.view(np.uint32).reshape(-1, 8)
    inside = set(int(i) for i in ids)
    n, st = 0, [0]
    while st:
        k = st.pop()
        if u[k, 7] == 0:
            st += [int(u[k, 6]), int(u[k, 6]) + 1]
            continue
        members = [int(i) in inside for i in idx[int(u[k, 6]):int(u[k, 6]) + int(u[k, 7])]]
        n += any(members) and not all(members)
    return n
