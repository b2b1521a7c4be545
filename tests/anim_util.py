"""Scenes of the every-primitive update tests (test_prim_records_host.py, test_update_prims_gpu.py):
the reference's animated room -- its root scene.h:264-281 with SetTime's three movers (scene.h:286-304:
the swinging quad light, the spinning cube, the bouncing sphere) -- plus two triangles."""
import numpy as np

MOVERS = (0, 1, 3)          # the quad light, the bouncing sphere, the spinning cube
TIMES = (0.0, 0.7, 1.3, 2.9)


def room_mats(rt):
    return [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.DIFFUSE, (0.8, 0.7, 0.6)),
            rt.material(rt.MIRROR, (0.9, 0.9, 0.9)), rt.material(rt.DIFFUSE, (0.3, 0.5, 0.9))]


def room_prims(rt, t):
    """The room at SetTime(t): 0 the quad light, 1 the bouncing sphere, 2 the corner sphere, 3 the
    cube, 4-9 the walls, 10-11 two triangles.  float32 throughout, matrices through rt.mat4_*."""
    f = np.float32
    t = f(t)
    M1 = rt.mat4_mul(rt.mat4_translate(0, 2.6, 2), rt.mat4_rotate(2, f(np.sin(t * f(0.6))) * f(0.1)),
                     rt.mat4_translate(0, -0.9, 0))
    M2base = rt.mat4_mul(rt.mat4_rotate(0, f(np.pi) / f(4)), rt.mat4_rotate(2, f(np.pi) / f(4)))
    M2 = rt.mat4_mul(rt.mat4_translate(1.4, 0, 2), rt.mat4_rotate(1, t * f(0.5)), M2base)
    tm = f(1) - (f(np.fmod(t, f(2.0))) - f(1)) ** 2
    prims = [rt.quad(1.0, 0, M1),
             rt.sphere((-1.4, f(-0.5) + f(tm), 2.0), 0.5, 2),
             rt.sphere((0, 2.5, -3.07), 8.0, 1),
             rt.cube((0, 0, 0), 1.15, 3, M2),
             rt.plane((1, 0, 0), 3.0, 1), rt.plane((-1, 0, 0), 2.99, 1), rt.plane((0, 1, 0), 1.0, 1),
             rt.plane((0, -1, 0), 2.0, 1), rt.plane((0, 0, 1), 3.0, 1), rt.plane((0, 0, -1), 3.99, 1),
             rt.triangle((-0.6, -1.0, 2.6), (0.4, -1.0, 2.9), (-0.1, 0.1, 3.2), 3),
             rt.triangle((0.2, -0.9, 1.2), (0.9, -0.95, 1.4), (0.5, -0.2, 1.1), 1)]
    return prims


def split_tree(rt, prims):
    """A prebuilt tree (nodes [n, 32] uint8, indices) that keeps the unbounded planes in one leaf and
    gives the bounded primitives the builder's tree over them alone: root -> (planes' leaf, that
    tree).  The builder's own tree of such a scene mixes a plane into every leaf, so every box is
    +-1e30 and a refit has nothing to move."""
    planes = [i for i, p in enumerate(prims) if p.type == rt.PLANE]
    rest = [i for i, p in enumerate(prims) if p.type != rt.PLANE]
    sub, sidx, _ = rt.build_bvh_host([prims[i] for i in rest])
    su = sub.view(np.uint32).reshape(-1, 8)
    m = len(su)
    u = np.zeros((m + 2, 8), np.uint32)
    u[0, 6:8] = (2, 0)
    u[2, 6:8] = (0, len(planes))
    for k in [0] + list(range(2, m)):
        lf, cnt = int(su[k, 6]), int(su[k, 7])
        u[3 if k == 0 else k + 2, 6:8] = (lf + len(planes), cnt) if cnt else (lf + 2, 0)
    idx = np.array(planes + [rest[int(i)] for i in sidx], np.uint32)
    return rt.refit_bvh_host(prims, u.view(np.uint8).reshape(-1, 32), idx), idx


def with_prims(base, first, new):
    """base with primitives [first, first + len(new)) replaced"""
    out = list(base)
    out[first:first + len(new)] = list(new)
    return out
