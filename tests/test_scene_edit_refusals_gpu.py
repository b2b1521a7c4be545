"""The order of the scene-edit refusals where it depends on the scene: inputs for which two refusals hold
at once, on a plain and an SBVH build of one tiny scene (and a plain one whose sphere's box is infinite),
through the device form and the _host form of every entry point.  Code and full rt_last_error() text.

The _host forms report null, empty and range under their own name before the scene's kind is looked at and
everything later under the device form's name; the splice and compact routes check everything under the
name they were called by.  Every case is refused on the host: no kernel is launched, no frame, no renderer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SBVH = "an SBVH scene (leaves share primitives) cannot be refitted"
RANGE = "range outside the primitives"
BOX = "a primitive's box is NaN or infinite"
KIND = "primitive 7 is not a triangle"


def tiny(rt, radius=0.4):
    """0 the light, 1-6 triangles (two long diagonals across four small ones), 7 a sphere"""
    prims = [rt.sphere((0, 4, -2), 0.5, 0),
             rt.triangle((-4, -4, 5), (4, 4, 5), (4, 4.1, 5), 1), rt.triangle((-4, 4, 5), (4, -4, 5), (4, -4.1, 5), 1)]
    prims += [rt.triangle((x, y, 5), (x + .3, y, 5), (x, y + .3, 5), 1) for x, y in ((-3, 0), (3, 0), (0, 3), (0, -3))]
    prims += [rt.sphere((2, -2, 4), radius, 1)]
    mats = [rt.material(rt.LIGHT, (24, 24, 22)), rt.material(rt.DIFFUSE, (0.8, 0.6, 0.5))]
    return prims, mats


def test_two_refusals_at_once_keep_their_order(rt):
    import torch
    L = rt.lib()
    INV, UNS, OK = rt.RT_ERR_INVALID, rt.RT_ERR_UNSUPPORTED, rt.RT_OK
    prims, mats = tiny(rt)
    P = rt.Scene(prims, mats)
    S = rt.Scene(prims, mats, bvh_kind=rt.BVH_SBVH)
    N = rt.Scene(*tiny(rt, float("inf")))
    assert P.info["num_refs"] == 8 and S.info["num_refs"] != 8 and N.info["num_refs"] == 8
    infos = [g.info for g in (P, S, N)]

    buf = torch.zeros(256, dtype=torch.float32, device="cuda:0")      # never read: every call is refused before a launch
    dev = C.c_void_p(buf.data_ptr())
    verts = (C.c_float * 36)()
    recs = (rt.Prim * 4)(*([prims[1]] * 4))
    T = (C.c_float * 64)()
    imats = (C.c_int32 * 16)()
    keep = (C.c_uint8 * 8)(*([1] * 8))
    ticket = C.c_uint64(0)
    M = (C.c_float * 16)(*[1.0 if i % 5 == 0 else 0.0 for i in range(16)])

    def xf(*rows):
        return (rt.TriXform * len(rows))(*[rt.TriXform(f, n, M) for f, n in rows]), len(rows)

    def ed(*rows, prim=False):
        a = (rt.TriEdit * len(rows))(*[rt.TriEdit(*r) for r in rows])
        return (C.cast(a, C.POINTER(rt.PrimEdit)) if prim else a), len(rows)

    cases = []   # (scene, entry point, arguments, code, text or None)

    def add(g, name, args, code, said_by=None, body=None):
        cases.append((g, name, args, code, None if body is None else (said_by or name) + ": " + body))

    for form, tail in (("", (None,)), ("_async", (None, C.byref(ticket)))):
        ut, up, tt = "rt_scene_update_triangles" + form, "rt_scene_update_prims" + form, "rt_scene_transform_triangles" + form
        # SBVH and a range outside; SBVH and a non-triangle in the range: the scene's kind first
        for first, count in ((7, 2), (6, 2)):
            add(S, ut, (first, count, dev) + tail, UNS, body=SBVH)
            add(S, up, (first, count, dev, None) + tail, UNS, body=SBVH)
            add(S, tt, xf((first, count)) + (dev,) + tail, UNS, body=SBVH)
        add(S, tt, xf((1, 3), (3, 2)) + (None,) + tail, UNS, body=SBVH)            # ... before overlap and null rest
        # the plain scene: the range before the kind
        add(P, ut, (7, 2, dev) + tail, INV, body=RANGE)
        add(P, ut, (6, 2, dev) + tail, INV, body=KIND)
        add(P, up, (7, 2, dev, None) + tail, INV, body=RANGE)
        add(P, tt, xf((1, 2), (2, 0), (6, 3)) + (dev,) + tail, INV, body="range 2 outside the primitives")   # the caller's numbering
        add(P, tt, xf((6, 2), (1, 3), (3, 2)) + (None,) + tail, INV, body=KIND)    # the kind before overlap and null rest
        # null rest and overlapping ranges: the overlap first, in either order; null rest last
        add(P, tt, xf((1, 3), (3, 2)) + (None,) + tail, INV, body="ranges overlap")
        add(P, tt, xf((3, 2), (1, 3)) + (None,) + tail, INV, body="ranges overlap")
        add(P, tt, xf((3, 2), (1, 2)) + (None,) + tail, INV, body="null rest vertices")
        add(P, tt, xf((3, 0), (1, 0)) + (None,) + tail, OK)                        # nothing to do, null rest or not
    add(S, "rt_scene_update_prims_async", (0, 2, dev, None, None, C.byref(ticket)), UNS, body=SBVH)
    add(P, "rt_scene_update_prims_async", (0, 9, dev, None, None, C.byref(ticket)), INV, body=RANGE)       # the range before the light
    add(P, "rt_scene_update_prims_async", (0, 2, dev, None, None, C.byref(ticket)), UNS,
        body="the range holds primitive 0 (the light moves through rt_scene_update_prims)")
    # the _host update forms: the range under their own name, what follows under the device form's
    add(S, "rt_scene_update_triangles_host", (7, 2, verts), INV, body=RANGE)
    add(S, "rt_scene_update_triangles_host", (6, 2, verts), UNS, "rt_scene_update_triangles", SBVH)
    add(P, "rt_scene_update_triangles_host", (6, 2, verts), INV, "rt_scene_update_triangles", KIND)
    add(S, "rt_scene_update_prims_host", (7, 2, recs, T), INV, body=RANGE)
    add(S, "rt_scene_update_prims_host", (6, 2, recs, T), UNS, "rt_scene_update_prims", SBVH)
    add(S, "rt_scene_update_prims_host", (6, 2, recs, None), UNS, "rt_scene_update_prims", SBVH)

    for g, body in ((S, SBVH), (N, BOX)):
        add(g, "rt_scene_rebuild", (None,), UNS, body=body)
    add(S, "rt_scene_prepare_updates", (None,), UNS, body=SBVH)

    # the rebuild routes: the range, then the scene's kind, then its boxes, then the primitives' kind
    for form, d, tail in (("", dev, (None,)), ("_host", recs, ())):
        st = "rt_scene_splice_triangles" + form
        for g in (S, N, P):
            add(g, st, (7, 2, None, 0) + tail, INV, body=RANGE)
            add(g, st, (0, 9, None, 1) + tail, INV, body="first = 0 (primitive 0 is the light and stays)")
            add(g, st, (3, 0, None, 0) + tail, OK)                                  # nothing to do
        add(S, st, (6, 2, d, 1) + tail, UNS, body=SBVH)
        add(N, st, (6, 2, d, 1) + tail, UNS, body=BOX)
        add(P, st, (6, 2, d, 1) + tail, INV, body=KIND)
        for route, prim, extra in (("rt_scene_splice_ranges", False, ()), ("rt_scene_splice_prims", True, (None,))):
            sr = route + form
            for g in (S, N, P):
                add(g, sr, ed((2, 1, 0), (7, 2, 0), prim=prim) + (d,) + extra + tail, INV, body="edit 1: " + RANGE)
                add(g, sr, ed((7, 2, 0), (2, 2, 0), (3, 1, 1), prim=prim) + (d,) + extra + tail, INV,
                    body="edit 2: its removed range overlaps another edit's")    # the overlap before the range
                add(g, sr, ed((3, 0, 0), prim=prim) + (None,) + extra + tail, OK)
            add(S, sr, ed((6, 2, 1), prim=prim) + (d,) + extra + tail, UNS, body=SBVH)
            add(N, sr, ed((6, 2, 1), prim=prim) + (d,) + extra + tail, UNS, body=BOX)
            if not prim:
                add(P, sr, ed((2, 1, 0), (6, 2, 1)) + (d,) + tail, INV, body=KIND)
        for route in ("rt_scene_compact_triangles", "rt_scene_compact_prims"):
            k = dev if form == "" else keep
            add(S, route + form, (k,) + tail, UNS, body=SBVH)
            add(N, route + form, (k,) + tail, UNS, body=BOX)
            add(S, route + form, (None,) + tail, INV, body="null mask")
        sm = "rt_scene_set_prim_materials" + form
        m = dev if form == "" else imats
        for g in (S, P):
            add(g, sm, (0, 9, m) + tail, INV, body="the range holds primitive 0 (the light's material stays)")
            add(g, sm, (7, 2, m) + tail, INV, body=RANGE)
            add(g, sm, (0, 9, None) + tail, INV, body="null materials")

    for g, name, args, code, text in cases:
        rc = getattr(L, name)(g.h, *args)
        msg = L.rt_last_error().decode()
        print(name, "SBVH" if g is S else "infinite" if g is N else "plain", rc, msg if rc else "")
        assert rc == code and (text is None or msg == text), (name, rc, msg, code, text)
    assert ticket.value == 0
    st = rt.UpdateStatus()
    for g, info in zip((P, S, N), infos):
        assert L.rt_scene_update_sync(g.h, C.byref(st)) == OK and st.submitted == 0
        assert g.info == info
        g.close()
    assert float(buf.sum()) == 0.0
    assert np.all(np.frombuffer(keep, np.uint8) == 1)
