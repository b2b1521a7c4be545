"""Every scene-edit entry point of the C ABI on a null scene, without a device: the exact code and the exact
rt_last_error() text, with otherwise valid arguments and with null or empty ones.  The strings are written
out here; they are what a caller has seen since each entry point was added, and no change of the library's
layout may alter one of them."""
import ctypes as C


def test_every_edit_entry_point_refuses_a_null_scene_by_name(rt):
    L = rt.lib()
    INV = rt.RT_ERR_INVALID
    tri = rt.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), 0)
    recs = (rt.Prim * 2)(tri, tri)
    verts = (C.c_float * 18)()
    T = (C.c_float * 32)()
    mats = (C.c_int32 * 2)(0, 0)
    keep = (C.c_uint8 * 4)(1, 1, 1, 1)
    ticket = C.c_uint64(7)
    status = rt.UpdateStatus()
    M = (C.c_float * 16)(*[1.0 if i % 5 == 0 else 0.0 for i in range(16)])
    ranges = (rt.TriXform * 2)(rt.TriXform(1, 2, M), rt.TriXform(5, 0, M))

    def edits(*rows):
        return (rt.TriEdit * max(len(rows), 1))(*[rt.TriEdit(*r) for r in rows]), len(rows)

    one, n_one = edits((1, 0, 1))
    light, n_light = edits((5, 1, 0), (0, 0, 1))
    norec, n_norec = edits((5, 1, 0), (9, 0, 1))
    none, n_none = edits()

    # (entry point, arguments after the scene, message after "<entry point>: ")
    table = []
    for name, tail in (("rt_scene_update_triangles", (None,)), ("rt_scene_update_triangles_host", ()),
                       ("rt_scene_update_triangles_async", (None, C.byref(ticket)))):
        table += [(name, (1, 2, verts) + tail, "null scene"), (name, (1, 0, None) + tail, "null scene"),
                  (name, (1, 2, None) + tail, "null scene")]
    for name, tail in (("rt_scene_update_prims", (None,)), ("rt_scene_update_prims_host", ()),
                       ("rt_scene_update_prims_async", (None, C.byref(ticket)))):
        table += [(name, (1, 2, recs, T) + tail, "null scene"), (name, (1, 2, recs, None) + tail, "null scene"),
                  (name, (0, 0, None, None) + tail, "null scene")]
    for name, tail in (("rt_scene_transform_triangles", (None,)), ("rt_scene_transform_triangles_async", (None, C.byref(ticket)))):
        table += [(name, (ranges, 2, verts) + tail, "null scene"), (name, (None, 0, None) + tail, "null scene"),
                  (name, (None, 2, None) + tail, "null scene")]
    table += [("rt_scene_rebuild", (None,), "null scene"), ("rt_scene_prepare_updates", (None,), "null scene"),
              ("rt_scene_update_sync", (C.byref(status),), "null scene"), ("rt_scene_update_sync", (None,), "null scene")]
    for name, tail in (("rt_scene_splice_triangles", (None,)), ("rt_scene_splice_triangles_host", ())):
        table += [(name, (1, 0, recs, 1) + tail, "null scene"),
                  (name, (1, 0, None, 0) + tail, "null scene"),            # ... also with nothing to do
                  (name, (0, 0, recs, 1) + tail, "first = 0 (primitive 0 is the light and stays)"),
                  (name, (0, 0, None, 0) + tail, "first = 0 (primitive 0 is the light and stays)"),
                  (name, (1, 0, None, 1) + tail, "null records"),
                  (name, (0, 0, None, 1) + tail, "first = 0 (primitive 0 is the light and stays)")]   # the light before the records
    for name, tail in (("rt_scene_splice_ranges", (None,)), ("rt_scene_splice_ranges_host", ()),
                       ("rt_scene_splice_prims", (None, None)), ("rt_scene_splice_prims_host", (None,)),
                       ("rt_scene_splice_prims", (T, None)), ("rt_scene_splice_prims_host", (T,))):
        as_rows = (lambda a: C.cast(a, C.POINTER(rt.PrimEdit))) if "prims" in name else (lambda a: a)   # one layout, two names
        table += [(name, (as_rows(one), n_one, recs) + tail, "null scene"),
                  (name, (as_rows(none), n_none, None) + tail, "null scene"),
                  (name, (None, 0, None) + tail, "null scene"),
                  (name, (as_rows(light), n_light, recs) + tail, "edit 1: first = 0 (primitive 0 is the light and stays)"),
                  (name, (as_rows(norec), n_norec, None) + tail, "edit 1: null records"),
                  (name, (as_rows(light), n_light, None) + tail, "edit 1: first = 0 (primitive 0 is the light and stays)"),
                  (name, (None, 3, recs) + tail, "null edits")]
    for name, tail in (("rt_scene_compact_triangles", (None,)), ("rt_scene_compact_triangles_host", ()),
                       ("rt_scene_compact_prims", (None,)), ("rt_scene_compact_prims_host", ())):
        table += [(name, (keep,) + tail, "null scene"), (name, (None,) + tail, "null scene")]
    for name, tail in (("rt_scene_set_prim_materials", (None,)), ("rt_scene_set_prim_materials_host", ())):
        table += [(name, (1, 2, mats) + tail, "null scene"), (name, (1, 0, None) + tail, "null scene"),
                  (name, (0, 2, None) + tail, "null scene")]

    seen = set()
    for name, args, body in table:
        rc = getattr(L, name)(None, *args)
        msg = L.rt_last_error().decode()
        print(name, rc, msg)
        assert rc == INV and msg == name + ": " + body, (name, args, rc, msg)
        seen.add(name)
    assert len(seen) == 23 and ticket.value == 7
    assert L.rt_abi_version() == 4
