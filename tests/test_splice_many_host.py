"""rt_scene_splice_ranges and rt_scene_compact_triangles without a GPU.  The text their kernels run --
csrc/rt_splice.h, then the builder's csrc/rt_build.h -- runs with one lane in the kernels' launch order in
tests/cpp/splice_many_host.cpp, a stand-alone host program built with AddressSanitizer and UBSan: after
every batched edit, by ranges or by mask, the whole state equals pack_scene of the edited description
byte for byte, the two routes agree with each other and with the single splice, and every refusal leaves
every array as it was.  The argument errors that need no device are checked on the library."""
import ctypes as C
import os
import subprocess

from conftest import ROOT


def test_batched_splice_text_on_the_host(tmp_path):
    exe = tmp_path / "splice_many_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join(ROOT, "advancedgraphicsraytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", csrc, os.path.join(ROOT, "tests", "cpp", "splice_many_host.cpp")]
                   + [os.path.join(csrc, f) for f in ("rt_scene_pack.cpp", "rt_host.cpp", "rt_sbvh.cpp")]
                   + ["-lz", "-pthread", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "advancedgraphicsraytracer_amd", "data")],
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "splice_many_host ok" in r.stdout, r.stdout + r.stderr


def test_symbols_and_the_argument_errors_that_need_no_device(rt):
    L = rt.lib()
    for name in ("rt_scene_splice_ranges", "rt_scene_splice_ranges_host", "rt_scene_compact_triangles",
                 "rt_scene_compact_triangles_host"):
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert hasattr(rt.Scene, "splice_ranges") and hasattr(rt.Scene, "compact_triangles")
    assert C.sizeof(rt.TriEdit) == 12

    tri = rt.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), 0)
    recs = (rt.Prim * 2)(tri, tri)

    def both(edits, recs):
        """(code, message) of the device and the host entry point on a null scene"""
        arr = (rt.TriEdit * max(len(edits), 1))(*[rt.TriEdit(*e) for e in edits])
        out = []
        for call in (lambda: L.rt_scene_splice_ranges(None, arr, len(edits), recs, None),
                     lambda: L.rt_scene_splice_ranges_host(None, arr, len(edits), recs)):
            rc = call()
            out.append((rc, L.rt_last_error().decode()))
        return out

    for rc, msg in both([(1, 0, 1)], recs):                       # a null scene
        assert rc == rt.RT_ERR_INVALID and "null scene" in msg
    for rc, msg in both([], None):                                # ... also with nothing to do
        assert rc == rt.RT_ERR_INVALID and "null scene" in msg
    for rc, msg in both([(5, 1, 0), (0, 0, 1)], recs):            # first = 0: the light stays
        assert rc == rt.RT_ERR_INVALID and "first = 0" in msg and "edit 1" in msg
    for rc, msg in both([(0, 0, 0)], None):                       # ... also for an empty edit
        assert rc == rt.RT_ERR_INVALID and "first = 0" in msg
    for rc, msg in both([(5, 1, 0), (9, 0, 1)], None):            # null records
        assert rc == rt.RT_ERR_INVALID and "null records" in msg
    for rc, msg in both([(0xffffffff, 2, 0)], None):              # a range outside any scene: no device call either
        assert rc == rt.RT_ERR_INVALID
    for rc, msg in both([(9, 1, 0), (5, 5, 1)], recs):            # overlapping ranges, in any order
        assert rc == rt.RT_ERR_INVALID and "overlaps" in msg
    for rc, msg in both([(5, 1, 0), (7, 0, 1), (5, 0, 1)], recs):  # the same first twice
        assert rc == rt.RT_ERR_INVALID and "same first" in msg
    for rc, msg in both([(5, 2, 0), (7, 2, 1)], recs):            # adjacent ranges are fine: the null scene is what is refused
        assert rc == rt.RT_ERR_INVALID and "null scene" in msg
    for rc in (L.rt_scene_splice_ranges(None, None, 3, recs, None), L.rt_scene_splice_ranges_host(None, None, 3, recs)):
        assert rc == rt.RT_ERR_INVALID and "null edits" in L.rt_last_error().decode()

    keep = (C.c_uint8 * 4)(1, 1, 1, 1)
    for rc in (L.rt_scene_compact_triangles(None, keep, None), L.rt_scene_compact_triangles_host(None, keep)):
        assert rc == rt.RT_ERR_INVALID and "null scene" in L.rt_last_error().decode()
    assert L.rt_abi_version() == 4
