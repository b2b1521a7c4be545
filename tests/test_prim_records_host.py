"""What rt_scene_update_prims runs per primitive on the device (PrimRecs and refit_level of
csrc/rt_update.h, over the record encoders of csrc/rt_records.h) needs no GPU:
tests/cpp/prim_records_host.cpp checks, writes and refits one primitive of each kind at a second pose
and compares every array, the packed nodes included, with a fresh pack_scene of that pose, built
with AddressSanitizer and UBSan as a stand-alone host program.  And the host refit over the animated room
equals its numpy restatement; the compat header's new methods compile, link and report the library's
error on a null handle."""
import ctypes as C
import os
import subprocess

import numpy as np

from anim_util import MOVERS, TIMES, room_prims, split_tree, with_prims
from conftest import ROOT
from refit_util import numpy_refit


def test_prim_records_equal_a_fresh_pack(tmp_path):
    exe = tmp_path / "prim_records_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join(ROOT, "advancedgraphicsraytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", csrc, os.path.join(ROOT, "tests", "cpp", "prim_records_host.cpp")]
                   + [os.path.join(csrc, f) for f in ("rt_scene_pack.cpp", "rt_host.cpp", "rt_sbvh.cpp")]
                   + ["-lz", "-pthread", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "prim_records_host ok" in r.stdout, r.stdout + r.stderr


def test_host_refit_of_the_room_equals_numpy(rt):
    """Scene.update_prims' semantics on the host: the movers' records replaced, the tree of t = 0 refitted."""
    base = room_prims(rt, 0.0)
    built = rt.build_bvh_host(base)[:2]
    for nodes, idx in (built, split_tree(rt, base)):     # the builder's tree; the planes in a leaf of their own
        assert rt.refit_bvh_host(base, nodes, idx).tobytes() == nodes.tobytes()
        seen = {nodes.tobytes()}
        for t in TIMES[1:]:
            pose = room_prims(rt, t)
            new = base
            for i in MOVERS:
                new = with_prims(new, i, [pose[i]])
            host = rt.refit_bvh_host(new, nodes, idx)
            assert host.tobytes() == numpy_refit(rt, new, nodes, idx).tobytes()
            seen.add(host.tobytes())
    assert len(seen) == len(TIMES)                       # in the split tree every pose moved a box


def test_pack_prims_layout(rt):
    prims = room_prims(rt, 0.7)
    rec, T = rt.pack_prims(prims)
    assert rec.shape == (len(prims), 11) and rec.dtype == np.int32 and T.shape == (len(prims), 16)
    assert list(rec[:, 0]) == [p.type for p in prims] and list(rec[:, 1]) == [p.material for p in prims]
    assert np.array_equal(rec[3, 2:].view(np.float32), np.array(list(prims[3].v), np.float32))
    assert np.array_equal(T[3], prims[3].T) and np.array_equal(T[1], np.eye(4, dtype=np.float32).reshape(16))


def test_null_scene_is_invalid(rt):
    L = rt.lib()
    one = (rt.Prim * 1)(rt.sphere((0, 0, 0), 1.0, 0))
    x = (rt.TriXform * 1)()
    assert L.rt_scene_update_prims_host(None, 0, 1, one, None) == rt.RT_ERR_INVALID
    assert b"rt_scene_update_prims_host" in L.rt_last_error()
    assert L.rt_scene_update_prims(None, 0, 1, None, None, None) == rt.RT_ERR_INVALID
    assert L.rt_scene_transform_triangles(None, x, 1, None, None) == rt.RT_ERR_INVALID
    assert b"rt_scene_transform_triangles" in L.rt_last_error()


COMPAT_HOST = r"""
#include <cstdio>
#include "rt_compat.hpp"
using namespace Tmpl8;
int main() {
    Scene scene((rt_scene *)nullptr);      // an adopted null handle: nothing to create, nothing to destroy
    rt_prim p{RT_SPHERE, 0, {0, 0, 0, 1}};
    const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    rt_tri_xform x{1, 1, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    int seen = 0;
    try { scene.UpdatePrimitives(0, &p, T, 1); } catch (const RtError &e) { seen += e.code == RT_ERR_INVALID; std::printf("%s\n", e.what()); }
    try { scene.UpdatePrimitivesDevice(0, nullptr, nullptr, 1); } catch (const RtError &e) { seen += e.code == RT_ERR_INVALID; }
    try { scene.TransformTriangles(&x, 1, nullptr); } catch (const RtError &e) { seen += e.code == RT_ERR_INVALID; std::printf("%s\n", e.what()); }
    std::printf("seen %d\n", seen);
    return seen == 3 ? 0 : 1;
}
"""


def test_compat_methods_compile_and_report_invalid(rt, tmp_path):
    src, exe = tmp_path / "anim_compat_host.cpp", tmp_path / "anim_compat_host"
    src.write_text(COMPAT_HOST)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    rt.LIB_PATH, "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{os.path.dirname(rt.LIB_PATH)}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "seen 3" in r.stdout, r.stdout + r.stderr
    assert "rt_scene_update_prims_host: null scene" in r.stdout and "rt_scene_transform_triangles: null scene" in r.stdout
