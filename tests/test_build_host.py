"""The GPU rebuild's text -- csrc/rt_build.h, every line a lane of the kernels of csrc/rt_build.hip
runs -- needs no GPU: tests/cpp/build_host.cpp runs it with one lane in the kernels' launch order,
built with AddressSanitizer and UBSan as a stand-alone host program.  It checks the partition's closed
form against the reference's sequential loop (every flag string up to length 16, 10,000 random ones),
whole builds against the host builder byte for byte (nodes, indices, depth, widest leaf) and against a
fresh pack_scene (packed nodes, slot records, slot boxes, slot map), and the refusal of a tree that
breaks a kernel limit."""
import os
import subprocess

from conftest import ROOT


def test_rebuild_text_on_the_host(tmp_path):
    exe = tmp_path / "build_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join(ROOT, "advancedgraphicsraytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", csrc, os.path.join(ROOT, "tests", "cpp", "build_host.cpp")]
                   + [os.path.join(csrc, f) for f in ("rt_scene_pack.cpp", "rt_host.cpp", "rt_sbvh.cpp")]
                   + ["-lz", "-pthread", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "advancedgraphicsraytracer_amd", "data")],
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "build_host ok" in r.stdout, r.stdout + r.stderr
