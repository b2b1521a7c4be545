"""The timed choices' group schedule (csrc/rt_tune.h: camera walk, split order, frames in flight)
needs no GPU: tests/cpp/tune_host.cpp drives it with scripted stall flags and group times, built
with AddressSanitizer and UBSan as a stand-alone host program."""
import os
import subprocess

from conftest import ROOT


def test_group_schedule_and_decisions(tmp_path):
    exe = tmp_path / "tune_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "advancedgraphicsraytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tune_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "tune_host ok" in r.stdout, r.stdout + r.stderr
