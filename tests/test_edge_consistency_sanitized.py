"""The shared edge-consistency code (csrc/host/edge_check.hpp) on the host under AddressSanitizer and UBSan:
tests/edge_consistency_check.cpp is a stand-alone program that runs the bearing and odometry scores against a
long-double evaluation, the NaN rules, and the selection of the largest w2 through the association's register list
on negated scores against a plain descending sort. The sanitizer runtimes are linked statically, so the program
needs nothing preloaded and does not mind what is."""
import os
import subprocess

from conftest import ROOT


def test_edge_consistency_code_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "edge_consistency_check.cpp")
    exe = str(tmp_path / "edge_consistency_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert "3008 cases, 200 selections, 0 failures" in run.stdout
