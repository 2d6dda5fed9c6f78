"""The shared joint-compatibility code (csrc/host/joint.hpp) on the host under AddressSanitizer and UBSan:
tests/joint_check.cpp is a stand-alone program that runs the S entry against a plain sum and through the
block references, the LDL^T / prefix recurrence for m = 0, 1 and 32 against a Cholesky solve, the prefix
property, pivots that are not positive, NaN inputs, the argument rules and the batch builder on a hand-made
assembly tree. The sanitizer runtimes are linked statically, so the program needs nothing preloaded and does
not mind what is."""
import os
import re
import subprocess

from conftest import ROOT


def test_joint_code_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "joint_check.cpp")
    exe = str(tmp_path / "joint_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    m = re.search(r"(\d+) cases, 0 failures", run.stdout)
    assert m and int(m.group(1)) >= 200, run.stdout
