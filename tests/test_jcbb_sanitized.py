"""The shared JCBB code (csrc/host/jcbb.hpp) on the host under AddressSanitizer and UBSan: tests/jcbb_check.cpp is
a stand-alone program that runs the row extension against joint_ldl_prefix for every prefix of random SPD
matrices up to 32, the comparator and the prunings, the search's stack at depth 32, the budget, the search with
and without the bound against an exhaustive recursion, and the argument rules. The sanitizer runtimes are linked
statically, so the program needs nothing preloaded and does not mind what is."""
import os
import re
import subprocess

from conftest import ROOT


def test_jcbb_code_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "jcbb_check.cpp")
    exe = str(tmp_path / "jcbb_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    m = re.search(r"(\d+) cases, 0 failures", run.stdout)
    assert m and int(m.group(1)) >= 300, run.stdout
