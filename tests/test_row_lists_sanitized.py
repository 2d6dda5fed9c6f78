"""The host side of the association and matching calls (csrc/host/row_lists.hpp) under AddressSanitizer and
UBSan: tests/row_lists_check.cpp is a stand-alone program that checks the grouping of rows by node against a
brute-force regrouping and the scatter of a chunk's lists against a direct triple loop, on exactly sized
buffers. The sanitizer runtimes are linked statically, so the program needs nothing preloaded and does not mind
what is."""
import os
import re
import subprocess

from conftest import ROOT


def test_row_lists_code_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "row_lists_check.cpp")
    exe = str(tmp_path / "row_lists_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    m = re.search(r"(\d+) cases, 0 failures", run.stdout)
    assert m and int(m.group(1)) >= 200, run.stdout
