"""The shared matching code (csrc/host/match.hpp) on the host under AddressSanitizer and UBSan:
tests/match_check.cpp is a stand-alone program that runs the two score functions against a plain solve and
their recipe, pivots that are not positive and NaN inputs, the information matrix's validation and inverse,
and the argument rules. The sanitizer runtimes are linked statically, so the program needs nothing preloaded
and does not mind what is."""
import os
import subprocess

from conftest import ROOT


def test_matching_code_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "match_check.cpp")
    exe = str(tmp_path / "match_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert "514 cases, 0 failures" in run.stdout
