"""The shared association code (csrc/host/associate.hpp) on the host under AddressSanitizer and UBSan:
tests/associate_check.cpp is a stand-alone program that runs the selection's register lists, merged the way
the kernels merge them, against a plain sort, the nis expression and the argument rules. The sanitizer
runtimes are linked statically, so the program needs nothing preloaded and does not mind what is."""
import os
import subprocess

from conftest import ROOT


def test_association_code_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "associate_check.cpp")
    exe = str(tmp_path / "associate_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert "160 selections, 0 failures" in run.stdout
