"""The device-memory owner (csrc/hip/device_mem.hpp) on a malloc backend, under AddressSanitizer and
UBSan: tests/device_mem_check.cpp is a stand-alone program that runs every operation the library's call
sites use and then fails each backend call in turn. The sanitizer runtimes are linked statically, so the
program needs nothing preloaded and does not mind what is."""
import os
import subprocess

from conftest import ROOT


def test_device_mem_bookkeeping_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "device_mem_check.cpp")
    exe = str(tmp_path / "device_mem_check")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0 and build.stderr == "", build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert "every one failed in turn" in run.stdout
