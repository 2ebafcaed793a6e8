"""Builds tests/native/scan_reader_check.cpp with the host compiler against
sail_amd/ops/csrc/scan_reader.h and runs it: the host half of the pipelined
column-chunk reader (slicer, worker pool, ring, errors) needs no GPU. The
program compares every case with a plain sequential read and prints "ok"
last; the same source is what the address, undefined-behaviour and thread
sanitizer runs are built from."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found (set CXX)")


def test_scan_reader_check_program(tmp_path):
    exe = str(tmp_path / "scan_reader_check")
    build = subprocess.run(
        [_compiler(), "-std=c++17", "-O1", "-g", "-pthread", "-Wall",
         "-I", os.path.join(ROOT, "sail_amd", "ops", "csrc"),
         os.path.join(ROOT, "tests", "native", "scan_reader_check.cpp"),
         "-o", exe],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    lines = run.stdout.split()
    assert lines[-1] == "ok" and "FAIL" not in run.stdout
    # 2 and 3 slots x 1, 2 and 8 threads, and the run with small pieces
    assert run.stdout.count("passed") == 7
