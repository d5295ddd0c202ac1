"""tests/ring_selftest.cpp, built and run here as tests/test_selftests.py runs its programs: a stand-alone program with its own main, built from
csrc/ring_arith.hpp and csrc/inner_reduce.hpp (the text the ring kernels compile) and tests/selftest.hpp alone under AddressSanitizer and
UndefinedBehaviorSanitizer.  It must exit 0, print "ring_arith: N checks" with N > 500,000 and "ok: 0 failures", and leave no sanitizer report on
stderr.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_ring_selftest_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "ring_selftest")
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, "ring_selftest.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"ring_arith: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 500000, m and m.group(1)
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
