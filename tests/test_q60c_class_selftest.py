"""tests/q60c_class_selftest.cpp, built and run here as tests/test_selftests.py runs its programs: a stand-alone program with its own main, built from
csrc/q60c_class.hpp (the host-side questions about moduli 2^60 - c: q60c_of, and q60c_skip_class, the per-plan flag by which registry id 165 chooses its
skip-form kernel) and tests/selftest.hpp alone under AddressSanitizer and UndefinedBehaviorSanitizer.  It must exit 0, print "q60c_class: N checks" with
N > 100,000 and "ok: 0 failures", and leave no sanitizer report on stderr.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_q60c_class_selftest_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "q60c_class_selftest")
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, "q60c_class_selftest.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"q60c_class: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 100000, m and m.group(1)
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
