"""agx::basis_constants (csrc/host_math.cpp) -- the constants of agx_ntt_basis_extend, computed once on the host -- checked on the CPU: the
stand-alone program tests/basis_selftest.cpp, built from that file and host_math.cpp alone with AddressSanitizer and
UndefinedBehaviorSanitizer, compares them with brute force in unsigned __int128 (17-, 30-, 60- and 62-bit-class primes, S = 1, 2, 16,
targets that are sources, equal source moduli refused).  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc")


def test_basis_constants_against_brute_force(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "basis_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "basis_selftest.cpp"), os.path.join(CSRC, "host_math.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"basis_constants: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 50000
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
