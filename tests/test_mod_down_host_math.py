"""agx::moddown_constants (csrc/host_math.cpp) -- the constants agx_ntt_basis_mod_down adds to a basis, computed once on the host -- checked on the
CPU: the stand-alone program tests/moddown_selftest.cpp, built from that file and host_math.cpp alone with AddressSanitizer and
UndefinedBehaviorSanitizer, compares them with brute force in unsigned __int128 (D^-1 mod q_j, the scaled n^-1 and w1n with their quotients;
17-, 30-, 60- and 62-bit-class primes, S = 1, 2, 16; a target that is a source modulus reported, not crashed on).  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc")


def test_moddown_constants_against_brute_force(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "moddown_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "moddown_selftest.cpp"), os.path.join(CSRC, "host_math.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"moddown_constants: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 50000
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
