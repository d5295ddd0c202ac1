"""agx::fold_twiddle_pack (csrc/host_math.cpp) -- the table entry of the two-twiddle butterfly for moduli 2^60 - c (registry id 165) -- and that
butterfly's arithmetic, checked on the CPU: the stand-alone program tests/fold_selftest.cpp, built from that file and host_math.cpp alone with
AddressSanitizer and UndefinedBehaviorSanitizer, compares the packing with brute force in unsigned __int128 (wC = w 2^32 mod q, halves below 2^29 and
2^31, exact recombination; the four benchmark primes and both boundary primes) and runs a plain-C++ restatement of the six-link chain with every partial
sum checked below 2^64 on the corners of the operand ranges, plus the class-wide bounds at c = 2^28 - 1.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc")


def test_fold_packing_and_butterfly_against_brute_force(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "fold_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "fold_selftest.cpp"), os.path.join(CSRC, "host_math.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"two-twiddle butterfly: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 1000000
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
