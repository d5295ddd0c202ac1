"""tests/weighted_selftest.cpp, built and run here as tests/test_ring_selftest.py runs its program: a stand-alone program with its own main, built from
csrc/weighted_arith.hpp, csrc/ring_arith.hpp and csrc/inner_reduce.hpp (the text the weighted kernels compile) and tests/selftest.hpp alone under
AddressSanitizer and UndefinedBehaviorSanitizer.  Its moduli are its built-in list and the class edges of tests/modulus_cases.py at n = 4096 and n = 8, passed
as arguments: the primes next to 2^31, 2^60 and 2^62, both sides of 2^60 - 2^28, and the six smallest admitted primes.  It must exit 0, print
"weighted_arith: N checks" with N > 500,000 and "ok: 0 failures", and leave no sanitizer report on stderr.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

from modulus_cases import MIXES, edge_moduli

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
EDGES = ("below31", "above31", "below60", "above60", "below61", "above61", "below62", "c_max", "c_out", "min")


def test_weighted_selftest_program(orc, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    moduli = []
    for n in (4096, 8):
        e = edge_moduli(orc, n)
        moduli += [e[name] for name in EDGES] + list(MIXES(orc, n)["tiny"])
    moduli = sorted(set(moduli))
    assert any(q > (1 << 62) - (1 << 20) for q in moduli) and min(moduli) == 17      # the top of the admitted range, and the smallest prime of n = 8
    exe = str(tmp_path / "weighted_selftest")
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, "weighted_selftest.cpp")], check=True)
    run = subprocess.run([exe, *[str(q) for q in moduli]], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"moduli: {15 + len(moduli)}" in run.stdout
    m = re.search(r"weighted_arith: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 500000, m and m.group(1)
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
