"""tests/bfv_conv_selftest.cpp, built and run here as tests/test_moddown_modes_selftest.py runs its program: a stand-alone program with its own main, built
from csrc/bfv_conv_arith.hpp (the per-word steps of agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont: the text the kernel compiles),
csrc/host_math.cpp (the constants of agx_ntt_basis_create_aux) and tests/selftest.hpp alone under AddressSanitizer and UndefinedBehaviorSanitizer.  Its
moduli are the class edges of tests/modulus_cases.py at n = 4096 and n = 8, passed as arguments: the primes next to 2^31, 2^60, 2^61 and 2^62, both sides of
2^60 - 2^28, and the six smallest admitted primes; it takes S = 1, 2 and 16 sources from every position of that list, with the auxiliary prime from every
position too.  It must exit 0, print its two counts and "ok: 0 failures", and leave no sanitizer report on stderr.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

from modulus_cases import MIXES, edge_moduli

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_MATH = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc", "host_math.cpp")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
EDGES = ("below31", "above31", "below60", "above60", "below61", "above61", "below62", "c_max", "c_out", "min")


def test_bfv_conv_selftest_program(orc, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    moduli = []
    for n in (4096, 8):
        e = edge_moduli(orc, n)
        moduli += [e[name] for name in EDGES] + list(MIXES(orc, n)["tiny"])
    moduli = list(dict.fromkeys(moduli))      # distinct, the order kept: wide and narrow moduli meet in one source set
    assert len(moduli) >= 20 and any(q > (1 << 62) - (1 << 20) for q in moduli) and min(moduli) == 17
    assert sum(q > 1 << 59 for q in moduli) >= 8
    exe = str(tmp_path / "bfv_conv_selftest")
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, "bfv_conv_selftest.cpp"), HOST_MATH], check=True)
    run = subprocess.run([exe, *[str(q) for q in moduli]], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"moduli: {len(moduli)}" in run.stdout
    m = re.search(r"bfv_conv_arith: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 10000, m and m.group(1)
    m = re.search(r"bfv_conversions: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 10000, m and m.group(1)
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
