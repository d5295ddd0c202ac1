"""tests/sample_selftest.cpp built and run here, as tests/test_plain_selftest.py builds and runs its program: from the sources listed below and nothing else,
under AddressSanitizer and UndefinedBehaviorSanitizer; it must exit 0, print "ok: 0 failures", reach the counts below and leave no sanitizer report on stderr.
Nothing is loaded into python.  The program compares csrc/sample_arith.hpp (the ChaCha20 block and the per-cell / per-word steps of agx_ntt_sample_uniform /
_ternary / _cbd: the text the kernels compile) with the two standard vectors and a brute-force restatement; its moduli are the class edges of
tests/modulus_cases.py and the smallest admitted primes, passed as arguments."""
import os
import re
import shutil
import subprocess

import pytest

from modulus_cases import MIXES, edge_moduli

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
EDGES = ("below31", "above31", "below60", "above60", "below61", "above61", "below62", "c_max", "c_out", "min")


def test_sample_selftest(orc, tmp_path):
    moduli = []
    for n in (4096, 8, 2):
        e = edge_moduli(orc, n)
        moduli += [e[name] for name in EDGES] + list(MIXES(orc, n)["tiny"])
    moduli = list(dict.fromkeys(moduli))      # distinct, the order kept
    assert len(moduli) >= 20 and any(q > (1 << 62) - (1 << 20) for q in moduli) and min(moduli) == 5 and 17 in moduli
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "sample_selftest")
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, "sample_selftest.cpp")], check=True)
    run = subprocess.run([exe, *[str(q) for q in moduli]], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"moduli: {len(moduli)}" in run.stdout
    for pattern, least in ((r"vectors: (\d+) checks", 30), (r"uniform: (\d+) checks", 10000), (r"cap: (\d+) checks", 500), (r"ternary: (\d+) checks", 20000),
                           (r"cbd: (\d+) checks", 9000), (r"residue: (\d+) checks", 1000)):
        m = re.search(pattern, run.stdout)
        assert m and int(m.group(1)) > least, (pattern, least, m and m.group(1))
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
