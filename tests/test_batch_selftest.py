"""tests/batch_selftest.cpp built and run here, as tests/test_ckks_selftest.py builds and runs its program: from the sources listed below and nothing else,
under AddressSanitizer and UndefinedBehaviorSanitizer; it must exit 0, print "ok: 0 failures", reach the counts below and leave no sanitizer report on stderr.
Nothing is loaded into python.  The program compares csrc/batch_arith.hpp and plain_from_digits of csrc/plain_arith.hpp (the text the kernels compile), the
index tables of agx::prepare_batch_image and the agx_ntt_plain_reduce constants of agx::prepare_plain_image (csrc/host_math.cpp) with brute force in unsigned
__int128.  Its moduli are the class edges of tests/modulus_cases.py and the smallest admitted primes, passed as arguments."""
import os
import re
import shutil
import subprocess

import pytest

from modulus_cases import MIXES, edge_moduli

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_MATH = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc", "host_math.cpp")
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
EDGES = ("below62", "above61", "below61", "above60", "below60", "c_max", "c_out", "above31", "below31", "min")


def test_batch_selftest(orc, tmp_path):
    moduli = []
    for n in (4096, 8):
        e = edge_moduli(orc, n)
        moduli += [e[name] for name in EDGES] + list(MIXES(orc, n)["tiny"])
    moduli = list(dict.fromkeys(moduli))      # distinct, the order kept: wide and narrow moduli meet in one set
    assert len(moduli) >= 20 and any(q > (1 << 62) - (1 << 20) for q in moduli) and min(moduli) == 17
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "batch_selftest")
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, "batch_selftest.cpp"), HOST_MATH], check=True)
    run = subprocess.run([exe, *[str(q) for q in moduli]], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"moduli: {len(moduli)}" in run.stdout
    for pattern, least in ((r"batch_reduce: (\d+) checks", 10000), (r"batch_source: (\d+) checks", 2999), (r"batch_tables: (\d+) checks", 20000),
                           (r"plain_digits: (\d+) checks", 50000)):
        m = re.search(pattern, run.stdout)
        assert m and int(m.group(1)) > least, (pattern, least, m and m.group(1))
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
