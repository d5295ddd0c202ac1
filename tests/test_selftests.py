"""The stand-alone CPU programs tests/*_selftest.cpp that run under the sanitizers, built and run here, one parametrised test for all of them
(operands_selftest, which asks 29 million questions and runs without them, keeps tests/test_operands.py).  Each program compares host-compilable product
code with brute force (mostly in unsigned __int128) and shares only tests/selftest.hpp -- CHECK, the counters, splitmix64, mulmod and the report lines --
with the others; its own header comment says what it covers.  A program is built from the sources its row lists and nothing else, under AddressSanitizer
and UndefinedBehaviorSanitizer, and must exit 0, print "ok: 0 failures", reach the counts of its row, and leave no sanitizer report on stderr.  Nothing
is loaded into python."""
import operator
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc")
HOST_MATH = os.path.join(CSRC, "host_math.cpp")

FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# program -> (what it checks, sources beside <program>.cpp, [(line printed, comparison, count)])
PROGRAMS = {
    "basis_selftest": ("agx::basis_constants (csrc/host_math.cpp), the constants of agx_ntt_basis_extend: 17-, 30-, 60- and 62-bit-class primes, S = 1, 2, 16, "
                       "targets that are sources, equal source moduli refused",
                       [HOST_MATH], [(r"basis_constants: (\d+) checks", operator.gt, 50000)]),
    "moddown_selftest": ("agx::moddown_constants (csrc/host_math.cpp), the constants agx_ntt_basis_mod_down adds to a basis: D^-1 mod q_j, the scaled n^-1 and "
                         "w1n with their quotients; a target that is a source modulus reported, not crashed on",
                         [HOST_MATH], [(r"moddown_constants: (\d+) checks", operator.gt, 50000)]),
    "fold_selftest": ("agx::fold_twiddle_pack (csrc/host_math.cpp), the table entry of the two-twiddle butterfly for moduli 2^60 - c (registry id 165), and a "
                      "plain-C++ restatement of that butterfly's six-link chain with every partial sum checked below 2^64",
                      [HOST_MATH], [(r"two-twiddle butterfly: (\d+) checks", operator.gt, 1000000)]),
    "inner_selftest": ("csrc/inner_reduce.hpp (the accumulate-and-reduce text the kernel itself compiles) and csrc/keyswitch_layout.hpp: 1, 2, 15 and 16 terms, "
                       "moduli from 2 to 62 bits; digit ranges, the scratch partition, counts past 2^60 words",
                       [], [(r"inner_reduce: (\d+) checks", operator.gt, 500000), (r"keyswitch_layout: (\d+) checks", operator.gt, 1000),
                                       # the range argument of csrc/inner_reduce.hpp: the estimate is low by at most 3
                                       (r"worst multiple of q before the subtracts: (\d+)", operator.le, 3)]),
    "hoist_selftest": ("csrc/keyswitch_layout.hpp for the two halves of the key switch, and a restatement of the permutation agx_ntt_inner_product_galois "
                       "reads through: a bijection, pi(2i + 1) = pi(2i) XOR 1, aligned blocks onto aligned blocks, sigma_g on the evaluation points",
                       [], [(r"hoisted_layout: (\d+) checks", operator.gt, 300),
                                       (r"galois_pi: (\d+) checks", operator.gt, 60000)]),      # every odd g at n = 2048 ... 32768 alone is 63488
}


@pytest.mark.parametrize("program", PROGRAMS)
def test_selftest_program(tmp_path, program):
    _, sources, counters = PROGRAMS[program]
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / program)
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, program + ".cpp"), *sources], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    for pattern, compare, count in counters:
        m = re.search(pattern, run.stdout)
        assert m and compare(int(m.group(1)), count), (pattern, compare.__name__, count, m and m.group(1))
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
