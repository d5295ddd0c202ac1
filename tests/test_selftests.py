"""The stand-alone CPU programs tests/*_selftest.cpp that run under the sanitizers, built and run here, one parametrised test for all of them
(operands_selftest, which asks 29 million questions and runs without them, keeps tests/test_operands.py).  Each program compares host-compilable product
code with brute force (mostly in unsigned __int128) and shares only tests/selftest.hpp -- CHECK, the counters, splitmix64, mulmod and the report lines --
with the others; its own header comment says what it covers.  A program is built from the sources its row lists and nothing else, under AddressSanitizer
and UndefinedBehaviorSanitizer, and must exit 0, print "ok: 0 failures", reach the counts of its row, and leave no sanitizer report on stderr.  Nothing
is loaded into python.  A row may build the program's arguments; only the rows whose arguments are the oracle's class-edge moduli ask for the oracle."""
import operator
import os
import re
import shutil
import subprocess

import pytest

from modulus_cases import MIXES, edge_moduli

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "agilex-ntt_amd", "csrc")
HOST_MATH = os.path.join(CSRC, "host_math.cpp")
BASIS_GOLDEN = os.path.join(HERE, "golden", "basis_constants.txt")

FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
EDGES = ("below31", "above31", "below60", "above60", "below61", "above61", "below62", "c_max", "c_out", "min")


def edge_list(request):
    """The class edges of tests/modulus_cases.py at n = 4096 and n = 8: the primes next to 2^31, 2^60, 2^61 and 2^62, both sides of 2^60 - 2^28, and the six
    smallest admitted primes; with repeats, in that order."""
    orc = request.getfixturevalue("orc")
    moduli = []
    for n in (4096, 8):
        e = edge_moduli(orc, n)
        moduli += [e[name] for name in EDGES] + list(MIXES(orc, n)["tiny"])
    return moduli


def edges_in_order(request):
    moduli = list(dict.fromkeys(edge_list(request)))      # distinct, the order kept: wide and narrow moduli meet in one source set
    assert len(moduli) >= 20 and any(q > (1 << 62) - (1 << 20) for q in moduli) and min(moduli) == 17
    assert sum(q > 1 << 59 for q in moduli) >= 8
    return [str(q) for q in moduli], [f"moduli: {len(moduli)}"]


def edges_sorted(request):
    moduli = sorted(set(edge_list(request)))
    assert any(q > (1 << 62) - (1 << 20) for q in moduli) and min(moduli) == 17      # the top of the admitted range, and the smallest prime of n = 8
    return [str(q) for q in moduli], [f"moduli: {15 + len(moduli)}"]      # beside the program's built-in list of 15


def golden_words(path):
    with open(path) as f:
        return len(f.read().split())


# program -> (what it checks, sources beside <program>.cpp, [(line printed, comparison, count)], optional: request -> (arguments, lines that must be printed))
PROGRAMS = {
    "basis_selftest": ("agx::prepare_basis_image (csrc/host_math.cpp), the constants of agx_ntt_basis_extend: 17-, 30-, 60- and 62-bit-class primes, S = 1, 2, 16, "
                       "targets that are sources, equal source moduli refused; and every word of every image against tests/golden/basis_constants.txt, the "
                       "record the four builders that the image replaced left behind: as many checks as the file has words",
                       [HOST_MATH], [(r"basis_constants: (\d+) checks", operator.gt, 50000), (r"golden: (\d+) checks", operator.eq, golden_words(BASIS_GOLDEN))],
                       lambda request: ([BASIS_GOLDEN], [])),
    "moddown_selftest": ("agx::prepare_basis_image (csrc/host_math.cpp), the constants agx_ntt_basis_mod_down adds to a basis: D^-1 mod q_j, the scaled n^-1 and "
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
    "ring_selftest": ("csrc/ring_arith.hpp and csrc/inner_reduce.hpp, the text the ring kernels compile",
                      [], [(r"ring_arith: (\d+) checks", operator.gt, 500000)]),
    "weighted_selftest": ("csrc/weighted_arith.hpp, csrc/ring_arith.hpp and csrc/inner_reduce.hpp, the text the weighted kernels compile.  Its moduli are its "
                          "built-in list and the class edges, passed as arguments",
                          [], [(r"weighted_arith: (\d+) checks", operator.gt, 500000)], edges_sorted),
    "moddown_modes_selftest": ("csrc/moddown_arith.hpp (the two per-word steps of AGX_RESCALE_ROUND: the text the kernels compile) and csrc/host_math.cpp (the "
                               "constants of agx_ntt_basis_mod_down_mode and agx_ntt_basis_create_plain).  Its moduli are the class edges, passed as arguments; "
                               "it takes S = 1, 2 and 16 sources from every position of that list with t = 1, 2, 65537 and 2^64 - 59",
                               [HOST_MATH], [(r"moddown_arith: (\d+) checks", operator.gt, 10000), (r"moddown_mode_constants: (\d+) checks", operator.gt, 100000)],
                               edges_in_order),
    "bfv_conv_selftest": ("csrc/bfv_conv_arith.hpp (the per-word steps of agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont: the text the kernel "
                          "compiles) and csrc/host_math.cpp (the constants of agx_ntt_basis_create_aux).  Its moduli are the class edges, passed as arguments; "
                          "it takes S = 1, 2 and 16 sources from every position of that list, with the auxiliary prime from every position too",
                          [HOST_MATH], [(r"bfv_conv_arith: (\d+) checks", operator.gt, 10000), (r"bfv_conversions: (\d+) checks", operator.gt, 10000)],
                          edges_in_order),
    "q60c_class_selftest": ("csrc/q60c_class.hpp, the host-side questions about moduli 2^60 - c: q60c_of, and q60c_skip_class, the per-plan flag by which "
                            "registry id 165 chooses its skip-form kernel",
                            [], [(r"q60c_class: (\d+) checks", operator.gt, 100000)]),
}


@pytest.mark.parametrize("program", PROGRAMS)
def test_selftest_program(request, tmp_path, program):
    _, sources, counters, *arguments = PROGRAMS[program]
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    argv, lines = arguments[0](request) if arguments else ([], [])
    exe = str(tmp_path / program)
    subprocess.run([cxx, *FLAGS, "-o", exe, os.path.join(HERE, program + ".cpp"), *sources], check=True)
    run = subprocess.run([exe, *argv], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    for line in lines:
        assert line in run.stdout
    for pattern, compare, count in counters:
        m = re.search(pattern, run.stdout)
        assert m and compare(int(m.group(1)), count), (pattern, compare.__name__, count, m and m.group(1))
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
