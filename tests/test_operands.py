"""csrc/operands.hpp -- the integer predicates behind the argument rules of the device-pointer calls -- checked on the CPU: the stand-alone
program tests/operands_selftest.cpp compares them with brute force over frame starts on a grid of small layouts, and asks them about the
largest shapes and extents the ABI admits, where 64-bit arithmetic would wrap."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_operand_predicates_against_brute_force_and_at_the_limits(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "operands_selftest")
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "operands_selftest.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"brute force: (\d+) cases", run.stdout)
    # n in {2, 8}, 1..3 primes, 1..4 polynomials, strides 0..5nB+3 and 0..5nP+3: 113,184 layouts asked of self_overlap, and the
    # 29,357,526 offsets (-extent-2 .. extent+2) of the 80,080 that do not overlap themselves asked of partial_overlap
    assert m and int(m.group(1)) == 29470710
    # down_buffers_ok against the rules agx_ntt_basis_mod_down and agx_ntt_rescale used to spell out: slabs of 0..3 words, 1..3 target slabs, four
    # bases (1..3 source slabs) resp. rescale's three on a grid of 14 words: 4 * 3 * (3 * 14**4 + 14**3) placements
    m = re.search(r"down_buffers_ok: (\d+) placements", run.stdout)
    assert m and int(m.group(1)) == 4 * 3 * (3 * 14**4 + 14**3) == 1415904
    # scratch_buffers_ok against the rule agx_ntt_basis_quotient, agx_ntt_plain_scale_down / _reduce, agx_ntt_ckks_decode and agx_ntt_batch_decode used to spell
    # out: x and the scratch of 0, 1, 2, 3, 4 or 6 words, out of 0..3, three bases on a grid of 14 words
    m = re.search(r"scratch_buffers_ok: (\d+) placements", run.stdout)
    assert m and int(m.group(1)) == 6 * 4 * 14**3 == 65856
    assert "ok: 0 failures" in run.stdout
