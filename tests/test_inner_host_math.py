"""The host-compilable parts of agx_ntt_inner_product and agx_ntt_keyswitch_*, checked on the CPU: the stand-alone program tests/inner_selftest.cpp,
built from that file, csrc/inner_reduce.hpp (the accumulate-and-reduce text the kernel itself compiles) and csrc/keyswitch_layout.hpp alone with
AddressSanitizer and UndefinedBehaviorSanitizer, compares them with unsigned __int128 arithmetic (1, 2, 15 and 16 terms, all operands q - 1,
random 128-bit sums, moduli from 2 to 62 bits; digit ranges, the scratch partition, counts past 2^60 words).  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_accumulate_reduce_and_layout_against_brute_force(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "inner_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "inner_selftest.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"inner_reduce: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 500000
    m = re.search(r"keyswitch_layout: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 1000
    m = re.search(r"worst multiple of q before the subtracts: (\d+)", run.stdout)
    assert m and int(m.group(1)) <= 3      # the range argument of csrc/inner_reduce.hpp: the estimate is low by at most 3
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
