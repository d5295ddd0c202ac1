"""The host-compilable parts of the hoisted key switch, checked on the CPU: the stand-alone program tests/hoist_selftest.cpp, built from that file
and csrc/keyswitch_layout.hpp alone with AddressSanitizer and UndefinedBehaviorSanitizer.  It checks the buffers of agx_ntt_keyswitch_decompose and
agx_ntt_keyswitch_apply_decomposed against the parts of the one-call scratch, the 2^60 limits, the two launch counts against the one call's, and a
restatement of the permutation agx_ntt_inner_product_galois reads through: a bijection, pi(2i + 1) = pi(2i) XOR 1, aligned blocks onto aligned
blocks (every odd g < 2n at every position for n = 2 ... 1024; for n = 2048 ... 32768 sampled: every g on 512 positions for the pair property, some
65 elements at every position for all three), and sigma_g on the evaluation points.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hoisted_layout_and_the_galois_permutation(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "hoist_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "hoist_selftest.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"hoisted_layout: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 300
    m = re.search(r"galois_pi: (\d+) checks", run.stdout)
    assert m and int(m.group(1)) > 60000      # every odd g at n = 2048 ... 32768 alone is 63488
    assert "ok: 0 failures" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
