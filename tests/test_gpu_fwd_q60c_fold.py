"""The two-twiddle butterfly of the forward kernel for moduli q = 2^60 - c, 0 < c < 2^28 (registry id 165, csrc/modarith.hpp:
ct_butterfly_q60c_fold): six multiply-adds, coefficients carried as arbitrary 64-bit words, a pass table whose slots hold {w, w 2^32 mod q} split at
bit 29 -- derived from w alone, whoever supplied the plan's tables.  tests/test_gpu_fwd_q60c.py and tests/test_gpu_variant_routes.py run this kernel
through id 165 as they stand; here: the top of the input range on the boundary values of c, in place and out of place; library-made against
caller-supplied tables; the kernel it replaced under its diagnostics id 167, and the two side by side.  Fully reduced outputs depend on (x, q, psi)
alone, so every result is compared word for word with the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import oracle_tables, plan_for_moduli, rand_coeffs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
FOLD_ID, OLD_TWIN_ID = 165, 167
BIG = 4096 + 1      # frames per prime past the companion's threshold (routing queries only: nothing of this size is launched here)


@pytest.fixture(scope="module")
def fold_case(agx, orc):
    """both boundary primes of tests/golden/q60c_boundary.json (the smallest and the largest c) and the second benchmark prime (the first IS the
    smallest-c boundary prime); per prime one frame of all 4q - 1, one of all zero, one random in [0,4q); the oracle's transform, computed once"""
    with open(os.path.join(ROOT, "tests", "golden", "q60c_boundary.json")) as f:
        moduli = [c["q"] for c in json.load(f)["cases"]] + [agx.find_primes(60, N, 2)[1]]
    assert len(set(moduli)) == 3 and all(0 < (1 << 60) - q < (1 << 28) for q in moduli)
    tabs = [oracle_tables(orc, N, q) for q in moduli]
    rng = np.random.default_rng(29)
    frames = [np.concatenate([np.full(N, 4 * q - 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64), rand_coeffs(rng, N, q, hi_mult=4)]) for q in moduli]
    want = [orc.forward(f, t[0], t[2], t[3], N) for f, t in zip(frames, tabs)]
    for a in frames + want:
        a.setflags(write=False)
    return {"moduli": moduli, "tabs": tabs, "frames": frames, "want": want}


def _take(per_prime, first, batch):
    """[prime][batch][n] flat: frames first .. first + batch of every prime"""
    return np.concatenate([a[first * N:(first + batch) * N] for a in per_prime])


def _check(got, want, tabs, batch, lazy, where):
    for p, t in enumerate(tabs):
        sl = slice(p * batch * N, (p + 1) * batch * N)
        if lazy:
            assert (got[sl] < np.uint64(4 * t[0])).all(), (where, p, "a lazy output at or above 4q")
            assert np.array_equal(got[sl] % np.uint64(t[0]), want[sl]), (where, p, "lazy outputs not congruent to the oracle's")
        else:
            assert np.array_equal(got[sl], want[sl]), (where, p, "reduced outputs differ from the oracle's")


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [True, False], ids=["in place", "out of place"])
def test_top_of_the_input_range_on_the_boundary_primes(agx, orc, dev, fold_case, in_place):
    """id 165 chosen explicitly; batch 3 (the three frames) and batch 1 (each frame on its own), reduced and lazy"""
    tabs = fold_case["tabs"]
    plan, _ = plan_for_moduli(agx, orc, N, fold_case["moduli"], inverse=False)
    assert plan.forward_kernel(BIG) == FOLD_ID
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + FOLD_ID)
    for first, batch in ((0, 3), (0, 1), (1, 1), (2, 1)):
        assert plan.forward_kernel(batch) == FOLD_ID
        x, want = _take(fold_case["frames"], first, batch), _take(fold_case["want"], first, batch)
        for lazy in (False, True):
            d_in = dev.to_device(x)
            d_out = d_in if in_place else dev.empty(d_in.numel())
            (plan.forward_lazy if lazy else plan.forward)(d_in.data_ptr(), d_out.data_ptr(), batch, dev.stream)
            _check(dev.to_host(d_out), want, tabs, batch, lazy, (first, batch, lazy))
            if not in_place:
                assert np.array_equal(dev.to_host(d_in), x), (first, batch, lazy, "an out-of-place call changed its input")
    plan.close()


@pytest.mark.gpu
def test_caller_supplied_tables_give_the_library_made_plan_s_outputs(agx, orc, dev, fold_case):
    """the slots of id 165's table are made from w alone: a plan created from the oracle's {w, w'} tables and one the library made for the same
    moduli and roots write the same words, lazy ones included"""
    tabs, moduli = fold_case["tabs"], fold_case["moduli"]
    x, want = _take(fold_case["frames"], 0, 3), _take(fold_case["want"], 0, 3)
    supplied, _ = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    made = agx.Plan(N, moduli, psi=[t[1] for t in tabs])
    out = []
    for plan in (supplied, made):
        assert plan.forward_kernel(BIG) == FOLD_ID
        plan.set_variant(agx.VARIANT_REGBLOCK_BASE + FOLD_ID)
        res = []
        for lazy in (False, True):
            d = dev.to_device(x)
            (plan.forward_lazy if lazy else plan.forward)(d.data_ptr(), d.data_ptr(), 3, dev.stream)
            res.append(dev.to_host(d))
            _check(res[-1], want, tabs, 3, lazy, lazy)
        out.append(res)
        plan.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_tables_that_break_the_precon_contract_never_reach_the_kernel(agx, orc, dev, fold_case):
    """one precomputed quotient off by one: the plan takes the exact kernels (which repeat the reference's operations on whatever tables they are
    given), its large launches do not go to id 165, and id 165 refuses the plan"""
    tabs, moduli = fold_case["tabs"], fold_case["moduli"]
    tw = np.stack([t[2] for t in tabs])
    pre = np.stack([t[3] for t in tabs])
    pre[1, 5] ^= np.uint64(1)
    plan = agx.Plan(N, moduli, tables=(tw, pre))
    assert plan.forward_kernel(BIG) not in (FOLD_ID, OLD_TWIN_ID, 159) and plan.forward_kernel(3) != FOLD_ID
    x = _take(fold_case["frames"], 0, 3)
    want = np.concatenate([orc.forward(np.ascontiguousarray(x[p * 3 * N:(p + 1) * 3 * N]), t[0], tw[p], pre[p], N) for p, t in enumerate(tabs)])
    d = dev.to_device(x)
    plan.forward(d.data_ptr(), d.data_ptr(), 3, dev.stream)
    assert np.array_equal(dev.to_host(d), want)
    with pytest.raises(agx.AgxError) as ei:
        plan.set_variant(agx.VARIANT_REGBLOCK_BASE + FOLD_ID)
    assert ei.value.status == 2
    plan.close()


def _diag_child(agx, script, *ids):
    if not os.path.exists(agx.DIAG_LIB_PATH):
        agx.build_diag()
    env = dict(os.environ, AGX_NTT_LIB=agx.DIAG_LIB_PATH)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", script)] + [str(i) for i in ids], capture_output=True, text=True, timeout=300, env=env)


@pytest.mark.gpu
def test_replaced_arithmetic_under_its_diag_id(agx):
    """the kernel id 165 was (quotient estimate from {w, w'}) lives on as A/B twin 167 in lib/libagxntt_diag.so; a process binds one library, so it is
    checked in a child bound to that one (tests/q60c_diag_child.py, as the 512-thread twin 166 is)"""
    r = _diag_child(agx, "q60c_diag_child.py", OLD_TWIN_ID)
    assert r.returncode == 0 and "Q60C TWIN OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_old_and_new_kernels_write_identical_reduced_outputs(agx):
    """ids 167 and 165 on the same 5 frames per prime, in one child bound to the diagnostics library (tests/q60c_fold_diag_child.py)"""
    r = _diag_child(agx, "q60c_fold_diag_child.py", OLD_TWIN_ID, FOLD_ID)
    assert r.returncode == 0 and "FOLD AB OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
