"""Registry id 165 with two kernels behind it (csrc/reg_s4096.hip): plans whose moduli q = 2^60 - c all have c <= 2^27 get the skip form of the
two-twiddle butterfly (reduction by the top four bits on the even stages only, 7q in place of 8q: csrc/modarith.hpp), every other plan of the class
c < 2^28 -- one larger c is enough -- the kernel with the sign-bit subtract on every stage.  The choice is the launch function's, from a flag of the plan;
here id 165 is named explicitly (as tests/test_gpu_fwd_q60c_fold.py does) on plans on both sides of the limit and on a mixed one, and once the plan
routes a launch past the companion threshold itself.  n = 4096 is the only size the kernel has.  Fully reduced outputs depend on (x, q, psi) alone, so
every result is compared word for word with the oracle's; the CPU model of the same schedule is tests/test_q60c_skip_model.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import oracle_tables, plan_for_moduli, rand_coeffs
from q60c_skip_cases import N, SKIP_MAX_C, prime_above_c, prime_at_or_below_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP_ID, EVERY_STAGE_TWIN_ID, MAIN_ID = 165, 168, 93
BIG = 4096 + 1      # frames per prime past the companion's 4,096-frame threshold, with an odd tail
KINDS = ("all 4q-1", "all q-1", "zeros", "random in [0,4q)")


@pytest.fixture(scope="module")
def skip_case(agx, orc):
    """the moduli, per modulus one frame of each input kind, and the oracle's transform of them, computed once"""
    q_in, c_in = prime_at_or_below_c(orc, SKIP_MAX_C)
    q_out, c_out = prime_above_c(orc, SKIP_MAX_C)
    bench = list(agx.find_primes(60, N, 4))
    assert c_in <= SKIP_MAX_C < c_out < (1 << 28) and [(1 << 60) - q for q in bench] == [16383, 98303, 163839, 245759]
    rng = np.random.default_rng(168)
    frames, want = {}, {}
    for q in [q_in, q_out] + bench:
        t = oracle_tables(orc, N, q)
        frames[q] = np.concatenate([np.full(N, 4 * q - 1, dtype=np.uint64), np.full(N, q - 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64),
                                    rand_coeffs(rng, N, q, hi_mult=4)])
        want[q] = orc.forward(frames[q], t[0], t[2], t[3], N)
        frames[q].setflags(write=False)
        want[q].setflags(write=False)
    plans = {"largest c at the limit": [q_in], "smallest c above the limit": [q_out], "benchmark primes": bench, "one c on each side": [q_in, q_out]}
    return {"plans": plans, "frames": frames, "want": want, "q_in": q_in}


def _take(per_q, moduli, first, batch):
    """[prime][batch][n] flat: frames first .. first + batch of every modulus"""
    return np.concatenate([per_q[q][first * N:(first + batch) * N] for q in moduli])


def _check(got, want, moduli, batch, lazy, where):
    for p, q in enumerate(moduli):
        sl = slice(p * batch * N, (p + 1) * batch * N)
        if lazy:
            assert (got[sl] < np.uint64(4 * q)).all(), (where, p, "a lazy output at or above 4q")
            assert np.array_equal(got[sl] % np.uint64(q), want[sl]), (where, p, "lazy outputs not congruent to the oracle's")
        else:
            assert np.array_equal(got[sl], want[sl]), (where, p, "reduced outputs differ from the oracle's")


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [True, False], ids=["in place", "out of place"])
@pytest.mark.parametrize("which", ["largest c at the limit", "smallest c above the limit", "benchmark primes", "one c on each side"])
def test_id_165_is_exact_on_both_sides_of_the_limit(agx, orc, dev, skip_case, which, in_place):
    """id 165 chosen explicitly; batch 3 (two windows over the four frames) and batch 1 (each frame on its own), reduced and lazy; every plan exact.
    Exactness does not tell which kernel ran (real data stay far from the words on which the skip form would wrap just above the limit): nor do the
    lazy words, since folding the top four bits gives the same word for v and v + q): the rule behind the choice -- every modulus of the plan within the
    limit, wherever the outsider stands -- is checked on the host code itself by tests/q60c_class_selftest.cpp"""
    moduli = skip_case["plans"][which]
    plan, _ = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    assert plan.forward_kernel(BIG) == SKIP_ID and plan.forward_kernel(1) == MAIN_ID
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + SKIP_ID)
    for first, batch in ((0, 3), (1, 3), (0, 1), (1, 1), (2, 1), (3, 1)):
        assert plan.forward_kernel(batch) == SKIP_ID
        x, want = _take(skip_case["frames"], moduli, first, batch), _take(skip_case["want"], moduli, first, batch)
        for lazy in (False, True):
            d_in = dev.to_device(x)
            d_out = d_in if in_place else dev.empty(d_in.numel())
            (plan.forward_lazy if lazy else plan.forward)(d_in.data_ptr(), d_out.data_ptr(), batch, dev.stream)
            _check(dev.to_host(d_out), want, moduli, batch, lazy, (which, first, batch, lazy))
            if not in_place:
                assert np.array_equal(dev.to_host(d_in), x), (which, first, batch, lazy, "an out-of-place call changed its input")
    plan.close()


@pytest.mark.gpu
def test_the_plan_s_own_route_past_the_companion_threshold(agx, orc, dev, skip_case):
    """4,096 + 1 frames per prime, the plan choosing its kernel: id 165, and within it the skip form (the largest c at the limit and the benchmark's
    smallest); every frame, reduced and lazy, compared on the device.  The big batch repeats the four frames of the fixture"""
    torch = dev.torch
    moduli = [skip_case["q_in"], skip_case["plans"]["benchmark primes"][0]]
    plan, _ = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    assert plan.forward_kernel(BIG) == SKIP_ID
    idx = torch.arange(BIG, device=dev.device) % 4
    tiled = lambda per_q: dev.to_device(np.concatenate([per_q[q] for q in moduli])).view(len(moduli), 4, N)[:, idx, :].contiguous().view(-1)      # noqa: E731
    d_x, d_want = tiled(skip_case["frames"]), tiled(skip_case["want"])
    d_y = dev.empty(d_x.numel())
    plan.forward(d_x.data_ptr(), d_y.data_ptr(), BIG, dev.stream)
    dev.sync()
    bad = (d_y != d_want).nonzero().flatten()[:4].tolist()
    assert not bad, ("reduced outputs differ from the oracle's at", bad)
    d_y.zero_()
    plan.forward_lazy(d_x.data_ptr(), d_y.data_ptr(), BIG, dev.stream)
    dev.sync()
    y = d_y.view(len(moduli), -1)
    for p, q in enumerate(moduli):
        # words are below 4q < 2^62, so int64 arithmetic is exact
        assert bool((y[p] >= 0).all()) and bool((y[p] < 4 * q).all()), (p, "a lazy output at or above 4q")
        assert torch.equal(y[p] % q, d_want.view(len(moduli), -1)[p]), (p, "lazy outputs not congruent to the oracle's")
    plan.close()


@pytest.mark.gpu
def test_every_stage_twin_and_id_165_write_identical_reduced_outputs(agx):
    """ids 168 (always the every-stage kernel) and 165 (the skip form on this plan) on the same 5 frames per prime, in one child bound to the diagnostics
    library: a process binds one library (tests/q60c_skip_diag_child.py)."""
    if not os.path.exists(agx.DIAG_LIB_PATH):
        agx.build_diag()
    env = dict(os.environ, AGX_NTT_LIB=agx.DIAG_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "q60c_skip_diag_child.py"), str(EVERY_STAGE_TWIN_ID), str(SKIP_ID)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SKIP AB OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
