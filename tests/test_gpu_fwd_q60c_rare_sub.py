"""The last conditional subtract of registry id 165 (csrc/reg_s4096.hip), taken once per wave behind a scalar branch instead of once per coefficient
(csrc/rb_frame.hpp: kOptQ60cRareSub; the rule and its bound: csrc/modarith.hpp, q60c_tail_bounds; in Python integers: tests/test_q60c_rare_sub_model.py).
The subtract is due only for outputs below 16c, which random data never have, so every frame here is built to have some (tests/q60c_rare_cases.py): an
all-zero frame and constant polynomials put one in every lane of both waves; planted outputs put one into one wave of the workgroup only, or into
neither.  Every result is compared word for word with the oracle's, in place and out of place, reduced and lazy, on plans that take the skip-form
kernel and the every-stage kernel, which share the change; a child bound to the diagnostics library runs the same frames through the kernels id 165
launched before (twin 169) and with each half of the change alone (170, 171).  n = 4096 is the only size the kernels have."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import oracle_tables, plan_for_moduli
from q60c_rare_cases import N, constant_terms, forced_frames, planted_frames
from q60c_skip_cases import SKIP_MAX_C, prime_above_c, prime_at_or_below_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID, OLD_TWIN_ID, RARE_ONLY_ID, BASES_ONLY_ID = 165, 169, 170, 171
PLANS = ("benchmark primes", "largest c at the limit", "smallest c above the limit", "one c on each side")
SETS = ("zeros and constants", "planted outputs")


@pytest.fixture(scope="module")
def rare_case(agx, orc):
    """per modulus the two frame sets and the oracle's transform of them, computed once and read-only"""
    q_in, c_in = prime_at_or_below_c(orc, SKIP_MAX_C)
    q_out, c_out = prime_above_c(orc, SKIP_MAX_C)
    bench = list(agx.find_primes(60, N, 4))
    assert c_in <= SKIP_MAX_C < c_out < (1 << 28) and all(0 < (1 << 60) - q <= SKIP_MAX_C for q in bench)
    rng = np.random.default_rng(169)
    frames, want = {}, {}
    for q in [q_in, q_out] + bench:
        _, psi, tw, pre = oracle_tables(orc, N, q)
        forced = forced_frames(q)
        planted, outputs = planted_frames(orc, rng, q, psi)
        for name, x in zip(SETS, (forced, planted)):
            frames[name, q] = x
            want[name, q] = orc.forward(x, q, tw, pre, N)
        assert np.array_equal(want[SETS[1], q], outputs), "the oracle's forward does not return the planted outputs"
        w = want[SETS[0], q].reshape(-1, N)
        assert not w[0].any() and all((w[1 + i] == a).all() for i, a in enumerate(constant_terms(q)))
        for a in list(frames.values()) + list(want.values()):
            a.setflags(write=False)
    plans = {PLANS[0]: bench, PLANS[1]: [q_in], PLANS[2]: [q_out], PLANS[3]: [q_in, q_out]}
    return {"plans": plans, "frames": frames, "want": want}


@pytest.mark.gpu
@pytest.mark.parametrize("frame_set", SETS)
@pytest.mark.parametrize("which", PLANS)
def test_id_165_subtracts_where_it_is_due_and_only_there(agx, orc, dev, rare_case, which, frame_set):
    """6 or 3 frames per prime; each set in place and out of place, reduced (word for word the oracle's) and lazy (below 4q and congruent)"""
    moduli = rare_case["plans"][which]
    plan, _ = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + ID)
    x = np.concatenate([rare_case["frames"][frame_set, q] for q in moduli])
    want = np.concatenate([rare_case["want"][frame_set, q] for q in moduli])
    batch = x.size // (N * len(moduli))
    assert plan.forward_kernel(batch) == ID
    for in_place in (True, False):
        for lazy in (False, True):
            d_in = dev.to_device(x)
            d_out = d_in if in_place else dev.empty(d_in.numel())
            (plan.forward_lazy if lazy else plan.forward)(d_in.data_ptr(), d_out.data_ptr(), batch, dev.stream)
            got = dev.to_host(d_out)
            where = (which, frame_set, "in place" if in_place else "out of place", "lazy" if lazy else "reduced")
            if not in_place:
                assert np.array_equal(dev.to_host(d_in), x), (where, "an out-of-place call changed its input")
            for p, q in enumerate(moduli):
                sl = slice(p * batch * N, (p + 1) * batch * N)
                if lazy:
                    assert (got[sl] < np.uint64(4 * q)).all(), (where, p, "a lazy output at or above 4q")
                    assert np.array_equal(got[sl] % np.uint64(q), want[sl]), (where, p, "lazy outputs not congruent to the oracle's")
                else:
                    bad = np.flatnonzero(got[sl] != want[sl])[:4]
                    assert bad.size == 0, (where, p, "reduced outputs differ from the oracle's at", bad.tolist(), got[sl][bad].tolist(), want[sl][bad].tolist())
    plan.close()


@pytest.mark.gpu
def test_the_twins_write_identical_words(agx):
    """ids 169 (the kernels before the change), 170, 171 (each half alone) and 165 on the frames above, every plan, in one child bound to the
    diagnostics library: a process binds one library (tests/q60c_rare_diag_child.py)"""
    if not os.path.exists(agx.DIAG_LIB_PATH):
        agx.build_diag()
    env = dict(os.environ, AGX_NTT_LIB=agx.DIAG_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "q60c_rare_diag_child.py")] + [str(i) for i in (OLD_TWIN_ID, RARE_ONLY_ID, BASES_ONLY_ID, ID)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "RARE SUB AB OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
