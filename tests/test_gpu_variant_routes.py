"""Which kernel serves which call of a plan, through every change of agx_ntt_plan_set_variant: AUTO, an explicit registry id, the radix-2
kernels, REGBLOCK, and back to AUTO (which must bring the large-launch forward companion back).  In every state forward, forward_lazy,
inverse, polymul and polymul_ntt are compared word for word with the CPU oracle, whose results are computed once per module.

Expected ids at n = 4096: main 93, general forward companion 159, its twin 165 for moduli 2^60 - c, threshold
4,096 frames (batch x primes)."""
import numpy as np
import pytest

from gpu_util import oracle_polymul, oracle_tables, plan_for_moduli, radix2_twin, rand_coeffs

pytestmark = pytest.mark.gpu

BATCH = 3
MAIN_ID, TWIN_ID = 93, 165
ERR_BAD_SIZE, ERR_NO_INVERSE = 2, 9


def _case(orc, n, moduli, seed):
    """operands a in [0,4q), b in [0,q) ([prime][BATCH][n] flat) under `moduli` with their minimal roots, and the oracle's results"""
    rng = np.random.default_rng(seed)
    c = {"n": n, "moduli": [int(q) for q in moduli], "psi": [], "a": [], "b": [], "fwd": [], "inv": [], "mul": [], "mul0": []}
    for q in c["moduli"]:
        _, psi, tw, pre = oracle_tables(orc, n, q)
        itw, _ = orc.make_inv_tables(q, psi, n)
        a, b = rand_coeffs(rng, BATCH * n, q, hi_mult=4), rand_coeffs(rng, BATCH * n, q)
        fwd = orc.forward(a, q, tw, pre, n)
        c["psi"].append(psi)
        c["a"].append(a)
        c["b"].append(b)
        c["fwd"].append(fwd)
        c["inv"].append(orc.inverse(fwd, q, itw, n))
        c["mul"].append(oracle_polymul(orc, a, b, q, psi, n))
        c["mul0"].append(oracle_polymul(orc, a, np.tile(b[:n], BATCH), q, psi, n))      # every frame of a times frame 0 of b
    for k in ("a", "b", "fwd", "inv", "mul", "mul0"):
        c[k] = np.concatenate(c[k])
        c[k].setflags(write=False)
    return c


@pytest.fixture(scope="module")
def cases(agx, orc):
    return {
        "q60c": _case(orc, 4096, agx.find_primes(60, 4096, 4), 1),
        "n16384": _case(orc, 16384, [orc.find_prime(60, 16384, 0)], 2),
        "n64": _case(orc, 64, [orc.find_prime(30, 64, 0)], 3),
        "n64q60": _case(orc, 64, [orc.find_prime(60, 64, 0)], 4),
        "q61": _case(orc, 4096, [orc.find_prime(61, 4096, 0)], 5),
    }


def _check_forward(dev, plan, c, where):
    d_a, d_y = dev.to_device(c["a"]), dev.empty(c["a"].size)
    plan.forward(d_a.data_ptr(), d_y.data_ptr(), BATCH, dev.stream)
    assert np.array_equal(dev.to_host(d_y), c["fwd"]), (where, "forward")
    d_y.zero_()
    plan.forward_lazy(d_a.data_ptr(), d_y.data_ptr(), BATCH, dev.stream)
    got, per = dev.to_host(d_y), BATCH * c["n"]
    for p, q in enumerate(c["moduli"]):
        sl = slice(p * per, (p + 1) * per)
        assert (got[sl] < np.uint64(4 * q)).all(), (where, p, "a lazy output at or above 4q")
        assert np.array_equal(got[sl] % np.uint64(q), c["fwd"][sl]), (where, p, "lazy outputs not congruent to the oracle's")


def _check_inverse(dev, plan, c, where):
    d_x, d_y = dev.to_device(c["fwd"]), dev.empty(c["fwd"].size)
    plan.inverse(d_x.data_ptr(), d_y.data_ptr(), BATCH, dev.stream)
    assert np.array_equal(dev.to_host(d_y), c["inv"]), (where, "inverse")


def _check_products(dev, plan, c, where):
    n, primes = c["n"], len(c["moduli"])
    d_a, d_b = dev.to_device(c["a"]), dev.to_device(c["b"])
    d_c, d_s = dev.empty(c["a"].size), dev.empty(c["a"].size)
    plan.polymul(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), BATCH, dev.stream)
    assert np.array_equal(dev.to_host(d_c), c["mul"]), (where, "polymul")
    d_bhat = dev.empty(c["b"].size)
    plan.forward(d_b.data_ptr(), d_bhat.data_ptr(), BATCH, dev.stream)
    d_c.zero_()
    plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), BATCH, BATCH, dev.stream)
    assert np.array_equal(dev.to_host(d_c), c["mul"]), (where, "polymul_ntt, one bhat frame per frame")
    d_b0 = dev.to_device(np.concatenate([c["b"][p * BATCH * n:p * BATCH * n + n] for p in range(primes)]))
    d_bhat0 = dev.empty(primes * n)
    plan.forward_lazy(d_b0.data_ptr(), d_bhat0.data_ptr(), 1, dev.stream)
    d_c.zero_()
    plan.polymul_ntt(d_a.data_ptr(), d_bhat0.data_ptr(), d_c.data_ptr(), BATCH, 1, dev.stream)
    assert np.array_equal(dev.to_host(d_c), c["mul0"]), (where, "polymul_ntt, one bhat frame per prime")


def _check_all(dev, plan, c, where):
    _check_forward(dev, plan, c, where)
    _check_inverse(dev, plan, c, where)
    _check_products(dev, plan, c, where)


def _ids(plan, batches):
    return [plan.forward_kernel(b) for b in batches]


def test_n4096_q60c_walk_through_every_variant(agx, dev, cases):
    """(a) the four benchmark primes (all 2^60 - c): 1024 frames per prime are exactly the companion's 4,096-frame threshold"""
    c = cases["q60c"]
    plan = agx.Plan(c["n"], c["moduli"], psi=c["psi"])      # the library's own tables from the same roots, inverse included
    base = agx.VARIANT_REGBLOCK_BASE
    walk = [("AUTO (fresh)", None, MAIN_ID, TWIN_ID), ("BASE+165", base + 165, 165, 165), ("AUTO", agx.VARIANT_AUTO, MAIN_ID, TWIN_ID),
            ("LDS_RADIX2", agx.VARIANT_LDS_RADIX2, -1, -1), ("REGBLOCK", agx.VARIANT_REGBLOCK, MAIN_ID, TWIN_ID),
            ("BASE+92", base + 92, 92, 92), ("AUTO (last)", agx.VARIANT_AUTO, MAIN_ID, TWIN_ID)]
    for step, (name, variant, small, large) in enumerate(walk):
        if variant is not None:
            plan.set_variant(variant)
        where = (step, name)
        assert _ids(plan, (3, 1024)) == [small, large], where
        _check_all(dev, plan, c, where)
    assert plan.forward_kernel(1023) == MAIN_ID
    big = 1024
    twin = radix2_twin(agx, plan)
    d_x = dev.empty(len(c["moduli"]) * big * c["n"])
    plan.fill_synthetic(d_x.data_ptr(), big, 0, 7, dev.stream)
    d_y, d_z = dev.empty(d_x.numel()), dev.empty(d_x.numel())
    plan.forward(d_x.data_ptr(), d_y.data_ptr(), big, dev.stream)
    twin.forward(d_x.data_ptr(), d_z.data_ptr(), big, dev.stream)
    dev.sync()
    assert dev.torch.equal(d_y, d_z), "the companion's forward at its threshold differs from the radix-2 kernels'"
    twin.close()
    plan.close()


def _there_and_back(agx, dev, c, explicit_id, batches, check):
    plan = agx.Plan(c["n"], c["moduli"], psi=c["psi"])      # the library's own tables from the same roots, inverse included
    fresh = _ids(plan, batches)
    check(dev, plan, c, "fresh")
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + explicit_id)
    assert _ids(plan, batches) == [explicit_id] * len(batches)
    check(dev, plan, c, f"BASE+{explicit_id}")
    plan.set_variant(agx.VARIANT_AUTO)
    assert _ids(plan, batches) == fresh
    check(dev, plan, c, "AUTO")
    plan.close()


def test_n16384_explicit_id_and_back(agx, dev, cases):
    """(b) one 60-bit prime at n = 16384: the ticket-loop inverse runs behind a pass table rebuilt by set_variant"""
    def check(dev, plan, c, where):
        _check_forward(dev, plan, c, where)
        _check_inverse(dev, plan, c, where)
        n = c["n"]
        d_a, d_b, d_c, d_s = dev.to_device(c["a"]), dev.to_device(c["b"]), dev.empty(BATCH * n), dev.empty(BATCH * n)
        plan.polymul(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), BATCH, dev.stream)
        assert np.array_equal(dev.to_host(d_c), c["mul"]), (where, "polymul")

    _there_and_back(agx, dev, cases["n16384"], 117, (1, 3, 10**6), check)


def test_n64_explicit_id_and_back(agx, dev, cases):
    """(c) one 30-bit prime at n = 64: from the 32-bit wave-packed default to the 64-bit kernel 203 and back"""
    _there_and_back(agx, dev, cases["n64"], 203, (1, 3, 10**6), _check_all)


def test_plan_without_inverse_tables(agx, orc, dev, cases):
    """(d) n = 64 from forward tables only: forward is right in every state; inverse and both products answer AGX_ERR_NO_INVERSE"""
    c = cases["n64q60"]
    plan, _ = plan_for_moduli(agx, orc, c["n"], c["moduli"], inverse=False)
    n = c["n"]
    d_a, d_b, d_c, d_s = dev.to_device(c["a"]), dev.to_device(c["b"]), dev.empty(BATCH * n), dev.empty(BATCH * n)
    for name, variant in (("AUTO", None), ("BASE+203", agx.VARIANT_REGBLOCK_BASE + 203), ("LDS_RADIX2", agx.VARIANT_LDS_RADIX2)):
        if variant is not None:
            plan.set_variant(variant)
        _check_forward(dev, plan, c, name)
        calls = {"inverse": lambda: plan.inverse(d_a.data_ptr(), d_c.data_ptr(), BATCH, dev.stream),
                 "polymul": lambda: plan.polymul(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), BATCH, dev.stream),
                 "polymul_ntt": lambda: plan.polymul_ntt(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), BATCH, BATCH, dev.stream)}
        for what, call in calls.items():
            with pytest.raises(agx.AgxError) as ei:
                call()
            assert ei.value.status == ERR_NO_INVERSE, (name, what)
    plan.close()


@pytest.mark.parametrize("case,refused", [("n64", 93), ("q61", 93)], ids=["wrong size", "16q-lazy under a 61-bit modulus"])
def test_refused_choice_changes_nothing(agx, dev, cases, case, refused):
    """(e) an id that is not legal for the plan is refused with AGX_ERR_BAD_SIZE on the host, and the plan goes on as before"""
    c = cases[case]
    plan = agx.Plan(c["n"], c["moduli"], psi=c["psi"])      # the library's own tables from the same roots, inverse included
    before = _ids(plan, (1, 3, 10**6))
    with pytest.raises(agx.AgxError) as ei:
        plan.set_variant(agx.VARIANT_REGBLOCK_BASE + refused)
    assert ei.value.status == ERR_BAD_SIZE
    assert _ids(plan, (1, 3, 10**6)) == before
    _check_forward(dev, plan, c, "after the refusal")
    _check_inverse(dev, plan, c, "after the refusal")
    plan.close()
