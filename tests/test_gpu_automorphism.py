"""agx_ntt_automorphism on the device: a(X) -> a(X^g) mod (X^n + 1), g odd, on coefficient-form and NTT-form frames.

The expected words come from the definition, written here as the SCATTER j -> g j mod 2n (coefficient j lands on position g j mod 2n when
that is below n, and negated on g j mod 2n - n otherwise; the kernels gather), and, for the NTT form, from the CPU oracle's transforms:
the GPU applied to orc.forward(a) must equal orc.forward(sigma_g(a)).  No tolerance anywhere: every comparison is word for word."""
import functools

import numpy as np
import pytest

from gpu_util import (Layout, arena_for, canary, capture, group_of_two, moduli_for, ntt_pi as _pi, oracle_forward_rns, oracle_tables, plan_for_moduli,
                      sigma as _sigma, status_of)

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
FORMS = (COEFF, NTT)


# ---- the reference: the definition as a scatter ---------------------------------------------------------------------------------
def _sigma_all(a, g, n, moduli, batch):
    """the same on a dense [prime][batch][n] set"""
    a = np.asarray(a).reshape(len(moduli), batch * n)
    return np.concatenate([_sigma(a[p], g, n, q) for p, q in enumerate(moduli)])


@functools.lru_cache(maxsize=None)
def _case(orc, n, moduli, batch, seed):
    """(coefficients a [P][batch][n] in [0,q), their transform); computed once per case and shared (read-only)"""
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.integers(0, q, size=batch * n, dtype=np.uint64) for q in moduli])
    ahat = oracle_forward_rns(orc, a, [oracle_tables(orc, n, q) for q in moduli], n)
    a.setflags(write=False)
    ahat.setflags(write=False)
    return a, ahat


def _galois(n):
    if n <= 8:
        return list(range(1, 2 * n, 2))
    return sorted({1, 3, 5, n - 1, n + 1, 2 * n - 1, pow(5, 7, 2 * n)})


def _run(dev, plan, words, batch, g, form, d_in=None):
    d_in = dev.to_device(words) if d_in is None else d_in
    d_out = dev.empty(d_in.numel())
    plan.automorphism(d_in.data_ptr(), d_out.data_ptr(), batch, g, form, dev.stream)
    return dev.to_host(d_out)


# ---- parity ---------------------------------------------------------------------------------------------------------------------
SIZES = [2, 4, 8, 64, 512, 1024, 4096, 16384, 32768]
SPECS = [(60,), (60, 30, 61)]
PARITY = [(n, spec, b) for n in SIZES for spec in SPECS for b in ((1, 5, 259) if n in (8, 64) else (1, 5))]


@pytest.mark.parametrize("n,spec,batch", PARITY)
def test_parity_both_forms(agx, orc, dev, n, spec, batch):
    """every size at which a kernel shape or its tiling changes, one 60-bit prime and three primes of mixed classes; batch 259 at n = 8
    and 64 puts several frames into one wave and leaves the last wave partly filled"""
    moduli = moduli_for(orc.find_prime, n, spec)
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    a, ahat = _case(orc, n, moduli, batch, 31 * n + len(spec) + batch)
    d_a, d_ahat = dev.to_device(a), dev.to_device(ahat)
    for g in _galois(n):
        want = _sigma_all(a, g, n, moduli, batch)
        assert np.array_equal(_run(dev, plan, None, batch, g, COEFF, d_in=d_a), want), ("coefficient form", n, spec, batch, g)
        assert np.array_equal(_run(dev, plan, None, batch, g, NTT, d_in=d_ahat), oracle_forward_rns(orc, want, tabs, n)), ("NTT form", n, spec, batch, g)
    plan.close()


@pytest.mark.parametrize("n", [4096, 32768])
def test_ntt_form_moves_words_unchanged(agx, orc, dev, n):
    """arbitrary 64-bit words (none of them a residue) come out as the numpy permutation of them: nothing is reduced, nothing is lost"""
    batch = 3
    moduli = moduli_for(orc.find_prime, n, (60, 30, 61))
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    words = canary(7, len(moduli) * batch * n)
    for g in (5, 2 * n - 1, n + 1):
        got = _run(dev, plan, words, batch, g, NTT).reshape(-1, n)
        assert np.array_equal(got, words.reshape(-1, n)[:, _pi(n, g)]), g
        assert np.array_equal(np.sort(got, axis=1), np.sort(words.reshape(-1, n), axis=1)), g
    plan.close()


@pytest.mark.parametrize("n", [64, 4096, 32768])
@pytest.mark.parametrize("bits", [60, 30])
def test_coefficient_form_takes_the_lazy_range(agx, orc, dev, n, bits):
    """inputs in [0,4q) with 0, q, 2q, 3q, q-1 and 4q-1 planted where the image keeps its sign and where it is negated; outputs in [0,q)"""
    batch = 2
    moduli = moduli_for(orc.find_prime, n, (bits,))
    q = moduli[0]
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    rng = np.random.default_rng(n + bits)
    planted = [0, q, 2 * q, 3 * q, q - 1, 4 * q - 1]
    for g in (5, 2 * n - 1):
        a = rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64).reshape(batch, n)
        e = (np.arange(n) * g) % (2 * n)
        keeps, negated = np.flatnonzero(e < n), np.flatnonzero(e >= n)
        assert len(negated) >= len(planted) and (len(keeps) >= len(planted) or g == 2 * n - 1)      # X -> X^-1 keeps the sign of a_0 alone
        keeps = keeps[:len(planted)]
        a[:, keeps] = np.array(planted[:len(keeps)], dtype=np.uint64)
        a[:, negated[:len(planted)]] = np.array(planted, dtype=np.uint64)
        got = _run(dev, plan, a.reshape(-1), batch, g, COEFF)
        assert int(got.max()) < q
        assert np.array_equal(got, _sigma(a, g, n, q)), (n, bits, g)
        assert np.all(got.reshape(batch, n)[:, (e[negated[:2]] - n)] == 0), "-0 and -q are 0"
    plan.close()


# ---- algebra on the device --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 512])
def test_algebra_on_the_device(agx, orc, dev, n):
    batch = 3
    moduli = moduli_for(orc.find_prime, n, (60, 30, 61))
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    a, ahat = _case(orc, n, moduli, batch, 5 * n + 1)
    total = a.size
    d = {COEFF: dev.to_device(a), NTT: dev.to_device(ahat)}
    t1, t2, t3 = dev.empty(total), dev.empty(total), dev.empty(total)
    A = lambda src, dst, g, form: plan.automorphism(src.data_ptr(), dst.data_ptr(), batch, g, form, dev.stream)  # noqa: E731
    for g, h in ((5, 3), (pow(5, 7, 2 * n), 2 * n - 1), (n + 1, n - 1)):
        for form in FORMS:
            A(d[form], t1, g, form)
            A(t1, t2, h, form)
            A(d[form], t3, (g * h) % (2 * n), form)
            assert np.array_equal(dev.to_host(t2), dev.to_host(t3)), ("sigma_h o sigma_g = sigma_gh", g, h, form)
            A(t1, t2, pow(g, -1, 2 * n), form)
            assert np.array_equal(dev.to_host(t2), dev.to_host(d[form])), ("sigma_g^-1 o sigma_g = id", g, form)
        A(d[NTT], t1, g, NTT)
        plan.inverse(t1.data_ptr(), t2.data_ptr(), batch, dev.stream)
        A(d[COEFF], t3, g, COEFF)
        assert np.array_equal(dev.to_host(t2), dev.to_host(t3)), ("inverse(automorphism_ntt(forward(a))) = automorphism_coeff(a)", g)
    plan.close()


# ---- guarded arenas, rejections ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 1024, 32768])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("out_odd", [True, False])
def test_guarded_arenas_at_odd_offsets(agx, orc, dev, n, form, out_odd):
    """d_in (and d_out, or d_in alone) 8-byte but not 16-byte aligned inside one arena: the canaries and the input frames are intact, the
    output frames are as expected"""
    batch = 3
    moduli = moduli_for(orc.find_prime, n, (60, 30, 61))
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    a, ahat = _case(orc, n, moduli, batch, 3 * n + 2)
    src = a if form == COEFF else ahat
    li = Layout(n, len(moduli), batch, offset=1)
    lo = Layout(n, len(moduli), batch, offset=li.span() + (6 if out_odd else 7))
    assert li.offset % 2 == 1 and lo.offset % 2 == (1 if out_odd else 0)
    for g in (5, 2 * n - 1):
        arena = arena_for(dev, n, (li, src), (lo, None))
        plan.automorphism(arena.address(li.offset), arena.address(lo.offset), batch, g, form, dev.stream)
        img = arena.image()
        assert not arena.faults([(li, src), (lo, None)], img), "a word outside the output changed"
        want = _sigma_all(a, g, n, moduli, batch)
        assert np.array_equal(arena.frames(lo, img), want if form == COEFF else oracle_forward_rns(orc, want, tabs, n)), (n, form, g)
    plan.close()


@pytest.mark.parametrize("n", [64, 4096])
def test_rejections_write_nothing(agx, orc, dev, n):
    primes, batch = 3, 2
    moduli = moduli_for(orc.find_prime, n, (60,) * primes)
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    a, _ = _case(orc, n, moduli, batch, 7 * n)
    total = primes * batch * n
    li = Layout(n, primes, batch, offset=0)
    lo = Layout(n, primes, batch, offset=li.span() + 2 * n)
    arena = arena_for(dev, n, (li, a), (lo, None))
    before = arena.image()
    x, out = arena.address(0), arena.address(lo.offset)
    A, st, w = plan.automorphism, dev.stream, 8
    for form in FORMS:
        for g in (0, 2, 2 * n, 2 * n + 1):
            assert status_of(agx, A, x, out, batch, g, form, st) == 5, g
        assert status_of(agx, A, x, x, batch, 5, form, st) == 5                                   # in place
        assert status_of(agx, A, x, x + w * (n // 2), batch, 5, form, st) == 5
        assert status_of(agx, A, x, x + w * (total - n // 2), batch, 5, form, st) == 5            # out starts inside in's last frame
        assert status_of(agx, A, x, x + w * (total - 1), batch, 5, form, st) == 5
        assert status_of(agx, A, out + w * (total - n // 2), out, batch, 5, form, st) == 5        # in starts inside out's last frame
        assert status_of(agx, A, out + w * (total - 1), out, batch, 5, form, st) == 5
        assert status_of(agx, A, x + 4, out, batch, 5, form, st) == 5 and status_of(agx, A, x, out + 4, batch, 5, form, st) == 5      # uint64_t data
        assert status_of(agx, A, 0, out, batch, 5, form, st) == 1 and status_of(agx, A, x, 0, batch, 5, form, st) == 1
        A(x, out, 0, 5, form, st)      # empty batch: nothing happens
    for form in (2, -1):
        assert status_of(agx, A, x, out, batch, 5, form, st) == 5
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    A(x, x + w * total, batch, 5, NTT, st)      # out right behind in: the ranges do not touch
    dev.sync()
    plan.close()


# ---- graph capture, groups, forward-only plans ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,form", [(4096, NTT), (1024, COEFF)])
def test_calls_are_graph_capturable(agx, orc, dev, n, form):
    """two calls captured one after the other on a side stream (no parallel branches), replayed twice on new data"""
    torch = dev.torch
    batch, gs = 5, (5, 2 * n - 1)
    moduli = moduli_for(orc.find_prime, n, (60, 30, 61))
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    cases = [_case(orc, n, moduli, batch, n + k) for k in (1, 2)]
    d_in = dev.to_device(cases[0][form])
    d_out = [dev.empty(d_in.numel()) for _ in gs]

    def both_elements(s):
        for g, d in zip(gs, d_out):
            plan.automorphism(d_in.data_ptr(), d.data_ptr(), batch, g, form, s)

    graph = capture(dev, lambda s: plan.automorphism(d_in.data_ptr(), d_out[0].data_ptr(), batch, gs[0], form, s), both_elements)
    for a, ahat in cases:
        d_in.copy_(torch.from_numpy((a, ahat)[form].view(np.int64).copy()))
        for d in d_out:
            d.zero_()
        graph.replay()
        dev.sync()
        for g, d in zip(gs, d_out):
            want = _sigma_all(a, g, n, moduli, batch)
            assert np.array_equal(dev.to_host(d), want if form == COEFF else oracle_forward_rns(orc, want, tabs, n)), ("replay", g)
    plan.close()


def test_group_equals_the_single_plan(agx, orc, dev):
    """DeviceGroup.automorphism on devices [0, 0] with unequal batches, against Plan.automorphism on the same words"""
    n = 4096
    moduli = moduli_for(orc.find_prime, n, (60, 30, 61))
    tabs = [oracle_tables(orc, n, q) for q in moduli]
    grp, plan, batches = group_of_two(agx, orc, n, moduli, 5)
    assert batches == [3, 2]
    cases = [_case(orc, n, moduli, bt, 900 + i) for i, bt in enumerate(batches)]
    for form in FORMS:
        d_in = [dev.to_device(c[form]) for c in cases]
        d_out = [dev.empty(d.numel()) for d in d_in]
        for g in (5, 2 * n - 1):
            single = [_run(dev, plan, None, bt, g, form, d_in=d_in[i]) for i, bt in enumerate(batches)]
            grp.automorphism([d.data_ptr() for d in d_in], [d.data_ptr() for d in d_out], batches, g, form)
            grp.synchronize()
            for i, bt in enumerate(batches):
                got = dev.to_host(d_out[i])
                want = _sigma_all(cases[i][0], g, n, moduli, bt)
                assert np.array_equal(got, single[i]), f"shard {i} differs from the single plan"
                assert np.array_equal(got, want if form == COEFF else oracle_forward_rns(orc, want, tabs, n)), f"shard {i} differs from the reference"
    grp.close()
    plan.close()


@pytest.mark.parametrize("n", [64, 4096])
def test_forward_only_plans_run_both_forms(agx, orc, dev, n):
    batch = 2
    moduli = moduli_for(orc.find_prime, n, (60, 30, 61))
    plan, tabs = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    a, ahat = _case(orc, n, moduli, batch, 11 * n)
    g = pow(5, 7, 2 * n)
    want = _sigma_all(a, g, n, moduli, batch)
    assert np.array_equal(_run(dev, plan, a, batch, g, COEFF), want)
    assert np.array_equal(_run(dev, plan, ahat, batch, g, NTT), oracle_forward_rns(orc, want, tabs, n))
    plan.close()
