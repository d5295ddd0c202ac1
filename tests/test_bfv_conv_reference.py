"""tests/bfv_conv_ref.py, the Python-integer model of agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont, judged on the CPU against the properties
include/agx_ntt.h states: the exact conversion returns X' wherever |u - k| <= (m - 1) / 2 and follows its formula outside, at both edges of the centring
(exhaustively over tiny moduli); the Montgomery form's W is an integer, congruent to X, X or X - D, inside its bounds; with r = V mod m the exact conversion
is the approximate one (rns_ref.convert); lazy inputs change nothing; and a whole BFV multiplication by the seven steps of INTEGRATION.md decrypts -- and does
not once the exact conversion is replaced by the approximate one."""
import itertools

import numpy as np
import pytest

import bfv_conv_ref as ref
import rns_ref
from modulus_cases import prime_below

TINY = (17, 97, 113)
TARGETS = (241, 257, 13)      # any odd moduli coprime to the sources and to m serve the model


def source_sets(m):
    pool = [q for q in TINY if q != m]
    return [c for k in range(1, len(pool) + 1) for c in itertools.combinations(pool, k)]


def all_values(src):
    """every X in [0, D) for D below 20000, every seventh and both ends above"""
    D = ref.product(src)
    return list(range(D)) if D < 20000 else sorted(set(range(0, D, 7)) | {D - 1, D - 2, D // 2, D // 2 + 1})


@pytest.mark.parametrize("m", [193, 17])
def test_t1_extend_exact_returns_every_value_in_range_and_follows_the_formula_at_the_edges(m):
    half = (m - 1) // 2
    deltas = range(-half - 1, half + 2) if m == 17 else (-half - 1, -half, -half + 1, -1, 0, 1, half - 1, half, half + 1)
    seen = set()
    for src in source_sets(m):
        D, S = ref.product(src), len(src)
        X = all_values(src)
        x = [[v % q for v in X] for q in src]
        V = ref.lift(x, src)
        u = [v // D for v in V]
        assert all(v % D == xx for v, xx in zip(V, X)) and 0 <= min(u) and max(u) < S
        for delta in deltas:      # k = u - delta: X' = X + k D, negative ones included
            Xp = [xx + (uu - delta) * D for xx, uu in zip(X, u)]
            r = [v % m for v in Xp]
            alphas = ref.alpha_exact(x, r, src, m)[1]
            seen |= set(alphas)
            got = ref.extend_exact(x, r, src, TARGETS, m)
            if abs(delta) <= half:
                assert set(alphas) == {delta}
                assert got == [[v % q for v in Xp] for q in TARGETS], (src, m, delta)
            else:      # one past either edge: alpha wraps to the other edge, and the output is the formula's
                want = -half if delta > 0 else half
                assert set(alphas) == {want}
                assert got == [[(v - want * D) % q for v in V] for q in TARGETS], (src, m, delta)
                assert got != [[v % q for v in Xp] for q in TARGETS]
    assert {-half, half} <= seen and (m != 17 or seen == set(range(-8, 9)))
    # the stated bound: |X'| < ((m - 1) / 2 - S) D is inside |u - k| <= (m - 1) / 2 for every u in [0, S)
    for S in (1, 2, 3):
        for k in range(-half + S, half - S + 1):
            assert all(abs(u - k) <= half for u in range(S))


@pytest.mark.parametrize("m", [193, 17])
def test_t2_extend_mont_leaves_x_or_x_minus_d_inside_its_bounds(m):
    both = set()
    for src in source_sets(m):
        D, S = ref.product(src), len(src)
        assert m > 2 * S
        X = all_values(src)
        x = [[v % q for v in X] for q in src]
        W = ref.mont_value(x, src, m)      # asserts that m divides V + alpha D
        for xx, w in zip(X, W):
            assert (w - xx) % D == 0 and w in (xx - D, xx), (src, m, xx, w)
            assert -D < 2 * w and m * (2 * w - D) < 2 * S * D, (src, m, xx, w)      # -D/2 < W < D/2 + S D / m
            both.add(w == xx)
        assert ref.extend_mont(x, src, TARGETS, m) == [[w % q for w in W] for q in TARGETS]
    assert both == {True, False}


def wide_case(orc, seed, S, count=64):
    rng = np.random.default_rng(seed)
    primes = [prime_below(orc, 1 << 60, 64, k) for k in range(S + 4)]
    src, dst, m = primes[:S], primes[S:S + 3], primes[S + 3]
    x = [[int(v) for v in rng.integers(0, q, size=count, dtype=np.uint64)] for q in src]
    return rng, src, dst, m, x


@pytest.mark.parametrize("S", [1, 2, 5, 16])
def test_t3_with_r_equal_to_v_mod_m_it_is_the_approximate_conversion(orc, S):
    _, src, dst, m, x = wide_case(orc, 31 + S, S)
    V = ref.lift(x, src)
    got = ref.extend_exact(x, [v % m for v in V], src, dst, m)
    want = rns_ref.convert(np.array(x, dtype=np.uint64), src, dst)
    assert np.array_equal(np.array(got, dtype=np.uint64), want)
    assert got == ref.extend_approx(x, src, dst)


@pytest.mark.parametrize("S", [1, 3, 16])
def test_t4_lazy_inputs_change_nothing(orc, S):
    rng, src, dst, m, x = wide_case(orc, 47 + S, S)
    r = [int(v) for v in rng.integers(0, m, size=len(x[0]), dtype=np.uint64)]
    for k in range(4):
        lazy = [[v + ((k + e + i) % 4) * q for e, v in enumerate(row)] for i, (row, q) in enumerate(zip(x, src))]
        lazy_r = [v + ((k + e) % 4) * m for e, v in enumerate(r)]
        assert ref.extend_exact(lazy, lazy_r, src, dst, m) == ref.extend_exact(x, r, src, dst, m)
        assert ref.extend_mont(lazy, src, dst, m) == ref.extend_mont(x, src, dst, m)


def bfv_case(orc, n, seed):
    w = ref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    B = tuple(prime_below(orc, 1 << b, n) for b in w["B"])
    m_sk, m_tilde, t = prime_below(orc, 1 << w["m_sk"], n), prime_below(orc, 1 << w["m_tilde"], n), ref.BFV_T
    assert len(set(Q + B + (m_sk, m_tilde))) == 7
    rng = ref.Rng(seed)
    s = ref.keygen(rng, n)
    msgs = [[rng.below(t) for _ in range(n)] for _ in range(2)]
    cts = [ref.encrypt(rng, msg, s, Q, t) for msg in msgs]
    return Q, B, m_sk, m_tilde, t, s, msgs, cts


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_t5_the_bfv_model_decrypts_and_fails_to_with_the_approximate_conversion(orc, seed):
    n = 16
    Q, B, m_sk, m_tilde, t, s, msgs, cts = bfv_case(orc, n, seed)
    for msg, ct in zip(msgs, cts):
        assert ref.decrypt(ct, s, Q, t) == msg
    want = ref.negacyclic(msgs[0], msgs[1], t)
    stages = ref.multiply(cts[0], cts[1], Q, B, m_sk, m_tilde, t)
    assert ref.decrypt(stages["out"], s, Q, t) == want      # every coefficient
    wrong = ref.multiply(cts[0], cts[1], Q, B, m_sk, m_tilde, t, exact=False)
    assert wrong["floor"] == stages["floor"] and wrong["out"] != stages["out"]
    assert ref.decrypt(wrong["out"], s, Q, t) != want
