"""tests/moddown_modes_ref.py, the reference the GPU tests of agx_ntt_basis_mod_down_mode are judged against, pinned by properties in Python integers:
(X - delta) is divisible by D and the result is the quotient's residues; delta = 0 (mod t); t = 1 with FLOOR is rns_ref.mod_down; t = 1 with ROUND is
floor((X + h) / D) - u with 0 <= u < S; S = 1 is exactly floor((X + h) / q); X mod D on 0, 1, h - 1, h, h + 1, D - 1; and a BGV hybrid key switch in
integer polynomials at n = 8 with a noisy key, whose deviation is 0 modulo t on every coefficient.  No device, no library."""
import numpy as np
import pytest

from gpu_util import moduli_for
from moddown_modes_ref import FLOOR, ROUND, delta, half, keyswitch_coeff, lift_mode, mod_down_mode, negacyclic, plain_bound, sources_for_y, special_sources
from rns_ref import active_of, digits_of, mod_down, product, residues, ternary

MODES = (FLOOR, ROUND)
TS = (1, 2, 3, 65537, 65536, (1 << 64) - 59)


def _moduli(orc, spec, n=8):
    return moduli_for(orc.find_prime, n, spec)


def _values(rng, src, dst, count):
    """X in [0, D Q'): the edge values of X mod D under random quotients, then random values; returns (X, a [T][count], p [S][count])"""
    D, Qd = product(src), product(dst)
    H = D // 2
    rems = [0, 1, H - 1, H, H + 1, D - 1]
    rems = [r % D for r in rems] + [int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % D for _ in range(count - len(rems))]
    X = np.array([int(rng.integers(0, 1 << 62)) % Qd * D + r for r in rems], dtype=object)
    return X, residues(X, dst), residues(X, src)


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", TS)
def test_the_division_is_exact_and_keeps_the_value_modulo_t(orc, S, mode, t):
    moduli = _moduli(orc, [30, 60, 30, 61, 62][:S] + [60, 30, 62])
    src, dst = moduli[:S], moduli[S:]
    rng = np.random.default_rng(S * 10 + mode)
    X, a, p = _values(rng, src, dst, 40)
    D, h = product(src), half(src, mode)
    V, d = lift_mode(p, src, t, mode), delta(p, src, t, mode)
    assert all(0 <= v < S * D for v in V)
    assert all((int(x) - int(dd)) % D == 0 for x, dd in zip(X, d)), "X - delta is not divisible by D"
    assert all(int(dd) % t == 0 for dd in d), "delta is not 0 modulo t"
    assert all(int(dd) == t * (int(v) - h) for dd, v in zip(d, V))
    quotient = np.array([(int(x) - int(dd)) // D for x, dd in zip(X, d)], dtype=object)
    want = np.stack([np.array([int(y) % int(q) for y in quotient], dtype=np.uint64) for q in dst])
    assert np.array_equal(mod_down_mode(a, p, src, dst, t, mode), want)
    # the quotient times D is X modulo t: the value a BGV ciphertext carries is kept up to the factor D^-1
    assert all((int(y) * D - int(x)) % t == 0 for y, x in zip(quotient, X))


@pytest.mark.parametrize("S", [1, 2, 3])
def test_t_1_floor_is_the_existing_reference_and_round_is_the_rounded_quotient_less_u(orc, S):
    moduli = _moduli(orc, [60, 30, 61][:S] + [60, 62, 30])
    src, dst = moduli[:S], moduli[S:]
    rng = np.random.default_rng(S)
    X, a, p = _values(rng, src, dst, 60)
    D = product(src)
    assert np.array_equal(mod_down_mode(a, p, src, dst, 1, FLOOR), mod_down(a, p, src, dst))
    h = D // 2
    got = mod_down_mode(a, p, src, dst, 1, ROUND)
    V = lift_mode(p, src, 1, ROUND)
    for k, x in enumerate(X):
        u = int(V[k]) // D
        assert 0 <= u < S and int(V[k]) % D == (int(x) + h) % D
        want = (int(x) + h) // D - u
        assert [int(got[j, k]) for j in range(len(dst))] == [want % int(q) for q in dst], (k, u)
        if S == 1:
            assert u == 0


@pytest.mark.parametrize("bits", [30, 60, 62])
def test_one_source_is_the_rounded_division(orc, bits):
    moduli = _moduli(orc, [bits, 60, 61, 30])
    src, dst = moduli[:1], moduli[1:]
    q = int(src[0])
    h = q // 2
    rng = np.random.default_rng(bits)
    X, a, p = _values(rng, src, dst, 50)
    for mode, add in ((FLOOR, 0), (ROUND, h)):
        got = mod_down_mode(a, p, src, dst, 1, mode)
        for k, x in enumerate(X):
            assert [int(got[j, k]) for j in range(3)] == [(int(x) + add) // q % int(m) for m in dst], (mode, k)
    # the edges of the remainder: rounding turns at h + 1 (q = 2h + 1: r + h >= q iff r > h)
    edge = np.array([7 * q + r for r in (0, 1, h - 1, h, h + 1, q - 1)], dtype=object)
    got = mod_down_mode(residues(edge, dst), residues(edge, src), src, dst, 1, ROUND)
    assert [int(v) for v in got[0]] == [7, 7, 7, 7, 8, 8]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", [1, 65537])
def test_the_special_sources_are_what_they_say(orc, mode, t):
    src = _moduli(orc, [60, 30, 61])
    D = product(src)
    H = D // 2
    sp = special_sources(src, t, mode)
    assert sp.shape == (3, 7)
    X = [sum(int(sp[i, k]) * (D // int(q)) * pow(D // int(q), -1, int(q)) for i, q in enumerate(src)) % D for k in range(7)]
    assert X[:6] == [0, 1, H - 1, H, H + 1, D - 1]
    assert int(lift_mode(sp[:, 6:], src, t, mode)[0]) == sum((int(q) - 1) * (D // int(q)) for q in src), "not every y_i is q_i - 1"
    y = np.array([[5], [0], [int(src[2]) - 1]], dtype=object)
    assert int(lift_mode(sources_for_y(y, src, t, mode), src, t, mode)[0]) == sum(int(y[i, 0]) * (D // int(q)) for i, q in enumerate(src))


def _bgv_keys(rng, n, moduli, shape, t, s, s2, noisy):
    """key [digits][2][A][n] in coefficient form: key_{d,1} = a_d random, key_{d,0} = -a_d s + t e_d + P G_d s' modulo every active prime"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q = active[:q_count]
    Qp, P = product(Q), product(active[q_count:])
    key = []
    for first, count in digits_of(shape):
        Dd = product(Q[first:first + count])
        G = (Qp // Dd) * pow(Qp // Dd, -1, Dd)
        a = [int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % (Qp * P) for _ in range(n)]
        e = [int(v) * t for v in (rng.integers(-3, 4, size=n) if noisy else np.zeros(n, dtype=np.int64))]
        k0, k1 = [], []
        for q in active:
            k1.append(np.array([v % int(q) for v in a], dtype=object))
            k0.append(np.array([(int(e[i]) + P * G * int(s2[i]) - int(w)) % int(q) for i, w in enumerate(negacyclic(a, s, n, q))], dtype=object))
        key.append([k0, k1])
    return key


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("t", [2, 65537, 65536])
@pytest.mark.parametrize("noisy", [False, True], ids=["noise-free", "noisy"])
def test_a_bgv_key_switch_keeps_the_value_modulo_t(orc, mode, t, noisy):
    """three Q primes, two special primes, digits of two and one prime: out_0 + out_1 s - c s' is 0 modulo t on every coefficient and small; with a
    noise-free key in FLOOR mode it is within t p_count (1 + ||s||_1)"""
    n, shape = 8, (3, 3, 2, 2)
    moduli = _moduli(orc, [30] * 5, n)
    assert all(int(q) % t for q in moduli)
    rng = np.random.default_rng(1000 * mode + t % 97 + noisy)
    s, s2 = ternary(rng, n), ternary(rng, n)
    Q = moduli[:3]
    Qp = product(Q)
    c = np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in Q])
    cX = [sum(int(c[j, i]) * (Qp // int(q)) * pow(Qp // int(q), -1, int(q)) for j, q in enumerate(Q)) % Qp for i in range(n)]
    c = residues(cX, Q)
    key = _bgv_keys(rng, n, moduli, shape, t, s, s2, noisy)
    out = keyswitch_coeff(n, moduli, shape, c, key, t, mode)
    dev = []
    for j, q in enumerate(Q):
        dev.append((out[0, j].astype(object) + negacyclic(out[1, j], s, n, q) - negacyclic(negacyclic(c[j], s2, n, q), [1] + [0] * (n - 1), n, q)) % int(q))
    X = [sum(int(dev[j][i]) * (Qp // int(q)) * pow(Qp // int(q), -1, int(q)) for j, q in enumerate(Q)) % Qp for i in range(n)]
    X = [x - Qp if x > Qp // 2 else x for x in X]
    assert all(x % t == 0 for x in X), ("the deviation is not 0 modulo t", X)
    assert max(abs(x) for x in X) < Qp >> 20, "the deviation wraps modulo Q"
    if not noisy and mode == FLOOR:
        assert max(abs(x) for x in X) <= plain_bound(shape, s, t)
