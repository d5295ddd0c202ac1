"""tests/quotient_ref.py, the Python-integer model of agx_ntt_basis_quotient, judged on the CPU: it is steps 4 to 7 of a whole BFV multiplication
(bfv_conv_ref.multiply) fed the un-scaled tensor words; the folded form the device route takes -- scaled inverses, z_j = s_j - sum_i y_i (q_i^-1 B_j^-1),
f_m by the row q_i^-1 mod m, alpha from W mod m -- gives the model's words exactly, at tiny and wide moduli, for small, huge and even t; lazy inputs change
nothing; and the constructed auxiliary rows reach the alphas they are built for, all seventeen at m = 17 and both centring edges at a wide m."""
import numpy as np
import pytest

import bfv_conv_ref as ref
import quotient_ref as qref
from modulus_cases import prime_below


def folded(x, Q, B, m, t):
    """the device route in Python integers: what the scaled inverses hand the kernel, then the kernel's sums, every word reduced as the kernel keeps it"""
    Q, B = tuple(Q), tuple(B)
    L, K = len(Q), len(B)
    D, Bp = ref.product(Q), ref.product(B)
    count = len(x[0])
    y = [[t * (v % q) * pow(D // q, -1, q) % q for v in row] for row, q in zip(x[:L], Q)]
    s = [[t * (v % b) * pow(D, -1, b) * pow(Bp // b, -1, b) % b for v in row] for row, b in zip(x[L:L + K], B)]
    sm = [t * (v % m) * pow(D, -1, m) % m for v in x[L + K]]
    out = [[0] * count for _ in Q]
    for e in range(count):
        z = [(s[j][e] - sum(y[i][e] * (pow(Q[i], -1, b) * pow(Bp // b, -1, b) % b) for i in range(L))) % b for j, b in enumerate(B)]
        fm = (sm[e] - sum(y[i][e] * pow(Q[i], -1, m) for i in range(L))) % m
        wm = sum(zj * (Bp // b % m) for zj, b in zip(z, B)) % m
        alpha = ref.centre((wm - fm) * pow(Bp, -1, m) % m, m)
        for i, q in enumerate(Q):
            out[i][e] = (sum(zj * (Bp // b % q) for zj, b in zip(z, B)) - alpha * (Bp % q)) % q
    return out


TINY = (17, 97, 113, 193, 241, 257, 337)


@pytest.mark.parametrize("t", [1, 2, 65537, 2**64 - 59])
@pytest.mark.parametrize("shape", [((97,), (113,), 17), ((97, 113), (193, 241, 257), 17), ((193, 241, 257, 337), (97,), 17), ((17, 97), (113, 193), 241)], ids=str)
def test_the_folded_route_is_the_model_at_tiny_moduli(shape, t):
    Q, B, m = shape
    rng = np.random.default_rng(len(Q) + 7 * len(B) + t % 1000)
    count = 120
    x = [[int(v) for v in rng.integers(0, 4 * q, size=count, dtype=np.uint64)] for q in Q + B + (m,)]
    want = qref.quotient(x, Q, B, m, t)
    assert folded(x, Q, B, m, t) == want
    assert qref.quotient([[v % q for v in row] for row, q in zip(x, Q + B + (m,))], Q, B, m, t) == want      # lazy words are their residues
    assert all(0 <= v < q for row, q in zip(want, Q) for v in row)


def test_the_folded_route_is_the_model_at_wide_moduli(orc):
    n = 64
    widths = (62, 61, 60, 45, 31, 30, 59, 54, 52)
    p = [prime_below(orc, 1 << b, n) for b in widths]
    rng = np.random.default_rng(5)
    for Q, B, m in ((p[:3], p[3:6], p[6]), (p[3:5], p[:3], p[8]), (p[5:9], p[:2], p[2]), (p[:1], p[1:2], p[5])):
        for t in (65537, 2**64 - 59, 1 << 40):
            x = [[int(v) for v in rng.integers(0, q, size=40, dtype=np.uint64)] for q in tuple(Q) + tuple(B) + (m,)]
            assert folded(x, Q, B, m, t) == qref.quotient(x, Q, B, m, t), (Q, B, m, t)


def test_the_constructed_auxiliary_rows_reach_their_alphas(orc):
    rng = np.random.default_rng(11)
    Q, B, m, t = (97, 113), (193, 241, 257), 17, 65537
    wanted = list(range(-8, 9))
    x = qref.rows_with_alphas(rng, Q, B, m, t, 48, wanted)
    got = qref.alphas(x, Q, B, m, t)
    assert got == [wanted[e % 17] for e in range(48)] and set(got) == set(range(-8, 9))
    n = 64
    wide = prime_below(orc, 1 << 61, n)
    Q, B = (prime_below(orc, 1 << 45, n), prime_below(orc, 1 << 60, n)), (prime_below(orc, 1 << 31, n), prime_below(orc, 1 << 62, n))
    half = (wide - 1) // 2
    wanted = [half, -half, 0, None, half - 1, -half + 1]
    x = qref.rows_with_alphas(rng, Q, B, wide, 2**64 - 59, 30, wanted)
    got = qref.alphas(x, Q, B, wide, 2**64 - 59)
    assert all(w is None or g == w for g, w in zip(got, wanted * 5)) and {half, -half} <= set(got)
    assert all(0 <= v < q for row, q in zip(x, Q + B + (wide,)) for v in row)


def test_a_bfv_multiplication_is_the_model_on_the_unscaled_tensor(orc):
    """the parameters of the end-to-end tests at n = 16: multiply()'s "out" is the model applied to its "tensor" divided back by t, component by
    component, and the result decrypts"""
    n = 16
    w = ref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    B = tuple(prime_below(orc, 1 << b, n) for b in w["B"])
    m_sk, m_tilde, t = prime_below(orc, 1 << w["m_sk"], n), prime_below(orc, 1 << w["m_tilde"], n), ref.BFV_T
    rng = ref.Rng(7)
    s = ref.keygen(rng, n)
    msgs = [[rng.below(t) for _ in range(n)] for _ in range(2)]
    cts = [ref.encrypt(rng, msg, s, Q, t) for msg in msgs]
    model = ref.multiply(cts[0], cts[1], Q, B, m_sk, m_tilde, t)
    every = Q + B + (m_sk,)
    for k in range(3):
        unscaled = [[v * pow(t, -1, q) % q for v in row] for row, q in zip(model["tensor"][k], every)]
        assert qref.quotient(unscaled, Q, B, m_sk, t) == model["out"][k], k
        assert qref.floor_on_bsk(unscaled, Q, B, m_sk, t) == model["floor"][k], k
    assert ref.decrypt(model["out"], s, Q, t) == ref.negacyclic(msgs[0], msgs[1], t)
