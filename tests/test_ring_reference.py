"""The reference model of the ring calls alone, no device (tests/ring_cases.py): identities that tie add_galois_ref and tensor_ref to the definitions the
other references use, and the noise conditions of the two compositions the calls complete.  What the device tests compare against is therefore what a
homomorphic multiplication and a hoisted rotation need."""
import numpy as np
import pytest

from gpu_util import moduli_for, sigma
from ring_cases import (add_galois_ref, add_ref, hmult_case, hmult_deviation, hmult_ref, hrotate_case, hrotate_deviation, hrotate_ref, neg_ref, ring_operands,
                        sub_ref, tensor_ref)
from rns_ref import oracle_forward_set, oracle_inverse_set, rotation_bound

N, BATCH = 64, 2
SHAPES = [(4, 4, 2, 2), (3, 4, 2, 2), (4, 4, 2, 3), (2, 2, 1, 1)]


def _moduli(orc, n, spec=(60, 30, 61, 62)):
    return moduli_for(orc.find_prime, n, list(spec))


def test_linear_references_against_the_definition(orc):
    moduli = _moduli(orc, N)
    a, b, la, lb = ring_operands(N, moduli, BATCH, 3)
    for x, y in ((a[0], b[0]), (la[0], lb[0])):
        for p, q in enumerate(moduli):
            for f in range(BATCH):
                for i in (0, 1, 2, 3, N - 1):
                    u, v = int(x[p, f, i]) % q, int(y[p, f, i]) % q
                    assert int(add_ref(x, y, moduli)[p, f, i]) == (u + v) % q
                    assert int(sub_ref(x, y, moduli)[p, f, i]) == (u - v) % q
                    assert int(neg_ref(x, moduli)[p, f, i]) == (-u) % q
    assert np.array_equal(add_ref(a[0], b[0], moduli), add_ref(la[0], lb[0], moduli))      # lazy words are their residues
    assert np.array_equal(sub_ref(a[0], a[0], moduli), np.zeros_like(a[0]))
    assert np.array_equal(neg_ref(neg_ref(la[0], moduli), moduli), a[0])
    assert all(int(neg_ref(a[0], moduli)[p, 0, 0]) == 0 for p in range(len(moduli)))      # -0 = 0


@pytest.mark.parametrize("n", [8, 64])
def test_add_galois_with_g_1_is_add(orc, n):
    moduli = _moduli(orc, n)
    a, b, la, lb = ring_operands(n, moduli, BATCH, 4)
    assert np.array_equal(add_galois_ref(la[0], lb[0], moduli, 1), add_ref(a[0], b[0], moduli))
    assert not np.array_equal(add_galois_ref(la[0], lb[0], moduli, 5), add_ref(a[0], b[0], moduli))


def test_squaring_doubles_the_cross_term(orc):
    moduli = _moduli(orc, N)
    a, _, la, _ = ring_operands(N, moduli, BATCH, 5)
    c = tensor_ref(la, la, moduli)
    for p, q in enumerate(moduli):
        assert np.array_equal(c[1, p], (2 * a[0, p].astype(object) * a[1, p].astype(object) % q).astype(np.uint64))
        assert np.array_equal(c[0, p], (a[0, p].astype(object) ** 2 % q).astype(np.uint64))
    assert int(tensor_ref(a, ring_operands(N, moduli, BATCH, 5)[1], moduli)[0, 0, 0, 1]) == pow(moduli[0] - 1, 2, moduli[0])      # (q - 1)^2


@pytest.mark.parametrize("g", [3, 5, 2 * N - 1, pow(5, -1, 2 * N)])
def test_add_galois_of_zero_is_sigma_of_the_coefficients(orc, g):
    """INTT(add_galois_ref(0, NTT(x), g)) = sigma_g(x): the gather is the NTT form of X -> X^g"""
    moduli = moduli_for(orc.find_prime, N, [60, 30])
    rng = np.random.default_rng(g)
    x = np.stack([rng.integers(0, q, size=(BATCH, N), dtype=np.uint64) for q in moduli])
    xhat = oracle_forward_set(orc, N, moduli, x).reshape(len(moduli), BATCH, N)
    got = oracle_inverse_set(orc, N, moduli, add_galois_ref(np.zeros_like(xhat), xhat, moduli, g))
    for p, q in enumerate(moduli):
        assert np.array_equal(got[p], sigma(x[p], g, N, q))


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_hmult_meets_its_noise_condition(orc, shape, n):
    """(out_0 + d_0) + (out_1 + d_1) s - m m', CRT-centred modulo Q, is at most p_count (1 + ||s||_1): d_0 + d_1 s + d_2 s^2 = m m' exactly, everything
    before ModDown is exact modulo Q D_P for any target secret, and ModDown leaves less than that bound -- a condition, not a measurement"""
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    a, b, key, s, shat, mhat, mhat2 = hmult_case(orc, n, moduli, shape, BATCH, 2000 + sum(shape) + n)
    r = hmult_ref(orc, n, moduli, shape, a, b, key, BATCH)
    worst, bound = hmult_deviation(orc, n, moduli, shape, BATCH, r, shat, mhat, mhat2), rotation_bound(shape, s)
    print(f"shape {shape}, n = {n}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, n, worst, bound)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=[str(s) for s in SHAPES[:2]])
def test_hrotate_meets_its_noise_condition(orc, shape):
    """out_0 + sigma_g(c_0) + out_1 s - sigma_g(m) within the same bound: the key switch leaves sigma_g(c_1) sigma_g(s) up to it, add_galois is exact"""
    moduli = moduli_for(orc.find_prime, N, [60] * 6)
    c, key, s, shat, mhat = hrotate_case(orc, N, moduli, shape, 5, BATCH, 3000 + sum(shape))
    r = hrotate_ref(orc, N, moduli, shape, c, key, BATCH, 5)
    worst, bound = hrotate_deviation(orc, N, moduli, shape, 5, BATCH, r, shat, mhat), rotation_bound(shape, s)
    print(f"shape {shape}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, worst, bound)
