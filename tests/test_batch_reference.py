"""tests/batch_ref.py judged on the CPU, in Python integers: the batching model against the header's definition (z_j = m(psi^{e_j}), the pos formula in the
library's NTT order, encode as decode's inverse), the three properties the header states (slot-wise ring homomorphism, sigma_g with g = 5^r rotating both rows
left by r, g = 2n - 1 swapping them), and the reduce model against big integers: |X| at 0, 1, (D - 1) / 2 and random, odd, even and power-of-two t,
L = 1 ... 16, every factor; the device's digit form gives the same words."""
import random

import pytest

import batch_ref as ref

SMALL = ((2, 5), (4, 17), (16, 97), (64, 257))      # (n, t): the smallest admitted prime of each size


def _smallest_prime(n):
    t = 2 * n + 1
    while not ref.is_prime(t):
        t += 2 * n
    return t


def test_the_small_cases_are_the_smallest_admitted_primes():
    assert [(n, _smallest_prime(n)) for n, _ in SMALL] == list(SMALL)
    assert ref.min_root(5, 2) == 2 and ref.min_root(17, 4) == 2 and pow(ref.min_root(257, 64), 64, 257) == 256


@pytest.mark.parametrize("n,t", SMALL)
def test_exponents_and_positions(n, t):
    e = ref.exponents(n)
    assert sorted(e) == list(range(1, 2 * n, 2))      # every odd residue once: both tables are permutations
    assert all(e[n // 2 + j] == 2 * n - e[j] for j in range(n // 2)) and e[0] == 1
    pos = ref.slot_to_word(n)
    assert sorted(pos) == list(range(n))
    # the library's order: out[brev(k)] = x(psi^{2k+1}); slot j must be found at pos(j)
    rng = random.Random(n)
    m = [rng.randrange(t) for _ in range(n)]
    psi, bits = ref.min_root(t, n), n.bit_length() - 1
    out = [0] * n
    for k in range(n):
        out[ref.brev(k, bits)] = ref.evaluate(m, pow(psi, 2 * k + 1, t), t)
    z = ref.decode(m, n, t)
    assert [out[pos[j]] for j in range(n)] == z
    assert ref.decode_fast(m, n, t) == z


@pytest.mark.parametrize("n,t", SMALL + ((256, 7681), (1024, 12289)))
def test_encode_inverts_decode_and_takes_any_word(n, t):
    rng = random.Random(t)
    z = [rng.randrange(1 << 64) for _ in range(n)]
    z[0], z[-1] = (1 << 64) - 1, t
    m = ref.encode(z, n, t)
    assert all(0 <= c < t for c in m)
    assert ref.decode_fast(m, n, t) == [v % t for v in z]
    for j in random.Random(1).sample(range(n), min(n, 8)):
        assert ref.decode_slot(m, n, t, j) == z[j] % t
    back = [rng.randrange(t) for _ in range(n)]
    assert ref.encode(ref.decode_fast(back, n, t), n, t) == back


@pytest.mark.parametrize("n,t", SMALL)
def test_slotwise_ring_homomorphism(n, t):
    rng = random.Random(3 * n)
    a, b = ([rng.randrange(t) for _ in range(n)] for _ in range(2))
    za, zb = ref.decode(a, n, t), ref.decode(b, n, t)
    assert ref.decode([(u + v) % t for u, v in zip(a, b)], n, t) == [(u + v) % t for u, v in zip(za, zb)]
    assert ref.decode(ref.negacyclic(a, b, t), n, t) == [u * v % t for u, v in zip(za, zb)]
    assert ref.encode([u * v for u, v in zip(za, zb)], n, t) == ref.negacyclic(a, b, t)


@pytest.mark.parametrize("n,t", SMALL)
def test_rotation_and_row_swap(n, t):
    rng = random.Random(5 * n)
    m = [rng.randrange(t) for _ in range(n)]
    z = ref.decode(m, n, t)
    for r in range(max(n // 2, 1) + 1):
        g = pow(5, r, 2 * n)      # agx_ntt_galois_element(n, r)
        assert ref.decode(ref.automorphism(m, g, t), n, t) == ref.rotate_rows(z, r), r
    g_inv = pow(5, -1, 2 * n) if n > 1 else 1
    assert ref.decode(ref.automorphism(m, g_inv, t), n, t) == ref.rotate_rows(z, -1)
    assert ref.decode(ref.automorphism(m, 2 * n - 1, t), n, t) == ref.swap_rows(z)


def _primes_below(widths, step=128):
    """per width the largest prime = 1 (mod step) below 2^width that is not chosen yet"""
    chosen = []
    for bits in widths:
        c = ((1 << bits) - 2) // step * step + 1
        while c in chosen or not ref.is_prime(c):
            c -= step
        chosen.append(c)
    return chosen


PRIMES = _primes_below((60, 60, 50, 62, 17, 14, 9, 61, 40, 54, 43, 36, 31, 30, 25, 20))      # sixteen distinct odd primes, 9 to 62 bits, the widths mixed


def test_the_reduce_moduli_are_distinct_primes():
    assert len(set(PRIMES)) == 16 and all(ref.is_prime(q) for q in PRIMES)


@pytest.mark.parametrize("L", range(1, 17))
@pytest.mark.parametrize("t", [2, 3, 1 << 16, 257, 65537, 65536 * 3, (1 << 61) - 1, 1 << 61, (1 << 62) - 2])
def test_reduce_against_big_integers(L, t):
    Q = PRIMES[:L]
    D = ref.product(Q)
    H = (D - 1) // 2
    rng = random.Random(L * 1000003 + t)
    X = [0, 1, -1, H, -H, H - 1, 1 - H, 2, -2] + [rng.randrange(-H, H + 1) for _ in range(24)]
    x = [[v % q for v in X] for q in Q]
    assert [ref.centred_value([row[e] for row in x], Q) for e in range(len(X))] == X
    for factor in (1, 0, t - 1, (1 << 64) - 1, D % t):
        want = [factor % t * v % t for v in X]
        assert ref.reduce(x, Q, t, factor) == want
        assert ref.reduce_device_form(x, Q, t, factor) == want
    lazy = [[v + rng.randrange(4) * q for v in row] for row, q in zip(x, Q)]      # any words are reduced first
    assert ref.reduce(lazy, Q, t) == [v % t for v in X]


def test_reduce_decrypts_a_bgv_phase_and_undoes_a_dropped_modulus():
    Q, t = PRIMES[:3], 65537
    D = ref.product(Q)
    rng = random.Random(9)
    m = [rng.randrange(t) for _ in range(16)]
    X = [v + t * rng.randrange(-(1 << 40), 1 << 40) for v in m]      # m + t e
    assert ref.reduce([[v % q for v in X] for q in Q], Q, t) == m
    # a plaintext that carries D_dropped^-1 mod t, as a ModDown with t leaves it: factor = D_dropped mod t restores m, with no inverse formed here
    p = PRIMES[3]
    carried = [v * pow(p, -1, t) % t + t * rng.randrange(-5, 5) for v in m]
    assert ref.reduce([[v % q for v in carried] for q in Q], Q, t, p % t) == m
