"""The reference of the hoisted key switch alone, no device: hoisted_ref (tests/rns_ref.py) is keyswitch_ref with every NTT-form digit read
through pi_g.  With g = 1 it is keyswitch_ref word for word; with a noise-free rotation key it switches sigma_g(c) from sigma_g(s) to s within
the bound of test_it_switches_keys.  What the device tests compare against is therefore what a rotation needs."""
import numpy as np
import pytest

from gpu_util import moduli_for
from rns_cases import FIVE, FIVE_IDS, TWO_FULL_DIGITS, WIDE, WIDE_IDS, WIDE_PRIMES
from rns_ref import active_of, decompose_ref, digits_of, hoisted_ref, keyswitch_ref, rotation_bound, rotation_deviation, rotation_key_case

N, BATCH = 64, 2
ELEMENTS = (1, 5, 25, 2 * N - 1, 3, 77)


@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_g_1_is_the_one_call_reference(orc, shape):
    moduli = moduli_for(orc.find_prime, N, [60] * 6)
    active = active_of(moduli, shape)
    rng = np.random.default_rng(sum(shape))
    chat = np.stack([rng.integers(0, int(q), size=(BATCH, N), dtype=np.uint64) for q in active[:shape[0]]])
    key = np.stack([rng.integers(0, int(q), size=(len(digits_of(shape)), 2, N), dtype=np.uint64) for q in active], axis=2)
    assert np.array_equal(hoisted_ref(orc, N, moduli, shape, chat, key, BATCH, 1), keyswitch_ref(orc, N, moduli, shape, chat, key, BATCH))
    assert not np.array_equal(hoisted_ref(orc, N, moduli, shape, chat, key, BATCH, 5), keyswitch_ref(orc, N, moduli, shape, chat, key, BATCH))


@pytest.mark.parametrize("shape", WIDE, ids=WIDE_IDS)
def test_g_1_is_the_one_call_reference_at_wide_shapes(orc, shape):
    """the same on 33 primes: up to sixteen digits, sixteen sources a digit and sixteen special primes; and decompose_ref hands every digit's own
    residues through (a target that is a source gets x_j back)"""
    moduli = moduli_for(orc.find_prime, N, [60] * WIDE_PRIMES)
    active = active_of(moduli, shape)
    rng = np.random.default_rng(sum(shape))
    chat = np.stack([rng.integers(0, int(q), size=(BATCH, N), dtype=np.uint64) for q in active[:shape[0]]])
    key = np.stack([rng.integers(0, int(q), size=(len(digits_of(shape)), 2, N), dtype=np.uint64) for q in active], axis=2)
    one_call = keyswitch_ref(orc, N, moduli, shape, chat, key, BATCH)
    assert np.array_equal(hoisted_ref(orc, N, moduli, shape, chat, key, BATCH, 1), one_call)
    assert not np.array_equal(hoisted_ref(orc, N, moduli, shape, chat, key, BATCH, 5), one_call)
    ext = decompose_ref(orc, N, moduli, shape, chat)
    assert ext.shape == (len(digits_of(shape)), len(active), BATCH * N)
    for d, (first, count) in enumerate(digits_of(shape)):
        assert np.array_equal(ext[d, first:first + count], chat[first:first + count].reshape(count, -1)), ("digit", d)


def test_it_switches_rotated_keys_at_two_full_digits(orc):
    """the bound of test_it_switches_rotated_keys, p_count (1 + ||s||_1), on (12, 12, 6, 6) with g = 5: what test_gpu_keyswitch_wide.py asserts of the
    device is asserted of the reference here first"""
    shape, g = TWO_FULL_DIGITS, 5
    moduli = moduli_for(orc.find_prime, N, [60] * WIDE_PRIMES)
    chat, key, s, shat = rotation_key_case(orc, N, moduli, shape, g, BATCH, 1000 + sum(shape) + g)
    out = hoisted_ref(orc, N, moduli, shape, chat, key, BATCH, g)
    worst, bound = rotation_deviation(orc, N, moduli, shape, g, BATCH, chat, shat, out), rotation_bound(shape, s)
    print(f"shape {shape}, g = {g}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, g, worst, bound)


@pytest.mark.parametrize("g", ELEMENTS)
@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_it_switches_rotated_keys(orc, shape, g):
    """out_0 + out_1 s - sigma_g(c) sigma_g(s), CRT-centred modulo Q, is at most p_count (1 + ||s||_1) at every coefficient: pi_g(ext_d) is the NTT
    form of sigma_g(V_d), whose coefficients lie in (-S D_d, S D_d) and which is congruent to sigma_g(c) modulo D_d"""
    moduli = moduli_for(orc.find_prime, N, [60] * 6)
    chat, key, s, shat = rotation_key_case(orc, N, moduli, shape, g, BATCH, 1000 + sum(shape) + g)
    out = hoisted_ref(orc, N, moduli, shape, chat, key, BATCH, g)
    worst, bound = rotation_deviation(orc, N, moduli, shape, g, BATCH, chat, shat, out), rotation_bound(shape, s)
    print(f"shape {shape}, g = {g}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, g, worst, bound)
