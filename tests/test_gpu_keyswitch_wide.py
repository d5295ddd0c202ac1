"""The key switch at wide shapes on the device: agx_ntt_keyswitch_apply, _decompose, _apply_decomposed, _accumulate_decomposed and _mod_down on a plan of
33 primes, with up to sixteen digits, sixteen sources a digit, sixteen special primes and 32 active primes (rns_cases.WIDE) -- the sizes of real CKKS / BGV
parameter sets, where the [digits][A] walk through ext, the 16-term inner product, a short last digit beside special primes that lie apart and the
partition of the scratch are exercised beyond the six-prime shapes of test_gpu_keyswitch.py and test_gpu_keyswitch_hoisted.py.

The reference is rns_ref.keyswitch_ref, decompose_ref and apply_decomposed_ref (Python integers, pinned at these shapes by tests/test_hoist_reference.py)
and moddown_modes_ref.keyswitch_plain_ref.  Every comparison is word for word, from reduced inputs and from inputs spread over [0, 4q), into canary-filled
outputs."""
import numpy as np
import pytest

from gpu_util import canary, moduli_for, plan_for_moduli
from moddown_modes_ref import keyswitch_plain_ref
from rns_cases import TWO_FULL_DIGITS, WIDE, WIDE_IDS, WIDE_PRIMES, keyswitch_case, run_keyswitch
from rns_ref import apply_decomposed_ref, decompose_ref, digits_of, hoisted_ref, rotation_bound, rotation_deviation, rotation_key_case

pytestmark = pytest.mark.gpu

BATCH, G = 2, 5
T17 = 65537


def sizes_of(shape, n, batch):
    """(apply's scratch, ext, decompose's scratch, apply_decomposed's scratch) in words, from the header's formulas"""
    q_count, A, D = shape[0], shape[0] + shape[2], len(digits_of(shape))
    slab = batch * n
    return (q_count + (D + 2) * A) * slab, D * A * slab, q_count * slab, 2 * A * slab


def launches_of_the_parts(plan, shape):
    """(decompose, apply_decomposed) as the header composes them from the public calls' own reports: the inverse on Q (one launch at these sizes) + every
    ModUp basis' agx_ntt_basis_info -- one basis per digit onto the active primes, two (onto Q, onto P) when the special primes lie apart; the inner
    product + twice the ModDown basis' agx_ntt_basis_mod_down_info"""
    q_count, p_first, p_count, _ = shape
    up = 0
    for first, count in digits_of(shape):
        for df, dc in [(0, q_count + p_count)] if p_first == q_count else [(0, q_count), (p_first, p_count)]:
            basis = plan.basis(first, count, df, dc)
            up += basis.info()[4]
            basis.close()
    down = plan.basis(p_first, p_count, 0, q_count)
    second = 1 + 2 * down.mod_down_launches()
    down.close()
    return 1 + up, second


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


def _halves(dev, ks, chat, key, batch, g, out_words):
    """decompose into a canary-filled ext, then apply_decomposed(g) and accumulate_decomposed(w = NULL, accumulate = 0, g) + mod_down on it, every buffer
    of exactly the size hoisted_words reports; chat and key checked unchanged.  Returns (ext after decompose, apply_decomposed's out, the two halves' out,
    ext after everything)"""
    ext_words, dec_words, app_words = ks.hoisted_words(batch)
    d_chat, d_key = dev.to_device(chat), dev.to_device(key)
    d_ext, d_dec = dev.to_device(canary(0, ext_words)), dev.empty(dec_words)
    ks.decompose(d_chat.data_ptr(), d_ext.data_ptr(), d_dec.data_ptr(), batch, dev.stream)
    ext = dev.to_host(d_ext)
    d_out, d_app = dev.to_device(canary(0, out_words)), dev.empty(app_words)
    ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_app.data_ptr(), batch, g, dev.stream)
    d_acc, d_out2 = dev.to_device(canary(3, app_words)), dev.to_device(canary(7, out_words))
    ks.accumulate_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_acc.data_ptr(), batch, g, stream=dev.stream)
    ks.mod_down(d_acc.data_ptr(), d_out2.data_ptr(), batch, dev.stream)
    whole, halves = dev.to_host(d_out), dev.to_host(d_out2)
    assert np.array_equal(dev.to_host(d_chat), chat) and np.array_equal(dev.to_host(d_key), key), "an input changed"
    return ext, whole, halves, dev.to_host(d_ext)


def _check_shape(agx, orc, dev, n, shape):
    moduli = moduli_for(orc.find_prime, n, [60] * WIDE_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    chat, key, lchat, lkey, want = keyswitch_case(orc, n, moduli, shape, BATCH, 11 * n + sum(shape))
    want_ext = decompose_ref(orc, n, moduli, shape, chat).reshape(-1)
    want_g = apply_decomposed_ref(orc, n, moduli, shape, want_ext, key, BATCH, G).reshape(-1)
    ks = plan.keyswitch(*shape)
    # the handle's reports
    assert ks.info()[:5] == shape + (len(digits_of(shape)),)
    assert (ks.scratch_words(BATCH),) + ks.hoisted_words(BATCH) == sizes_of(shape, n, BATCH)
    assert ks.hoisted_info() == launches_of_the_parts(plan, shape) and ks.info()[5] == sum(ks.hoisted_info()), (n, shape)
    # the one call
    for name, c_words, k_words in (("reduced", chat, key), ("spread", lchat, lkey)):
        got = run_keyswitch(dev, ks, c_words, k_words, BATCH)
        assert np.array_equal(got, want), (n, shape, "apply", name, "first differing words", _first_bad(got, want))
    # the halves, and the second half in its own halves
    for name, c_words, k_words in (("reduced", chat, key), ("spread", lchat, lkey)):
        ext, whole, halves, ext_after = _halves(dev, ks, c_words, k_words, BATCH, G, want.size)
        assert np.array_equal(ext, want_ext), (n, shape, "decompose", name, "first differing words", _first_bad(ext, want_ext))
        assert np.array_equal(whole, want_g), (n, shape, "apply_decomposed", name, "first differing words", _first_bad(whole, want_g))
        assert np.array_equal(halves, whole), (n, shape, "accumulate_decomposed + mod_down", name, "first differing words", _first_bad(halves, whole))
        assert np.array_equal(ext_after, want_ext), (n, shape, "ext changed", name)
    ks.close()
    plan.close()


@pytest.mark.parametrize("shape", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", [64, 1024])
def test_every_call_at_wide_shapes(agx, orc, dev, n, shape):
    """apply equals keyswitch_ref; decompose equals decompose_ref; apply_decomposed(g = 5) equals apply_decomposed_ref; accumulate_decomposed (no weight,
    not accumulating) followed by mod_down equals apply_decomposed; ext stays as decompose wrote it; the sizes are the header's formulas and the launches
    the sum of the parts' own reports.  n = 64: the generic routes; n = 1024: the fused ones where they serve"""
    _check_shape(agx, orc, dev, n, shape)


def test_two_full_digits_at_4096(agx, orc, dev):
    """the default kernels of n = 4096 (the q = 2^60 - c forward among them) on 18 active primes"""
    _check_shape(agx, orc, dev, 4096, TWO_FULL_DIGITS)


def test_plaintext_modulus_with_special_primes_apart(agx, orc, dev):
    """a handle of agx_ntt_keyswitch_create_plain (t = 65537) on (13, 14, 7, 5) at n = 1024: ModDown from seven sources keeps the value modulo t"""
    n, shape = 1024, WIDE[1]
    moduli = moduli_for(orc.find_prime, n, [60] * WIDE_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    chat, key, lchat, lkey, plain = keyswitch_case(orc, n, moduli, shape, BATCH, 11 * n + sum(shape))
    want = keyswitch_plain_ref(orc, n, moduli, shape, chat, key, BATCH, T17).reshape(-1)
    assert not np.array_equal(want, plain), "t changes nothing: the case tests nothing"
    ks = plan.keyswitch(*shape, t=T17)
    for name, c_words, k_words in (("reduced", chat, key), ("spread", lchat, lkey)):
        got = run_keyswitch(dev, ks, c_words, k_words, BATCH)
        assert np.array_equal(got, want), (name, "first differing words", _first_bad(got, want))
    ks.close()
    plan.close()


def test_it_switches_rotated_keys_at_two_full_digits(agx, orc, dev):
    """the device's outputs with the noise-free rotation key of rns_ref.rotation_key_case on (12, 12, 6, 6), n = 64, g = 5: word for word the reference's,
    and out_0 + out_1 s - sigma_g(c) sigma_g(s), CRT-centred modulo Q, is at most p_count (1 + ||s||_1) at every coefficient -- a derived condition that
    tests/test_hoist_reference.py asserts of the reference on this very case"""
    n, shape = 64, TWO_FULL_DIGITS
    moduli = moduli_for(orc.find_prime, n, [60] * WIDE_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    chat, key, s, shat = rotation_key_case(orc, n, moduli, shape, G, BATCH, 1000 + sum(shape) + G)
    ks = plan.keyswitch(*shape)
    _, out, halves, _ = _halves(dev, ks, chat.reshape(-1), key.reshape(-1), BATCH, G, 2 * chat.size)
    ks.close()
    plan.close()
    assert np.array_equal(out, hoisted_ref(orc, n, moduli, shape, chat, key, BATCH, G).reshape(-1)) and np.array_equal(halves, out)
    worst, bound = rotation_deviation(orc, n, moduli, shape, G, BATCH, chat, shat, out), rotation_bound(shape, s)
    print(f"shape {shape}, g = {G}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, G, worst, bound)
