"""agx_ntt_inner_product_galois on the device: c_o[i] = sum_t a_t[pi_g(i)] o bhat_{t,o}[i] mod q, one launch, no permuted copy of a.

The expected words come from Python integers: rns_ref.inner_ref applied to a[..., ntt_pi(n, g)].  The call is also held
against the device pair it replaces -- agx_ntt_automorphism(AGX_FORM_NTT, g) on a, then agx_ntt_inner_product -- and, at g = 1, against
agx_ntt_inner_product itself.  Every comparison is word for word."""
import functools

import numpy as np
import pytest

from gpu_util import Layout, arena_for, canary, capture, moduli_for, ntt_pi, plan_for_moduli, status_of
from rns_cases import TRIP, device_words, inner_layouts, inner_operands
from rns_ref import inner_ref, spread

pytestmark = pytest.mark.gpu


def elements(n):
    """1 (the plain kernel), two small ones, -1 (conjugation) and the inverse of the rotation generator"""
    return (1, 3, 5, 2 * n - 1, pow(5, -1, 2 * n))


@functools.lru_cache(maxsize=None)
def _want(n, moduli, batch, seed, terms, broadcast, g):
    """inner_ref on a[..., pi_g] for two outputs, once per case (read-only); one output is its first half"""
    a, b, _, _ = inner_operands(n, moduli, batch, seed)
    bb = np.ascontiguousarray(b[:terms, :, :, :1] if broadcast else b[:terms])
    want = inner_ref(np.ascontiguousarray(a[:terms][..., ntt_pi(n, g)]), bb, moduli)
    want.setflags(write=False)
    return want


def _run(dev, plan, a, b, batch, terms, outputs, bhat_batch, g):
    """out of place into a canary-filled c; returns the output words [outputs][P][batch][n] and checks a and bhat unchanged"""
    d_a, d_b = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1))
    d_c = dev.to_device(canary(0, outputs * a[0].size))
    plan.inner_product_galois(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, g, outputs, bhat_batch, dev.stream)
    got = dev.to_host(d_c).reshape((outputs,) + a.shape[1:])
    assert np.array_equal(dev.to_host(d_a), a.reshape(-1)) and np.array_equal(dev.to_host(d_b), b.reshape(-1)), "an input changed"
    return got


def _check(dev, plan, moduli, n, batch, terms, seed, what):
    """outputs 1 and 2, both key forms, every element, reduced inputs and inputs spread over [0, 4q): the reference's words"""
    a, b, la, lb = inner_operands(n, tuple(moduli), batch, seed)
    for g in elements(n):
        for broadcast in (True, False):
            want = _want(n, tuple(moduli), batch, seed, terms, broadcast, g)
            for outputs in (1, 2):
                pick = lambda x: np.ascontiguousarray(x[:terms, :outputs, :, :1] if broadcast else x[:terms, :outputs])      # noqa: E731
                for name, aw, bw in (("reduced", a, b), ("spread", la, lb)):
                    got = _run(dev, plan, np.ascontiguousarray(aw[:terms]), pick(bw), batch, terms, outputs, 1 if broadcast else batch, g)
                    bad = np.argwhere(got != want[:outputs])
                    assert bad.size == 0, (what, g, broadcast, outputs, name, "first differing (output, prime, frame, word)", bad[:4].tolist())


# ---- parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [1, 3, 4, 5, 16])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])
def test_parity_60_bit(agx, orc, dev, n, batch, terms):
    moduli = moduli_for(orc.find_prime, n, [60] * 2)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(dev, plan, moduli, n, batch, terms, n + batch, (n, batch, terms))
    plan.close()


def test_sixteen_terms_under_a_62_bit_prime(agx, orc, dev):
    """the accumulation edge through the gather: sixteen products of (q - 1)^2 with q just below 2^62 wherever pi_g lands in the first frame (all of
    it q - 1 in a, the first half of every key frame q - 1), random operands elsewhere"""
    n, batch, terms = 1024, 3, 16
    moduli = tuple(agx.find_primes(62, n, 1))
    assert moduli[0] > (1 << 62) - (1 << 40)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    rng = np.random.default_rng(62)
    a = rng.integers(0, moduli[0], size=(terms, 1, batch, n), dtype=np.uint64)
    a[:, :, 0, :] = moduli[0] - 1
    for g in (5, 2 * n - 1):
        for outputs, bb in ((2, 1), (2, batch), (1, 1)):
            b = rng.integers(0, moduli[0], size=(terms, outputs, 1, bb, n), dtype=np.uint64)
            b[..., :n // 2] = moduli[0] - 1
            want = inner_ref(a[..., ntt_pi(n, g)], b, moduli)
            assert int(want[0, 0, 0, 0]) == int(want[0, 0, 0, n // 2 - 1]) == 16 * (moduli[0] - 1) ** 2 % moduli[0]
            for aw, bw in ((a, b), (spread(rng, a, moduli, 1), spread(rng, b, moduli, 2))):
                assert np.array_equal(_run(dev, plan, aw, bw, batch, terms, outputs, bb, g), want), (g, outputs, bb)
    plan.close()


@pytest.mark.parametrize("widths", [[30] * 4, [60, 30, 61, 30]], ids=["30-bit", "mixed"])
def test_other_moduli(agx, orc, dev, widths):
    n, batch = 1024, 5
    moduli = moduli_for(orc.find_prime, n, widths)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    a, b, la, lb = inner_operands(n, tuple(moduli), batch, 1024 + widths[1])
    for terms, outputs, broadcast, g in ((3, 2, True, 5), (16, 2, False, 2 * n - 1), (2, 1, True, 3)):
        pick = lambda x: np.ascontiguousarray(x[:terms, :outputs, :, :1] if broadcast else x[:terms, :outputs])      # noqa: E731
        want = inner_ref(a[:terms][..., ntt_pi(n, g)], pick(b), moduli)
        for aw, bw in ((a, b), (la, lb)):
            got = _run(dev, plan, np.ascontiguousarray(aw[:terms]), pick(bw), batch, terms, outputs, 1 if broadcast else batch, g)
            assert np.array_equal(got, want), (widths, terms, outputs, broadcast, g)
    plan.close()


# ---- against the device calls it stands for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64, 4096])
def test_it_is_automorphism_then_inner_product(agx, orc, dev, n):
    """agx_ntt_automorphism(AGX_FORM_NTT, g) over the terms P slabs of a, then agx_ntt_inner_product: the same words; and g = 1 is agx_ntt_inner_product"""
    batch, terms, outputs = 5, 3, 2
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 60])
    P = len(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, la, lb = inner_operands(n, tuple(moduli), batch, n + 17)
    a = np.ascontiguousarray(la[:terms])
    for broadcast in (True, False):
        b = np.ascontiguousarray(lb[:terms, :outputs, :, :1] if broadcast else lb[:terms, :outputs])
        bb = 1 if broadcast else batch
        d_a, d_b = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1))
        d_perm, d_c = dev.empty(a.size), dev.empty(outputs * a[0].size)
        for g in elements(n):
            for t in range(terms):      # the automorphism moves words only, so a plan of P primes serves one term's P slabs
                plan.automorphism(d_a.data_ptr() + 8 * t * P * batch * n, d_perm.data_ptr() + 8 * t * P * batch * n, batch, g, agx.FORM_NTT, dev.stream)
            plan.inner_product((d_a if g == 1 else d_perm).data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, outputs, bb, dev.stream)
            pair = dev.to_host(d_c)
            got = _run(dev, plan, a, b, batch, terms, outputs, bb, g)
            assert np.array_equal(got.reshape(-1), pair), (g, broadcast)
    plan.close()


# ---- placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)], ids=["16-byte", "odd", "c odd", "key odd", "a odd"])
@pytest.mark.parametrize("n,batch", [(8, 5), (4096, 3)])
def test_alignment_and_guard_bands(agx, orc, dev, n, batch, offsets):
    """every base 16-byte aligned (the pair form), every base at an odd word, one base odd (8-byte accesses for all three): the same words, a and
    bhat unchanged, and every word outside c as it was"""
    terms, outputs, g = 3, 2, 5
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 60])
    P = len(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, la_w, lb_w = inner_operands(n, tuple(moduli), batch, n + 11)
    for broadcast in (True, False):
        a = np.ascontiguousarray(la_w[:terms])
        b = np.ascontiguousarray(lb_w[:terms, :outputs, :, :1] if broadcast else lb_w[:terms, :outputs])
        want = inner_ref(a[..., ntt_pi(n, g)], b, moduli)
        la, lb, lc = inner_layouts(n, P, batch, terms, outputs, 1 if broadcast else batch, offsets)
        arena = arena_for(dev, n, (la, a), (lb, b), (lc, None))
        assert arena.address(0) % 16 == 0
        plan.inner_product_galois(arena.address(la.offset), arena.address(lb.offset), arena.address(lc.offset), batch, terms, g, outputs,
                                  1 if broadcast else batch, dev.stream)
        img = arena.image()
        assert not arena.faults([(la, a), (lb, b), (lc, None)], img), ("a word outside c changed", offsets, broadcast)
        assert np.array_equal(arena.frames(lc, img), want.reshape(-1)), (offsets, broadcast)
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_rejected_calls_write_nothing(agx, orc, dev, n):
    batch, terms, outputs, g = 2, 2, 2, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 2)
    P = len(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    aw, bw, _, _ = inner_operands(n, tuple(moduli), batch, 5 * n)
    a, b = np.ascontiguousarray(aw[:terms]), np.ascontiguousarray(bw[:terms, :outputs])
    la = Layout(n, terms * P, batch, offset=0)
    lb = Layout(n, terms * outputs * P, batch, offset=la.span() + 2 * n)
    lc = Layout(n, outputs * P, batch, offset=lb.span() + 2 * n)
    arena = arena_for(dev, n, (la, a), (lb, b), (lc, None))
    before = arena.image()
    pa, pb, pc = (arena.address(l.offset) for l in (la, lb, lc))
    st, w = dev.stream, 8
    a_words, b_words, c_words = a.size, b.size, outputs * P * batch * n

    def I(d_a, d_bhat, d_c, batch_, terms_, outputs_, bhat_batch, stream, elt=g):      # noqa: E743  (the plain call's argument order, the element last)
        plan.inner_product_galois(d_a, d_bhat, d_c, batch_, terms_, elt, outputs_, bhat_batch, stream)

    for elt in (0, 2, 4, 2 * n - 2, 2 * n, 2 * n + 1, 4 * n + 5, 0xfffffffe, 0xffffffff):      # even, 0, 2n, 2n + 1 and beyond
        assert status_of(agx, I, pa, pb, pc, batch, terms, outputs, batch, st, elt) == 5, elt
    assert status_of(agx, I, 0, pb, pc, batch, terms, outputs, batch, st, 4) == 1      # the NULL rule comes first
    # every rejection the plain call has, with a good element
    for k in range(3):      # NULL pointers
        args = [pa, pb, pc]
        args[k] = 0
        assert status_of(agx, I, *args, batch, terms, outputs, batch, st) == 1
    for t, o, bb in ((0, 2, batch), (17, 2, batch), (2, 0, batch), (2, 3, batch), (2, 2, 3), (2, 2, 0)):      # counts
        assert status_of(agx, I, pa, pb, pc, batch, t, o, bb, st) == 5, (t, o, bb)
    assert status_of(agx, I, 0, pb, pc, batch, 17, outputs, batch, st) == 1
    for k in range(3):      # uint64_t data
        args = [pa, pb, pc]
        args[k] += 4
        assert status_of(agx, I, *args, batch, terms, outputs, batch, st) == 5
    assert status_of(agx, I, pa, pb, pc, 1 << 40, terms, outputs, 1, st) == 5      # a batch past the grid limit
    assert status_of(agx, I, pa, pb, pc, 1 << 62, terms, outputs, 1, st) == 5      # terms P batch n would wrap 64 bits
    assert status_of(agx, I, pa, pb, pc, (1 << 64) - 1, 16, 2, 1, st) == 5
    assert status_of(agx, I, pa, pb, pa, batch, terms, outputs, batch, st) == 5                            # c is a: out of place only
    assert status_of(agx, I, pa, pb, pb, batch, terms, outputs, batch, st) == 5                            # c is bhat
    assert status_of(agx, I, pa, pb, pa + w * (a_words - 1), batch, terms, outputs, batch, st) == 5        # c's first word is a's last
    assert status_of(agx, I, pa, pb, pa - w * (c_words - 1), batch, terms, outputs, batch, st) == 5        # c's last word is a's first
    assert status_of(agx, I, pa, pb, pb + w * (b_words - 1), batch, terms, outputs, batch, st) == 5
    assert status_of(agx, I, pa, pb, pb - w * (c_words - 1), batch, terms, outputs, batch, st) == 5
    assert status_of(agx, I, pa, pb, pb + w * (terms * outputs * P * n - 1), batch, terms, outputs, 1, st) == 5      # the broadcast key's last word
    assert status_of(agx, I, pa, pb, pb + w * (n // 2), batch, 1, 1, 1, st) == 5
    I(pa, pb, pc, 0, terms, outputs, 0, st)      # empty batch: nothing launched
    assert status_of(agx, I, pa, pb, pc, 0, terms, outputs, 0, st, 2) == 5      # but a bad element is still one
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # ranges that meet end to end are accepted: a | bhat | c back to back
    packed = arena_for(dev, n, (Layout(n, terms * P, batch, offset=0), a), (Layout(n, terms * outputs * P, batch, offset=a_words), b),
                       (Layout(n, outputs * P, batch, offset=a_words + b_words), None))
    base = packed.address(0)
    I(base, base + w * a_words, base + w * (a_words + b_words), batch, terms, outputs, batch, st)
    assert np.array_equal(packed.frames(Layout(n, outputs * P, batch, offset=a_words + b_words)), inner_ref(a[..., ntt_pi(n, g)], b, moduli).reshape(-1))
    plan.close()


# ---- a second grid-stride trip of each width ------------------------------------------------------------------------------------------
def _second_trip(agx, orc, dev, batch, shift):
    """n = 4096, one 30-bit prime, two terms, two outputs, broadcast key, g = 5: products stay below 2^60 and the sum of two below 2^61, so torch
    int64 judges every word on the device.  shift: 0 = every base 16-byte aligned, 1 = every base 8 bytes further"""
    torch = dev.torch
    n, terms, outputs, g = 4096, 2, 2, 5
    moduli = moduli_for(orc.find_prime, n, [30])
    q = int(moduli[0])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    d_a, d_b = device_words(torch, dev, terms * batch * n + shift, q, 1), device_words(torch, dev, terms * outputs * n + shift, q, 2)
    d_c = dev.empty(outputs * batch * n + shift)
    d_c.fill_(-1)
    assert all(t.data_ptr() % 16 == 0 for t in (d_a, d_b, d_c))
    plan.inner_product_galois(d_a.data_ptr() + 8 * shift, d_b.data_ptr() + 8 * shift, d_c.data_ptr() + 8 * shift, batch, terms, g, outputs, 1, dev.stream)
    dev.sync()
    pi = torch.from_numpy(ntt_pi(n, g)).to(dev.device)
    av, bv, cv = d_a[shift:].view(terms, batch, n) % q, d_b[shift:].view(terms, outputs, 1, n) % q, d_c[shift:].view(outputs, batch, n)
    for o in range(outputs):
        want = (av[0][:, pi] * bv[0, o] + av[1][:, pi] * bv[1, o]) % q
        if not torch.equal(cv[o], want):
            pytest.fail(f"output {o}: first differing (frame, word) {(cv[o] != want).nonzero()[:4].tolist()}")
    if shift:
        assert int(d_c[0]) == -1, "the word in front of c changed"
    plan.close()


def test_second_trip_pair_form_every_word(agx, orc, dev):
    """2048 pairs per frame: 2,049 frames are the fewest whose per-prime work passes one trip of the 16-byte form"""
    batch = TRIP // (4096 // 2) + 1
    assert batch == 2049
    _second_trip(agx, orc, dev, batch, 0)


def test_second_trip_word_form_every_word(agx, orc, dev):
    """every base offset by 8 bytes: one word per work item, so 1,025 frames are the fewest past one trip"""
    batch = TRIP // 4096 + 1
    assert batch == 1025
    _second_trip(agx, orc, dev, batch, 1)


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_calls_are_graph_capturable(agx, orc, dev, n):
    """one call captured on a side stream (no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    batch, terms, outputs, g = 5, 3, 2, 2 * n - 1
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    first, second = inner_operands(n, tuple(moduli), batch, n + 5), inner_operands(n, tuple(moduli), batch, n + 6)
    pick = lambda ops: (np.ascontiguousarray(ops[2][:terms]), np.ascontiguousarray(ops[3][:terms, :outputs, :, :1]))      # noqa: E731
    a, b = pick(first)
    d_a, d_b, d_c = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1)), dev.empty(outputs * a[0].size)

    def call(s):
        plan.inner_product_galois(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, g, outputs, 1, s)

    graph = capture(dev, call, call)
    for ops in (second, first):
        a, b = pick(ops)
        d_a.copy_(torch.from_numpy(a.reshape(-1).view(np.int64).copy()))
        d_b.copy_(torch.from_numpy(b.reshape(-1).view(np.int64).copy()))
        d_c.zero_()
        graph.replay()
        dev.sync()
        want = inner_ref(a[..., ntt_pi(n, g)], b, moduli)
        assert np.array_equal(dev.to_host(d_c), want.reshape(-1)), "replay"
    plan.close()
