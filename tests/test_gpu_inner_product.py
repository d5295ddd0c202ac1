"""agx_ntt_inner_product on the device: c_o = sum_t a_t o bhat_{t,o} mod q on NTT-form frames, one launch, the key broadcast over the batch or not.

The expected words come from Python integers, from the definition (rns_ref.inner_ref): per word (sum_t (a_t mod q)(bhat_{t,o} mod q)) mod q.  Positions
are not interpreted by the call, so any words below 4q are NTT-form frames.  Every comparison is word for word."""
import numpy as np
import pytest

from gpu_util import Layout, arena_for, boundary_frames, canary, capture, moduli_for, plan_for_moduli, status_of
from rns_cases import TRIP, device_words, inner_layouts, inner_operands
from rns_ref import inner_ref, spread

pytestmark = pytest.mark.gpu


def _run(dev, plan, a, b, batch, terms, outputs, bhat_batch):
    """out of place into a canary-filled c; returns the output words [outputs][P][batch][n]"""
    d_a, d_b = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1))
    d_c = dev.to_device(canary(0, outputs * a[0].size))
    plan.inner_product(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, outputs, bhat_batch, dev.stream)
    return dev.to_host(d_c).reshape((outputs,) + a.shape[1:])


def _check(dev, plan, moduli, n, batch, terms, outputs, broadcast, seed, what):
    """reduced inputs and inputs spread over [0, 4q) must both give the reference's words"""
    a, b, la, lb = inner_operands(n, tuple(moduli), batch, seed)
    pick = lambda x: np.ascontiguousarray(x[:terms, :outputs, :, :1] if broadcast else x[:terms, :outputs])      # noqa: E731
    want = inner_ref(a[:terms], pick(b), moduli)
    for name, aw, bw in (("reduced", a, b), ("spread", la, lb)):
        got = _run(dev, plan, np.ascontiguousarray(aw[:terms]), pick(bw), batch, terms, outputs, 1 if broadcast else batch)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, name, "first differing (output, prime, frame, word)", bad[:4].tolist())
    return want


# ---- parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [1, 2, 3, 16])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])
def test_parity_60_bit(agx, orc, dev, n, batch, terms):
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for outputs in (1, 2):
        for broadcast in (True, False):
            _check(dev, plan, moduli, n, batch, terms, outputs, broadcast, n + batch, (n, batch, terms, outputs, broadcast))
    plan.close()


def test_parity_at_32768(agx, orc, dev):
    n = 32768
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(dev, plan, moduli, n, 2, 3, 2, True, 32768, "n = 32768")
    plan.close()


def test_sixteen_terms_under_a_62_bit_prime(agx, orc, dev):
    """the accumulation edge: sixteen products of (q - 1)^2 with q just below 2^62 -- the largest 128-bit sum the contract allows -- in the first half
    of each frame, random operands in the second half"""
    n, batch, terms = 1024, 3, 16
    moduli = tuple(agx.find_primes(62, n, 1))
    assert moduli[0] > (1 << 62) - (1 << 40)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    rng = np.random.default_rng(62)
    a = rng.integers(0, moduli[0], size=(terms, 1, batch, n), dtype=np.uint64)
    a[..., :n // 2] = moduli[0] - 1
    for outputs, bb in ((2, 1), (2, batch), (1, 1)):
        b = rng.integers(0, moduli[0], size=(terms, outputs, 1, bb, n), dtype=np.uint64)
        b[..., :n // 2] = moduli[0] - 1
        want = inner_ref(a, b, moduli)
        assert int(want[0, 0, 0, 0]) == 16 * (moduli[0] - 1) ** 2 % moduli[0]
        for aw, bw in ((a, b), (spread(rng, a, moduli, 1), spread(rng, b, moduli, 2))):
            assert np.array_equal(_run(dev, plan, aw, bw, batch, terms, outputs, bb), want), (outputs, bb)
    plan.close()


@pytest.mark.parametrize("widths", [[30] * 4, [60, 30, 61, 30]], ids=["30-bit", "mixed"])
def test_other_moduli(agx, orc, dev, widths):
    n, batch = 1024, 5
    moduli = moduli_for(orc.find_prime, n, widths)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for terms, outputs, broadcast in ((3, 2, True), (16, 2, False), (2, 1, True)):
        _check(dev, plan, moduli, n, batch, terms, outputs, broadcast, 1024 + widths[1], (widths, terms, outputs, broadcast))
    plan.close()


def test_one_term_one_output_is_pointwise(agx, orc, dev):
    n, batch = 4096, 5
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 60])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, la, lb = inner_operands(n, tuple(moduli), batch, 77)
    a, b = np.ascontiguousarray(la[:1]), np.ascontiguousarray(lb[:1, :1])
    got = _run(dev, plan, a, b, batch, 1, 1, batch)
    d_a, d_b, d_c = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1)), dev.empty(a.size)
    plan.pointwise(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, dev.stream)
    assert np.array_equal(got.reshape(-1), dev.to_host(d_c))
    plan.close()


# ---- variants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_every_variant_and_a_forward_only_plan(agx, orc, dev, n):
    batch, terms, outputs = 5, 3, 2
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    want = None
    for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_REGBLOCK, agx.VARIANT_AUTO):
        plan.set_variant(variant)
        want = _check(dev, plan, moduli, n, batch, terms, outputs, True, n + 3, ("variant", variant))
    plan.close()
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    a, b, _, _ = inner_operands(n, tuple(moduli), batch, n + 3)
    got = _run(dev, fwd_only, np.ascontiguousarray(a[:terms]), np.ascontiguousarray(b[:terms, :outputs, :, :1]), batch, terms, outputs, 1)
    assert np.array_equal(got, want), "a forward-only plan"
    fwd_only.close()


# ---- placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)], ids=["16-byte", "odd", "c odd", "key odd", "a odd"])
@pytest.mark.parametrize("n,batch", [(8, 5), (4096, 3)])
def test_alignment_and_guard_bands(agx, orc, dev, n, batch, offsets):
    """every base 16-byte aligned (the 16-byte kernel), every base at an odd word, one base odd (8-byte accesses for all three): the same words, a
    and bhat unchanged, and every word outside c as it was"""
    terms, outputs = 3, 2
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 60])
    P = len(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, la_w, lb_w = inner_operands(n, tuple(moduli), batch, n + 11)
    for broadcast in (True, False):
        a = np.ascontiguousarray(la_w[:terms])
        b = np.ascontiguousarray(lb_w[:terms, :outputs, :, :1] if broadcast else lb_w[:terms, :outputs])
        want = inner_ref(a, b, moduli)
        la, lb, lc = inner_layouts(n, P, batch, terms, outputs, 1 if broadcast else batch, offsets)
        arena = arena_for(dev, n, (la, a), (lb, b), (lc, None))
        assert arena.address(0) % 16 == 0
        plan.inner_product(arena.address(la.offset), arena.address(lb.offset), arena.address(lc.offset), batch, terms, outputs, 1 if broadcast else batch, dev.stream)
        img = arena.image()
        assert not arena.faults([(la, a), (lb, b), (lc, None)], img), ("a word outside c changed", offsets, broadcast)
        assert np.array_equal(arena.frames(lc, img), want.reshape(-1)), (offsets, broadcast)
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_rejected_calls_write_nothing(agx, orc, dev, n):
    batch, terms, outputs = 2, 2, 2
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
    I = plan.inner_product      # noqa: E741  (d_a, d_bhat, d_c, batch, terms, outputs, bhat_batch, stream)
    for k in range(3):      # NULL pointers
        args = [pa, pb, pc]
        args[k] = 0
        assert status_of(agx, I, *args, batch, terms, outputs, batch, st) == 1
    for t, o, bb in ((0, 2, batch), (17, 2, batch), (2, 0, batch), (2, 3, batch), (2, 2, 3), (2, 2, 0)):      # counts
        assert status_of(agx, I, pa, pb, pc, batch, t, o, bb, st) == 5, (t, o, bb)
    assert status_of(agx, I, 0, pb, pc, batch, 17, outputs, batch, st) == 1      # the NULL rule comes first
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
    I(pa, pb, pa, 0, terms, outputs, 1, st)
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # ranges that meet end to end are accepted: a | bhat | c back to back, and a broadcast key's shorter range frees the words behind it
    packed = arena_for(dev, n, (Layout(n, terms * P, batch, offset=0), a), (Layout(n, terms * outputs * P, batch, offset=a_words), b),
                       (Layout(n, outputs * P, batch, offset=a_words + b_words), None))
    base = packed.address(0)
    I(base, base + w * a_words, base + w * (a_words + b_words), batch, terms, outputs, batch, st)
    assert np.array_equal(packed.frames(Layout(n, outputs * P, batch, offset=a_words + b_words)), inner_ref(a, b, moduli).reshape(-1))
    plan.close()


# ---- a second grid-stride trip ------------------------------------------------------------------------------------------------------
def test_second_trip_30_bit_every_word(agx, orc, dev):
    """n = 4096, 16-byte accesses: 2048 pairs per frame, so 2,049 frames are the fewest whose per-prime work passes one trip.  Two terms, two outputs,
    one prime, broadcast key; with a 30-bit prime products stay below 2^60 and the sum of two below 2^61, so torch int64 judges every word"""
    torch = dev.torch
    n, terms, outputs = 4096, 2, 2
    batch = TRIP // (n // 2) + 1
    assert batch == 2049 and (batch - 1) * (n // 2) <= TRIP < batch * (n // 2)
    moduli = moduli_for(orc.find_prime, n, [30])
    q = int(moduli[0])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    d_a, d_b = device_words(torch, dev, terms * batch * n, q, 1), device_words(torch, dev, terms * outputs * n, q, 2)
    d_c = dev.empty(outputs * batch * n)
    d_c.fill_(-1)
    assert all(t.data_ptr() % 16 == 0 for t in (d_a, d_b, d_c))
    plan.inner_product(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, outputs, 1, dev.stream)
    dev.sync()
    av, bv, cv = d_a.view(terms, batch, n) % q, d_b.view(terms, outputs, 1, n) % q, d_c.view(outputs, batch, n)
    for o in range(outputs):
        want = (av[0] * bv[0, o] + av[1] * bv[1, o]) % q
        if not torch.equal(cv[o], want):
            bad = (cv[o] != want).nonzero()[:4].tolist()
            pytest.fail(f"output {o}: first differing (frame, word) {bad}")
    plan.close()


def test_second_trip_60_bit_boundary_frames(agx, orc, dev):
    """n = 4096, 8-byte accesses (every base at an odd word): one word per work item, so 1,025 frames are the fewest past one trip.  A 60-bit prime;
    the boundary frames, the two sides of the trip's end among them, against Python integers"""
    torch = dev.torch
    n, terms, outputs = 4096, 2, 2
    batch = TRIP // n + 1
    assert batch == 1025
    moduli = moduli_for(orc.find_prime, n, [60])
    q = int(moduli[0])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    d_a, d_b = device_words(torch, dev, terms * batch * n + 1, q, 3), device_words(torch, dev, terms * outputs * n + 1, q, 4)
    d_c = dev.empty(outputs * batch * n + 1)
    d_c.fill_(-1)
    plan.inner_product(d_a.data_ptr() + 8, d_b.data_ptr() + 8, d_c.data_ptr() + 8, batch, terms, outputs, 1, dev.stream)
    dev.sync()
    frames = boundary_frames(batch)
    assert batch - 2 in frames and batch - 1 in frames
    a = dev.to_host(d_a[1:].view(terms, 1, batch, n)[:, :, frames].contiguous())
    b = dev.to_host(d_b[1:]).reshape(terms, outputs, 1, 1, n)
    got = dev.to_host(d_c[1:].view(outputs, 1, batch, n)[:, :, frames].contiguous())
    want = inner_ref(a, b, moduli)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (output, prime, listed frame, word)", bad[:4].tolist(), frames)
    assert int(d_c[0]) == -1, "the word in front of c changed"
    plan.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_calls_are_graph_capturable(agx, orc, dev, n):
    """one call captured on a side stream (no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    batch, terms, outputs = 5, 3, 2
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    first, second = inner_operands(n, tuple(moduli), batch, n + 5), inner_operands(n, tuple(moduli), batch, n + 6)
    pick = lambda ops: (np.ascontiguousarray(ops[2][:terms]), np.ascontiguousarray(ops[3][:terms, :outputs, :, :1]))      # noqa: E731
    a, b = pick(first)
    d_a, d_b, d_c = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1)), dev.empty(outputs * a[0].size)

    def call(s):
        plan.inner_product(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, outputs, 1, s)

    graph = capture(dev, call, call)
    for ops in (second, first):
        a, b = pick(ops)
        d_a.copy_(torch.from_numpy(a.reshape(-1).view(np.int64).copy()))
        d_b.copy_(torch.from_numpy(b.reshape(-1).view(np.int64).copy()))
        d_c.zero_()
        graph.replay()
        dev.sync()
        want = inner_ref(a, b, moduli)
        assert np.array_equal(dev.to_host(d_c), want.reshape(-1)), "replay"
        assert np.array_equal(_run(dev, plan, a, b, batch, terms, outputs, 1), want), "direct call"
    plan.close()
