"""agx_ntt_keyswitch_* on the device: the RNS hybrid key switch of one ciphertext component in one call, NTT form in and out, at any level.

The reference is rns_ref.keyswitch_ref: the four-step definition of include/agx_ntt.h in Python integers, with the CPU oracle's forward and inverse
transforms:
  1. c_j = INTT_j(chat_j);   2. per digit d, V_d = sum_i y_i D_{d,i} with y_i = c_i D_{d,i}^-1 mod q_i, e_{d,j} = V_d mod q_j for every active j;
  3. acc_{o,j} = sum_d NTT_j(e_{d,j}) o key_{d,o,j} mod q_j;   4. out_{o,j} = NTT_j((INTT_j(acc_{o,j}) - V) D_P^-1 mod q_j), V the lift of acc_o's special slabs.
Every comparison is word for word."""
import numpy as np
import pytest

from gpu_util import Layout, arena_for, capture, moduli_for, plan_for_moduli, status_of
from rns_cases import LOWER, SHAPE_IDS, SHAPES, TOP, keyswitch_case, run_keyswitch
from rns_ref import active_of, digits_of, oracle_forward_set, oracle_inverse_set, product, ternary

pytestmark = pytest.mark.gpu


def _check(orc, dev, plan, n, moduli, shape, batch, seed, what):
    chat, key, lchat, lkey, want = keyswitch_case(orc, n, tuple(moduli), shape, batch, seed)
    ks = plan.keyswitch(*shape)
    q_count, p_first, p_count, alpha, digits, _ = ks.info()
    assert (q_count, p_first, p_count, alpha) == shape and digits == len(digits_of(shape))
    assert ks.scratch_words(batch) == (q_count + (digits + 2) * (q_count + p_count)) * batch * n
    for name, c_words, k_words in (("reduced", chat, key), ("spread", lchat, lkey)):
        got = run_keyswitch(dev, ks, c_words, k_words, batch)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, name, "first differing words", bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    ks.close()
    return want


# ---- parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])
def test_parity_60_bit(agx, orc, dev, n, batch, shape):
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(orc, dev, plan, n, moduli, shape, batch, n * 7 + batch + shape[0], (n, batch, shape))
    plan.close()


def test_parity_lower_level_at_32768(agx, orc, dev):
    n = 32768
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(orc, dev, plan, n, moduli, LOWER, 1, 32768, "n = 32768")
    plan.close()


@pytest.mark.parametrize("n,widths", [(64, [30] * 6), (4096, [30] * 6), (1024, [60, 30, 61, 30, 60, 60])], ids=["30-bit-64", "30-bit-4096", "mixed-1024"])
def test_parity_other_moduli(agx, orc, dev, n, widths):
    moduli = moduli_for(orc.find_prime, n, widths)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(orc, dev, plan, n, moduli, TOP, 5, n + widths[1], (n, widths))
    plan.close()


# ---- composition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_one_call_equals_the_public_calls(agx, orc, dev, n):
    """top level (the active primes are the whole plan): inverse on a Q-plan with the same roots, basis_extend to NTT form per digit, one
    inner_product, two basis_mod_down -- word for word what the one call writes"""
    batch, shape = 5, TOP
    q_count, p_first, p_count, alpha = shape
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    qplan, _ = plan_for_moduli(agx, orc, n, moduli[:q_count])
    _, _, lchat, lkey, want = keyswitch_case(orc, n, tuple(moduli), shape, batch, n + 41)
    ks = plan.keyswitch(*shape)
    assert np.array_equal(run_keyswitch(dev, ks, lchat, lkey, batch), want)
    A, digs, slab, st = q_count + p_count, digits_of(shape), batch * n, dev.stream
    d_chat, d_key = dev.to_device(lchat), dev.to_device(lkey)
    d_c, d_ext, d_acc, d_out = dev.empty(q_count * slab), dev.empty(len(digs) * A * slab), dev.empty(2 * A * slab), dev.empty(2 * q_count * slab)
    qplan.inverse(d_chat.data_ptr(), d_c.data_ptr(), batch, st)
    for d, (first, count) in enumerate(digs):
        up = plan.basis(first, count, 0, A)
        up.extend(d_c.data_ptr() + 8 * first * slab, d_ext.data_ptr() + 8 * d * A * slab, batch, agx.FORM_NTT, st)
        dev.sync()
        up.close()
    plan.inner_product(d_ext.data_ptr(), d_key.data_ptr(), d_acc.data_ptr(), batch, len(digs), 2, 1, st)
    down = plan.basis(p_first, p_count, 0, q_count)
    for o in range(2):
        xq = d_acc.data_ptr() + 8 * o * A * slab
        down.mod_down(xq, xq + 8 * q_count * slab, d_out.data_ptr() + 8 * o * q_count * slab, xq + 8 * q_count * slab, batch, st)
    assert np.array_equal(dev.to_host(d_out), want), "the composition of public calls differs"
    down.close()
    ks.close()
    qplan.close()
    plan.close()


# ---- it switches keys -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + ((3, 3, 3, 2),), ids=SHAPE_IDS + ["three-special"])
def test_it_switches_keys(agx, orc, dev, shape):
    """A noise-free key: key_{d,1} = a_d random, key_{d,0} = -a_d s + D_P G_d s' with G_d = (Q / D_d) [(Q / D_d)^-1 mod D_d], ternary s of Hamming
    weight 8, ternary s'.  Then out_0 + out_1 s - c s', lifted by CRT to the centred range modulo Q, is what the two approximate conversions leave:
    0 <= V < S D in both gives |.| <= p_count (1 + ||s||_1) at every coefficient -- a condition, not a measurement"""
    n, batch = 64, 2
    q_count, p_first, p_count, alpha = shape
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    active = active_of(moduli, shape)
    Q, A, digs = active[:q_count], len(active), digits_of(shape)
    Qp, DP = product(Q), product(active[q_count:])
    rng = np.random.default_rng(1000 + sum(shape))
    s, s2 = ternary(rng, n, 8), ternary(rng, n)
    shat = oracle_forward_set(orc, n, active, np.stack([(s % int(q)).astype(np.uint64) for q in active]))
    s2hat = oracle_forward_set(orc, n, active, np.stack([(s2 % int(q)).astype(np.uint64) for q in active]))
    key = np.empty((len(digs), 2, A, n), dtype=np.uint64)
    for d, (first, count) in enumerate(digs):
        Dd = product(Q[first:first + count])
        G = (Qp // Dd) * pow(Qp // Dd, -1, Dd)
        for j, q in enumerate(active):
            ahat = rng.integers(0, int(q), size=n, dtype=np.uint64)
            key[d, 1, j] = ahat
            key[d, 0, j] = ((DP * G % int(q)) * s2hat[j].astype(object) - ahat.astype(object) * shat[j].astype(object)) % int(q)
    chat = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in Q])
    ks = plan.keyswitch(*shape)
    out = run_keyswitch(dev, ks, chat.reshape(-1), key.reshape(-1), batch).reshape(2, q_count, batch, n)
    ks.close()
    plan.close()
    # (out_0 + out_1 s - c s') per prime of Q in NTT form, back through the oracle's inverse, then CRT to the centred range
    dhat = np.stack([((out[0, j].astype(object) + out[1, j].astype(object) * shat[j].astype(object) - chat[j].astype(object) * s2hat[j].astype(object)) % int(q)).astype(np.uint64)
                     for j, q in enumerate(Q)])
    dev_res = oracle_inverse_set(orc, n, Q, dhat)
    X = np.zeros(batch * n, dtype=object)
    for j, q in enumerate(Q):
        X = X + dev_res[j].astype(object) * ((Qp // int(q)) * pow(Qp // int(q), -1, int(q)))
    X = X % Qp
    centred = np.array([int(x) - Qp if int(x) > Qp // 2 else int(x) for x in X], dtype=object)
    worst, bound = max(abs(int(x)) for x in centred), p_count * (1 + int(np.abs(s).sum()))
    print(f"shape {shape}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, worst, bound)


# ---- placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
@pytest.mark.parametrize("n,odd", [(64, True), (4096, True), (4096, False)])
def test_guard_bands_and_odd_placement(agx, orc, dev, n, odd, shape):
    """all four buffers in one arena, at odd words (no frame starts on a 16-byte boundary) or at even ones: the right words, chat and keyhat
    unchanged, and every word outside out and the scratch as it was"""
    batch = 3
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    q_count, A, D = shape[0], shape[0] + shape[2], len(digits_of(shape))
    _, _, chat, key, want = keyswitch_case(orc, n, tuple(moduli), shape, batch, n + 23)
    place = lambda off: off + (off % 2 != (1 if odd else 0))      # noqa: E731
    lc = Layout(n, q_count, batch, offset=place(0))
    lk = Layout(n, D * 2 * A, 1, offset=place(lc.span() + 5))
    lo = Layout(n, 2 * q_count, batch, offset=place(lk.span() + 5))
    ls = Layout(n, ks.scratch_words(batch) // (batch * n), batch, offset=place(lo.span() + 5))
    assert all(l.offset % 2 == (1 if odd else 0) for l in (lc, lk, lo, ls)) and ls.primes * batch * n == ks.scratch_words(batch)
    arena = arena_for(dev, n, (lc, chat), (lk, key), (lo, None), (ls, None))
    ks.apply(arena.address(lc.offset), arena.address(lk.offset), arena.address(lo.offset), arena.address(ls.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lc, chat), (lk, key), (lo, None), (ls, None)], img), "a word outside out and the scratch changed"
    assert np.array_equal(arena.frames(lo, img), want)
    ks.close()
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
def test_create_rules(agx, orc, dev):
    n = 64
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    K = plan.keyswitch
    for shape in ((0, 4, 2, 2), (4, 4, 0, 2), (4, 4, 2, 0), (4, 4, 2, 17), (4, 3, 2, 2), (4, 0, 2, 2), (4, 5, 2, 2), (4, 6, 1, 2), (6, 6, 1, 2), (4, 7, 1, 2),
                  (4, 4, 17, 2), (7, 7, 1, 1), (4, 0xffffffff, 2, 2), (4, 4, 0xffffffff, 2)):
        assert status_of(agx, K, *shape) == 5, shape
    for shape in SHAPES + ((1, 5, 1, 16), (5, 5, 1, 3), (2, 3, 3, 1)):
        ks = K(*shape)
        assert ks.info()[:4] == shape and ks.info()[4] == len(digits_of(shape))
        assert status_of(agx, ks.scratch_words, 1 << 55) == 5 and status_of(agx, ks.scratch_words, (1 << 64) - 1) == 5      # reported, not wrapped
        assert ks.scratch_words(0) == 0
        ks.close()
    plan.close()
    many, _ = plan_for_moduli(agx, orc, n, tuple(agx.find_primes(60, n, 19)))
    assert status_of(agx, many.keyswitch, 17, 17, 2, 1) == 5      # seventeen digits
    ks = many.keyswitch(16, 17, 2, 1)                             # sixteen
    assert ks.info()[4] == 16
    ks.close()
    many.close()
    twice, _ = plan_for_moduli(agx, orc, n, (moduli[0], moduli[1], moduli[0], moduli[2]))
    assert status_of(agx, twice.keyswitch, 2, 2, 1, 1) == 3      # q_2 == q_0 among the active primes
    assert status_of(agx, twice.keyswitch, 3, 3, 1, 3) == 3
    ks = twice.keyswitch(2, 3, 1, 1)                             # the equal modulus is not active at this level
    ks.close()
    twice.close()


@pytest.mark.parametrize("n,shape", [(64, TOP), (4096, LOWER)])
def test_rejected_applies_write_nothing(agx, orc, dev, n, shape):
    batch = 2
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    q_count, A, D = shape[0], shape[0] + shape[2], len(digits_of(shape))
    chat, key, _, _, want = keyswitch_case(orc, n, tuple(moduli), shape, batch, 3 * n)
    sizes = [chat.size, key.size, 2 * chat.size, ks.scratch_words(batch)]
    lc = Layout(n, q_count, batch, offset=0)
    lk = Layout(n, D * 2 * A, 1, offset=lc.span() + 2 * n)
    lo = Layout(n, 2 * q_count, batch, offset=lk.span() + 2 * n)
    ls = Layout(n, sizes[3] // (batch * n), batch, offset=lo.span() + 2 * n)
    arena = arena_for(dev, n, (lc, chat), (lk, key), (lo, None), (ls, None))
    before = arena.image()
    ptrs = [arena.address(l.offset) for l in (lc, lk, lo, ls)]
    st, w = dev.stream, 8
    for k in range(4):      # NULL pointers
        args = list(ptrs)
        args[k] = 0
        assert status_of(agx, ks.apply, *args, batch, st) == 1
    for k in range(4):      # uint64_t data
        args = list(ptrs)
        args[k] += 4
        assert status_of(agx, ks.apply, *args, batch, st) == 5
    assert status_of(agx, ks.apply, *ptrs, 1 << 40, st) == 5                 # a batch past the grid limit
    assert status_of(agx, ks.apply, *ptrs, (1 << 31) - 1, st) == 5          # A batch workgroups past 2^31 - 1
    assert status_of(agx, ks.apply, *ptrs, (1 << 64) - 1, st) == 5
    for i in range(4):      # any two of the four touching: equal bases, one's first word on the other's last, and the other way round
        for j in range(4):
            if i == j:
                continue
            for at in (ptrs[i], ptrs[i] + w * (sizes[i] - 1), ptrs[i] - w * (sizes[j] - 1)):
                args = list(ptrs)
                args[j] = at
                assert status_of(agx, ks.apply, *args, batch, st) == 5, (i, j, at - ptrs[i])
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    no_inverse = fwd_only.keyswitch(*shape)
    assert status_of(agx, no_inverse.apply, *ptrs, batch, st) == 9
    assert status_of(agx, no_inverse.apply, ptrs[0], ptrs[1], ptrs[0], ptrs[3], batch, st) == 5      # the overlap rule comes first
    no_inverse.close()
    fwd_only.close()
    ks.apply(*ptrs, 0, st)      # empty batch: nothing launched
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # ranges that meet end to end are accepted: chat | keyhat | out | scratch back to back
    offs = [0, sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2]]
    packed = arena_for(dev, n, (lc.at(offs[0]), chat), (lk.at(offs[1]), key), (lo.at(offs[2]), None), (ls.at(offs[3]), None))
    ks.apply(*[packed.address(o) for o in offs], batch, st)
    assert np.array_equal(packed.frames(lo.at(offs[2])), want)
    ks.close()
    plan.close()


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def _expected_launches(agx, plan, shape, variant):
    """the sum include/agx_ntt.h states, from the info calls of the parts: the inverse on Q + every ModUp basis' launches_ntt_form + 1 + 2 ModDown
    calls.  The inverse has no info call: it is one launch, two under AGX_VARIANT_LDS_RADIX2 at n = 32768 (as agx_ntt_basis_mod_down documents)"""
    q_count, p_first, p_count, alpha = shape
    total = 2 if (variant == agx.VARIANT_LDS_RADIX2 and plan.n == 32768) else 1
    for first, count in digits_of(shape):
        targets = [(0, q_count + p_count)] if p_first == q_count else [(0, q_count), (p_first, p_count)]
        for df, dc in targets:
            b = plan.basis(first, count, df, dc)
            total += b.info()[4]
            b.close()
    down = plan.basis(p_first, p_count, 0, q_count)
    total += 1 + 2 * down.mod_down_launches()
    down.close()
    return total


def test_launch_counts_are_the_sum_of_the_parts(agx, orc, dev):
    for n, bits in [(64, 60), (1024, 60), (4096, 60), (32768, 60), (4096, 30)]:
        plan, _ = plan_for_moduli(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 6))
        for shape in SHAPES:
            ks = plan.keyswitch(*shape)
            seen = []
            for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_REGBLOCK, agx.VARIANT_AUTO):
                plan.set_variant(variant)
                assert ks.info()[5] == _expected_launches(agx, plan, shape, variant), (n, bits, shape, variant)
                seen.append(ks.info()[5])
            assert seen[0] == seen[3]
            ks.close()
        plan.close()


@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
@pytest.mark.parametrize("n", [1024, 4096])
def test_every_route_gives_the_same_words(agx, orc, dev, n, shape):
    """one handle, the plan switched AUTO -> LDS_RADIX2 -> REGBLOCK -> AUTO between its calls"""
    batch = 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, lchat, lkey, want = keyswitch_case(orc, n, tuple(moduli), shape, batch, n * 7 + batch + shape[0])
    ks = plan.keyswitch(*shape)
    for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_REGBLOCK, agx.VARIANT_AUTO):
        plan.set_variant(variant)
        assert ks.info()[5] == _expected_launches(agx, plan, shape, variant)
        assert np.array_equal(run_keyswitch(dev, ks, lchat, lkey, batch), want), ("variant", variant)
    ks.close()
    plan.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(64, TOP), (4096, LOWER)])
def test_apply_is_graph_capturable(agx, orc, dev, n, shape):
    """one apply captured on a side stream (one stream, no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    batch = 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    cases = [keyswitch_case(orc, n, tuple(moduli), shape, batch, n * 7 + batch + shape[0]), keyswitch_case(orc, n, tuple(moduli), shape, batch, n + 99)]
    d_chat, d_key = dev.to_device(cases[0][2]), dev.to_device(cases[0][3])
    d_out, d_s = dev.empty(2 * cases[0][0].size), dev.empty(ks.scratch_words(batch))

    def call(s):
        ks.apply(d_chat.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, s)

    graph = capture(dev, call, call)
    for _, _, lchat, lkey, want in cases[::-1]:
        d_chat.copy_(torch.from_numpy(lchat.view(np.int64).copy()))
        d_key.copy_(torch.from_numpy(lkey.view(np.int64).copy()))
        d_out.zero_()
        graph.replay()
        dev.sync()
        assert np.array_equal(dev.to_host(d_out), want), "replay"
    ks.close()
    plan.close()
