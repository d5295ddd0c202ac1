"""The key switch in two halves on the device: agx_ntt_keyswitch_decompose (steps 1 and 2: done once per ciphertext) and
agx_ntt_keyswitch_apply_decomposed (steps 3 and 4 with every digit read through pi_g: done once per rotation).

The reference is rns_ref.decompose_ref and rns_ref.apply_decomposed_ref: the four-step Python-integer reference of the one call cut in two, with the
NTT-form digits indexed by gpu_util.ntt_pi(n, g).  Every comparison is word for word."""
import functools

import numpy as np
import pytest

from gpu_util import Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, status_of
from rns_cases import FIVE, FIVE_IDS, LOWER, SHAPE_IDS, SHAPES, TOP, keyswitch_case, run_keyswitch
from rns_ref import active_of, apply_decomposed_ref, decompose_ref, digits_of, rotation_bound, rotation_deviation, rotation_key_case, spread

pytestmark = pytest.mark.gpu


def elements(n):
    return (1, 5, 2 * n - 1, 3)


def sizes_of(shape, n, batch):
    """(chat, key, out, ext, decompose scratch, apply scratch) in words, from the header's formulas"""
    q_count, A, D = shape[0], shape[0] + shape[2], len(digits_of(shape))
    slab = batch * n
    return q_count * slab, D * 2 * A * n, 2 * q_count * slab, D * A * slab, q_count * slab, 2 * A * slab


@functools.lru_cache(maxsize=None)
def _ext(orc, n, moduli, shape, batch, seed):
    """the words decompose must write for keyswitch_case's chat (reduced and spread alike), flat, once per case (read-only)"""
    ext = decompose_ref(orc, n, moduli, shape, keyswitch_case(orc, n, moduli, shape, batch, seed)[0]).reshape(-1)
    ext.setflags(write=False)
    return ext


@functools.lru_cache(maxsize=None)
def _keys(orc, n, moduli, shape, batch, seed, g):
    """(key reduced, key spread over [0,4q), the expected out) for element g, flat: a key of its own per element; g = 1 takes keyswitch_case's key, whose
    expected words are keyswitch_ref's (the one call's)"""
    case = keyswitch_case(orc, n, moduli, shape, batch, seed)
    if g == 1:
        return case[1], case[3], case[4]
    active = active_of(moduli, shape)
    rng = np.random.default_rng(seed * 131 + g)
    key = np.stack([rng.integers(0, int(q), size=(len(digits_of(shape)), 2, n), dtype=np.uint64) for q in active], axis=2)
    lkey = spread(rng, key, active, axis=2)
    want = apply_decomposed_ref(orc, n, moduli, shape, _ext(orc, n, moduli, shape, batch, seed), key, batch, g)
    out = (key.reshape(-1), lkey.reshape(-1), want.reshape(-1))
    for w in out:
        w.setflags(write=False)
    return out


def _decompose(dev, ks, chat, batch):
    """into a canary-filled ext with a scratch of exactly the reported size; returns the device tensor of ext and checks chat unchanged"""
    ext_words, scratch_words, _ = ks.hoisted_words(batch)
    d_chat, d_ext, d_s = dev.to_device(chat), dev.to_device(canary(0, ext_words)), dev.empty(scratch_words)
    ks.decompose(d_chat.data_ptr(), d_ext.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    dev.sync()
    assert np.array_equal(dev.to_host(d_chat), chat), "chat changed"
    return d_ext


def _apply(dev, ks, d_ext, key, batch, g, out_words):
    _, _, scratch_words = ks.hoisted_words(batch)
    d_key, d_out, d_s = dev.to_device(key), dev.to_device(canary(0, out_words)), dev.empty(scratch_words)
    ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, g, dev.stream)
    got = dev.to_host(d_out)
    assert np.array_equal(dev.to_host(d_key), key), "the key changed"
    return got


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


# ---- decompose ------------------------------------------------------------------------------------------------------------------------
def _check_decompose(orc, dev, plan, n, moduli, shape, batch, seed):
    chat, _, lchat, _, _ = keyswitch_case(orc, n, tuple(moduli), shape, batch, seed)
    want = _ext(orc, n, tuple(moduli), shape, batch, seed)
    ks = plan.keyswitch(*shape)
    assert ks.hoisted_words(batch) == sizes_of(shape, n, batch)[3:]
    assert sum(ks.hoisted_words(batch)) == ks.scratch_words(batch)
    for name, words in (("reduced", chat), ("spread", lchat)):
        got = dev.to_host(_decompose(dev, ks, words, batch))
        assert np.array_equal(got, want), (n, shape, batch, name, "first differing words", _first_bad(got, want))
    ks.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])
def test_decompose_writes_the_reference_digits(agx, orc, dev, n, batch, shape):
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_decompose(orc, dev, plan, n, moduli, shape, batch, n * 7 + batch + shape[0])
    plan.close()


@pytest.mark.parametrize("n,widths", [(64, [30] * 6), (4096, [30] * 6), (1024, [60, 30, 61, 30, 60, 60])], ids=["30-bit-64", "30-bit-4096", "mixed-1024"])
def test_decompose_other_moduli(agx, orc, dev, n, widths):
    moduli = moduli_for(orc.find_prime, n, widths)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_decompose(orc, dev, plan, n, moduli, TOP, 5, n + widths[1])
    plan.close()


# ---- apply_decomposed -------------------------------------------------------------------------------------------------------------------
def _check_apply(agx, orc, dev, plan, n, moduli, shape, batch, seed):
    """one decomposition, every element with a key of its own against hoisted_ref, reduced and spread keys; ext unchanged afterwards; g = 1 is the
    one call word for word, on the device too"""
    moduli = tuple(moduli)
    _, _, lchat, _, _ = keyswitch_case(orc, n, moduli, shape, batch, seed)
    ext = _ext(orc, n, moduli, shape, batch, seed)
    ks = plan.keyswitch(*shape)
    d_ext = _decompose(dev, ks, lchat, batch)
    out_words = sizes_of(shape, n, batch)[2]
    for g in elements(n):
        key, lkey, want = _keys(orc, n, moduli, shape, batch, seed, g)
        for name, k_words in (("reduced", key), ("spread", lkey)):
            got = _apply(dev, ks, d_ext, k_words, batch, g, out_words)
            assert np.array_equal(got, want), (n, shape, batch, g, name, "first differing words", _first_bad(got, want))
        if g == 1:
            assert np.array_equal(run_keyswitch(dev, ks, lchat, lkey, batch), want), "apply differs from the two halves at g = 1"
    assert np.array_equal(dev.to_host(d_ext), ext), "ext changed"
    ks.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n,batch", [(8, 5), (64, 5), (1024, 3), (4096, 2)])
def test_apply_decomposed_against_the_reference(agx, orc, dev, n, batch, shape):
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_apply(agx, orc, dev, plan, n, moduli, shape, batch, n * 7 + batch + shape[0])
    plan.close()


@pytest.mark.parametrize("n,widths", [(64, [30] * 6), (1024, [60, 30, 61, 30, 60, 60])], ids=["30-bit-64", "mixed-1024"])
def test_apply_decomposed_other_moduli(agx, orc, dev, n, widths):
    moduli = moduli_for(orc.find_prime, n, widths)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_apply(agx, orc, dev, plan, n, moduli, TOP, 5, n + widths[1])
    plan.close()


# ---- it switches rotated keys ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [5, 127])
@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_it_switches_rotated_keys(agx, orc, dev, shape, g):
    """the device's outputs with the noise-free rotation key of rns_ref.rotation_key_case: out_0 + out_1 s - sigma_g(c) sigma_g(s), CRT-centred
    modulo Q, is at most p_count (1 + ||s||_1) at every coefficient -- a condition, not a measurement"""
    n, batch = 64, 2
    assert g in (5, 2 * n - 1)
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    chat, key, s, shat = rotation_key_case(orc, n, moduli, shape, g, batch, 1000 + sum(shape) + g)
    ks = plan.keyswitch(*shape)
    d_ext = _decompose(dev, ks, chat.reshape(-1), batch)
    out = _apply(dev, ks, d_ext, key.reshape(-1), batch, g, 2 * chat.size)
    ks.close()
    plan.close()
    worst, bound = rotation_deviation(orc, n, moduli, shape, g, batch, chat, shat, out), rotation_bound(shape, s)
    print(f"shape {shape}, g = {g}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, g, worst, bound)


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def test_launch_counts_of_the_halves_sum_to_the_one_call(agx, orc, dev):
    for n, bits in [(64, 60), (1024, 60), (4096, 60), (32768, 60), (4096, 30)]:
        plan, _ = plan_for_moduli(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 6))
        down = plan.basis(4, 2, 0, 4)
        for shape in SHAPES:
            ks = plan.keyswitch(*shape)
            for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_REGBLOCK, agx.VARIANT_AUTO):
                plan.set_variant(variant)
                first, second = ks.hoisted_info()
                assert first >= 1 + len(digits_of(shape)) and first + second == ks.info()[5], (n, bits, shape, variant)
                if shape[1:3] == (4, 2):      # mod_down_launches depends on the plan alone: any ModDown basis of the plan tells
                    assert second == 1 + 2 * down.mod_down_launches(), (n, bits, shape, variant)
            ks.close()
        down.close()
        plan.close()


@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
@pytest.mark.parametrize("n", [1024, 4096])
def test_every_route_gives_the_same_words(agx, orc, dev, n, shape):
    """one handle, the plan switched AUTO -> LDS_RADIX2 -> REGBLOCK -> AUTO between its calls"""
    batch, g = 5, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    seed = n * 7 + batch + shape[0]
    _, _, lchat, _, _ = keyswitch_case(orc, n, tuple(moduli), shape, batch, seed)
    ext = _ext(orc, n, tuple(moduli), shape, batch, seed)
    _, lkey, want = _keys(orc, n, tuple(moduli), shape, batch, seed, g)
    ks = plan.keyswitch(*shape)
    for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_REGBLOCK, agx.VARIANT_AUTO):
        plan.set_variant(variant)
        assert sum(ks.hoisted_info()) == ks.info()[5]
        d_ext = _decompose(dev, ks, lchat, batch)
        assert np.array_equal(dev.to_host(d_ext), ext), ("decompose, variant", variant)
        assert np.array_equal(_apply(dev, ks, d_ext, lkey, batch, g, want.size), want), ("apply_decomposed, variant", variant)
    ks.close()
    plan.close()


# ---- placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
@pytest.mark.parametrize("n,odd", [(64, True), (4096, True), (4096, False)])
def test_guard_bands_and_odd_placement(agx, orc, dev, n, odd, shape):
    """the six buffers of the two calls in one arena, each of exactly the size hoisted_words reports, at odd words (every base 8 mod 16) or at even
    ones: the right words, chat, ext (after apply_decomposed) and keyhat unchanged, and every word outside ext, out and the two scratches as it was"""
    batch, g = 3, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    seed = n + 23
    _, _, chat, _, _ = keyswitch_case(orc, n, tuple(moduli), shape, batch, seed)
    ext = _ext(orc, n, tuple(moduli), shape, batch, seed)
    _, key, want = _keys(orc, n, tuple(moduli), shape, batch, seed, g)
    words = ks.hoisted_words(batch)
    assert words == sizes_of(shape, n, batch)[3:]
    place = lambda off: off + (off % 2 != (1 if odd else 0))      # noqa: E731
    slab = batch * n
    lc = Layout(n, chat.size // slab, batch, offset=place(0))
    lk = Layout(n, key.size // n, 1, offset=place(lc.span() + 5))
    lo = Layout(n, want.size // slab, batch, offset=place(lk.span() + 5))
    le = Layout(n, words[0] // slab, batch, offset=place(lo.span() + 5))
    ld = Layout(n, words[1] // slab, batch, offset=place(le.span() + 5))
    la = Layout(n, words[2] // slab, batch, offset=place(ld.span() + 5))
    assert all(l.offset % 2 == (1 if odd else 0) for l in (lc, lk, lo, le, ld, la))
    assert (le.primes * slab, ld.primes * slab, la.primes * slab) == words
    arena = arena_for(dev, n, (lc, chat), (lk, key), (lo, None), (le, None), (ld, None), (la, None))
    ks.decompose(arena.address(lc.offset), arena.address(le.offset), arena.address(ld.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lc, chat), (lk, key), (le, None), (ld, None)], img), "decompose changed a word outside ext and its scratch"
    assert np.array_equal(arena.frames(le, img), ext)
    ks.apply_decomposed(arena.address(le.offset), arena.address(lk.offset), arena.address(lo.offset), arena.address(la.offset), batch, g, dev.stream)
    img = arena.image()
    assert not arena.faults([(lc, chat), (lk, key), (le, ext), (lo, None), (ld, None), (la, None)], img), "apply_decomposed changed a word outside out and its scratch"
    assert np.array_equal(arena.frames(lo, img), want)
    ks.close()
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(64, TOP), (4096, LOWER)])
def test_rejected_calls_write_nothing(agx, orc, dev, n, shape):
    batch, g = 2, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    seed = 3 * n
    chat, _, _, _, _ = keyswitch_case(orc, n, tuple(moduli), shape, batch, seed)
    ext = _ext(orc, n, tuple(moduli), shape, batch, seed)
    key, _, want = _keys(orc, n, tuple(moduli), shape, batch, seed, g)
    chat_w, key_w, out_w, ext_w, ds_w, as_w = sizes_of(shape, n, batch)
    assert ks.hoisted_words(batch) == (ext_w, ds_w, as_w) and ks.hoisted_words(0) == (0, 0, 0)
    assert status_of(agx, ks.hoisted_words, 1 << 55) == 5 and status_of(agx, ks.hoisted_words, (1 << 64) - 1) == 5      # reported, not wrapped
    slab = batch * n
    lc = Layout(n, chat_w // slab, batch, offset=0)
    lk = Layout(n, key_w // n, 1, offset=lc.span() + 2 * n)
    lo = Layout(n, out_w // slab, batch, offset=lk.span() + 2 * n)
    le = Layout(n, ext_w // slab, batch, offset=lo.span() + 2 * n)
    ld = Layout(n, ds_w // slab, batch, offset=le.span() + 2 * n)
    la = Layout(n, as_w // slab, batch, offset=ld.span() + 2 * n)
    arena = arena_for(dev, n, (lc, chat), (lk, key), (lo, None), (le, ext), (ld, None), (la, None))
    before = arena.image()
    pc, pk, po, pe, pd, pa = (arena.address(l.offset) for l in (lc, lk, lo, le, ld, la))
    st, w = dev.stream, 8
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    no_inverse = fwd_only.keyswitch(*shape)
    # (call, its pointers, their sizes, the arguments behind the pointers)
    calls = [(ks.decompose, no_inverse.decompose, [pc, pe, pd], [chat_w, ext_w, ds_w], lambda b: (b, st)),
             (ks.apply_decomposed, no_inverse.apply_decomposed, [pe, pk, po, pa], [ext_w, key_w, out_w, as_w], lambda b: (b, g, st))]
    for call, call_no_inverse, ptrs, sizes, tail in calls:
        count = len(ptrs)
        for k in range(count):      # NULL pointers
            args = list(ptrs)
            args[k] = 0
            assert status_of(agx, call, *args, *tail(batch)) == 1
        for k in range(count):      # uint64_t data: an odd-byte pointer and one at 4 bytes
            for off in (1, 4):
                args = list(ptrs)
                args[k] += off
                assert status_of(agx, call, *args, *tail(batch)) == 5
        assert status_of(agx, call, *ptrs, *tail(1 << 40)) == 5                 # a batch past the grid limit
        assert status_of(agx, call, *ptrs, *tail((1 << 31) - 1)) == 5          # A batch workgroups past 2^31 - 1
        assert status_of(agx, call, *ptrs, *tail((1 << 64) - 1)) == 5
        for i in range(count):      # any two touching: equal bases, one's first word on the other's last, and the other way round
            for j in range(count):
                if i == j:
                    continue
                for at in (ptrs[i], ptrs[i] + w * (sizes[i] - 1), ptrs[i] - w * (sizes[j] - 1)):
                    args = list(ptrs)
                    args[j] = at
                    assert status_of(agx, call, *args, *tail(batch)) == 5, (call.__name__, i, j, at - ptrs[i])
        assert status_of(agx, call_no_inverse, *ptrs, *tail(batch)) == 9
        args = list(ptrs)
        args[1] = args[0]
        assert status_of(agx, call_no_inverse, *args, *tail(batch)) == 5      # the overlap rule comes first
        call(*ptrs, *tail(0))      # empty batch: nothing launched
    A = ks.apply_decomposed
    for elt in (0, 2, 2 * n - 2, 2 * n, 2 * n + 1, 0xffffffff):      # the Galois element: even, 0, 2n and beyond
        assert status_of(agx, A, pe, pk, po, pa, batch, elt, st) == 5, elt
    assert status_of(agx, A, 0, pk, po, pa, batch, 2, st) == 1                              # behind the NULL rule
    assert status_of(agx, no_inverse.apply_decomposed, pe, pk, po, pa, batch, 2, st) == 5      # in front of the missing inverse
    assert status_of(agx, A, pe, pk, po, pa, 0, 2, st) == 5                                 # and of the empty batch
    no_inverse.close()
    fwd_only.close()
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # ranges that meet end to end are accepted: chat | ext | scratch and ext | keyhat | out | scratch back to back
    offs = [0, chat_w, chat_w + ext_w]
    packed = arena_for(dev, n, (lc.at(offs[0]), chat), (le.at(offs[1]), None), (ld.at(offs[2]), None))
    ks.decompose(*[packed.address(o) for o in offs], batch, st)
    assert np.array_equal(packed.frames(le.at(offs[1])), ext)
    offs = [0, ext_w, ext_w + key_w, ext_w + key_w + out_w]
    packed = arena_for(dev, n, (le.at(offs[0]), ext), (lk.at(offs[1]), key), (lo.at(offs[2]), None), (la.at(offs[3]), None))
    ks.apply_decomposed(*[packed.address(o) for o in offs], batch, g, st)
    assert np.array_equal(packed.frames(lo.at(offs[2])), want)
    ks.close()
    plan.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(64, TOP), (4096, LOWER)])
def test_the_halves_are_graph_capturable(agx, orc, dev, n, shape):
    """one decompose and three apply_decomposed with three elements and three keys in ONE graph, captured on a side stream (one stream, no parallel
    branches), replayed on fresh inputs"""
    torch = dev.torch
    batch = 5
    moduli = tuple(moduli_for(orc.find_prime, n, [60] * 6))
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    gs = (5, 2 * n - 1, 3)
    seeds = (n * 7 + batch + shape[0], n + 99)
    chat_w, key_w, out_w, ext_w, ds_w, as_w = sizes_of(shape, n, batch)
    d_chat, d_ext, d_ds, d_as = dev.empty(chat_w), dev.empty(ext_w), dev.empty(ds_w), dev.empty(as_w)
    d_keys, d_outs = [dev.empty(key_w) for _ in gs], [dev.empty(out_w) for _ in gs]

    def load(seed):
        d_chat.copy_(torch.from_numpy(keyswitch_case(orc, n, moduli, shape, batch, seed)[2].view(np.int64).copy()))
        for d_key, d_out, g in zip(d_keys, d_outs, gs):
            d_key.copy_(torch.from_numpy(_keys(orc, n, moduli, shape, batch, seed, g)[1].view(np.int64).copy()))
            d_out.zero_()

    def call(s):
        ks.decompose(d_chat.data_ptr(), d_ext.data_ptr(), d_ds.data_ptr(), batch, s)
        for d_key, d_out, g in zip(d_keys, d_outs, gs):      # one scratch serves the three: they run one behind the other on the one stream
            ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_as.data_ptr(), batch, g, s)

    load(seeds[0])
    graph = capture(dev, call, call)
    for seed in seeds[::-1]:
        load(seed)
        graph.replay()
        dev.sync()
        for d_out, g in zip(d_outs, gs):
            assert np.array_equal(dev.to_host(d_out), _keys(orc, n, moduli, shape, batch, seed, g)[2]), ("replay", seed, g)
    ks.close()
    plan.close()
