"""agx_ntt_basis_extend on the device: fast RNS base conversion from the source primes of a basis to its target primes, in coefficient
form and fused with the targets' forward transform.

The expected words come from Python integers, from the definition (rns_ref.convert): y_i = (x_i mod q_i) (D_i^-1 mod q_i) mod q_i, V = sum_i y_i D_i
as an integer, out_j = V mod q_j; the NTT-form expectation is the CPU oracle's forward of those words.  Every comparison is word for word."""
import functools

import numpy as np
import pytest

from gpu_util import RESCALE_IDS, Layout, arena_for, assert_equals_chunked_calls, canary, capture, judged_frames, moduli_for, plan_for_moduli, registry_entries, status_of
from rns_ref import convert, device_residues, oracle_forward_set, product, residues, special_values, spread

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
FORMS = (COEFF, NTT)
# (source first, source count, target first, target count) on a plan of five primes
MODUP, MODDOWN, SINGLE = (1, 2, 0, 5), (3, 2, 0, 3), (2, 1, 0, 5)
SHAPES = (MODUP, MODDOWN, SINGLE)
# the product library's registry entries that carry launch_extend: exactly the ones that carry launch_rescale, one frame per workgroup each
EXTEND_IDS = RESCALE_IDS


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(rng, src, batch, n):
    """[S][batch][n] reduced residues.  Frame 0 opens with the special values and is random behind them; with five frames, frame 1 is all
    zero, frame 2 holds q_i - 1 everywhere (X = D - 1), frame 3 repeats the special values to its end, frame 4 is random"""
    x = np.stack([rng.integers(0, int(q), size=batch * n, dtype=np.uint64) for q in src]).reshape(len(src), batch, n)
    special = residues(special_values(src), src)
    k = min(n, special.shape[1])
    x[:, 0, :k] = special[:, :k]
    if batch >= 5:
        x[:, 1, :] = 0
        x[:, 2, :] = np.array([int(q) - 1 for q in src], dtype=np.uint64)[:, None]
        x[:, 3, :] = np.tile(special, (1, n // special.shape[1] + 1))[:, :n]
    return x.reshape(len(src), -1)


@functools.lru_cache(maxsize=None)
def _case(orc, n, moduli, shape, batch, seed):
    """(x reduced, x spread over [0,4q), {form: expected words [T][batch][n]}), computed once per case (read-only)"""
    sf, S, df, T = shape
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    rng = np.random.default_rng(seed)
    x = make_inputs(rng, src, batch, n)
    lazy = spread(rng, x, src)
    coeff = convert(x, src, dst)
    want = {COEFF: coeff.reshape(-1), NTT: oracle_forward_set(orc, n, dst, coeff).reshape(-1)}
    for a in (x, lazy, *want.values()):
        a.setflags(write=False)
    return x.reshape(-1), lazy.reshape(-1), want


def _extend(dev, basis, x, out_words, batch, form):
    d_x = dev.to_device(x)
    d_out = dev.to_device(canary(0, out_words))
    basis.extend(d_x.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
    return dev.to_host(d_out)


def _check(agx, orc, dev, plan, n, moduli, shape, batch, seed, what, forms=FORMS):
    """both forms, from reduced inputs and from inputs spread over [0, 4q)"""
    x, lazy, want = _case(orc, n, moduli, shape, batch, seed)
    basis = plan.basis(*shape)
    for form in forms:
        for name, words in (("reduced", x), ("spread", lazy)):
            got = _extend(dev, basis, words, shape[3] * batch * n, batch, form)
            bad = np.flatnonzero(got != want[form])
            assert bad.size == 0, (what, "form", form, name, "first differing words", bad[:4].tolist(), got[bad[:4]].tolist(), want[form][bad[:4]].tolist())
    basis.close()


# ---- parity -------------------------------------------------------------------------------------------------------------------------
SIZES = [8, 64, 512, 1024, 4096, 16384, 32768]


@pytest.mark.parametrize("shape", SHAPES, ids=["modup", "moddown", "single"])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", SIZES)
def test_parity_60_bit(agx, orc, dev, n, batch, shape):
    moduli = moduli_for(orc.find_prime, n, [60] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(agx, orc, dev, plan, n, moduli, shape, batch, n * 7 + batch + shape[0], (n, batch, shape))
    plan.close()


@pytest.mark.parametrize("shape", SHAPES, ids=["modup", "moddown", "single"])
@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_parity_30_bit(agx, orc, dev, n, shape):
    """plans whose moduli are all below 2^31: the generic route through the 32-bit forward kernels"""
    moduli = moduli_for(orc.find_prime, n, [30] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(agx, orc, dev, plan, n, moduli, shape, 5, n + 30 + shape[0], (n, "30-bit", shape))
    plan.close()


@pytest.mark.parametrize("shape", SHAPES, ids=["modup", "moddown", "single"])
def test_parity_mixed_widths(agx, orc, dev, shape):
    """[60, 30, 61, 30, 60]: 30-bit residues lifted under 60-bit targets and the other way round, a 61-bit modulus (the fast-arithmetic kernels)"""
    n = 1024
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 30, 60])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(agx, orc, dev, plan, n, moduli, shape, 5, 1024 + shape[0], ("mixed", shape))
    plan.close()


def test_sixteen_sources_of_62_bits(agx, orc, dev):
    """the accumulation edge: S = 16 sources of the widest class into all 17 primes; one frame with every residue at q_i - 1, and one
    whose y_i are all q_i - 1 (the largest sum) in its first half and random behind"""
    n, batch = 1024, 1
    moduli = tuple(agx.find_primes(62, n, 17))
    assert all(q > 1 << 61 for q in moduli)
    src = moduli[:16]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(0, 16, 0, 17)
    assert basis.info()[:4] == (0, 16, 0, 17)
    rng = np.random.default_rng(62)
    top = np.tile(np.array([q - 1 for q in src], dtype=np.uint64)[:, None], (1, n))
    D = product(src)
    largest = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in src])
    largest[:, :n // 2] = np.array([(q - 1) * (D // q) % q for q in src], dtype=np.uint64)[:, None]
    for name, x in (("every residue q_i - 1", top), ("every y_i = q_i - 1", largest)):
        coeff = convert(x, src, moduli)
        want = {COEFF: coeff.reshape(-1), NTT: oracle_forward_set(orc, n, moduli, coeff).reshape(-1)}
        for form in FORMS:
            for words in (x, spread(rng, x, src)):
                assert np.array_equal(_extend(dev, basis, words.reshape(-1), 17 * batch * n, batch, form), want[form]), (name, "form", form)
    basis.close()
    plan.close()


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def _fused_expected(n, bits, S):
    """the route shipped (profiles/r08_basis_extend.md): the fused kernel serves 64-bit plans of n >= 1024 for one source prime, and for two
    except at n = 4096 and 16384, where it measured behind the unfused pair; three or more sources take the pair"""
    return n >= 1024 and bits > 31 and (S == 1 or (S == 2 and n not in (4096, 16384)))


def test_launch_counts_follow_the_route(agx, orc, dev):
    """one launch to NTT form where the fused kernel serves under AGX_VARIANT_AUTO; the coefficient-form launch and the plan's forward
    elsewhere -- two launches, three where the radix-2 forward itself takes two (n = 32768)"""
    for n, bits in [(1024, 60), (2048, 61), (4096, 60), (8192, 62), (16384, 60), (32768, 60), (8, 60), (64, 60), (512, 60), (64, 30), (1024, 30), (4096, 30)]:
        plan, _ = plan_for_moduli(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 4))
        for S in (1, 2, 3, 4):
            want = 1 if _fused_expected(n, bits, S) else 2
            basis = plan.basis(0, S, 0, 4)
            assert basis.info() == (0, S, 0, 4, want), (n, bits, S)
            if want == 1:
                plan.set_variant(agx.VARIANT_LDS_RADIX2)      # computed at the info call: the basis follows the plan's variant
                assert basis.info()[4] == (2 if n <= 16384 else 3), (n, bits, S, "radix-2")
                plan.set_variant(agx.VARIANT_REGBLOCK)
                assert basis.info()[4] == 1, (n, bits, S, "regblock")
                plan.set_variant(agx.VARIANT_LDS_RADIX2)
                plan.set_variant(agx.VARIANT_AUTO)
                assert basis.info()[4] == 1, (n, bits, S, "auto again")
            basis.close()
        plan.close()


@pytest.mark.parametrize("n,shape", [(1024, MODUP), (4096, SINGLE), (16384, SINGLE), (32768, MODUP)])
def test_radix2_result_equals_the_fused_result(agx, orc, dev, n, shape):
    """one basis, the plan switched between its calls; shapes the fused kernel serves at each size"""
    batch = 5
    moduli = moduli_for(orc.find_prime, n, [60] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    x, lazy, want = _case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0])
    basis = plan.basis(*shape)
    assert basis.info()[4] == 1
    fused = [_extend(dev, basis, w, 5 * batch * n, batch, NTT) for w in (x, lazy)]
    plan.set_variant(agx.VARIANT_LDS_RADIX2)
    assert basis.info()[4] == (2 if n <= 16384 else 3)
    generic = [_extend(dev, basis, w, 5 * batch * n, batch, NTT) for w in (x, lazy)]
    for a, b in zip(fused, generic):
        assert np.array_equal(a, b), "fused and generic routes differ"
        assert np.array_equal(b, want[NTT])
    assert np.array_equal(_extend(dev, basis, x, 5 * batch * n, batch, COEFF), want[COEFF])
    basis.close()
    plan.close()


@pytest.mark.parametrize("config,n,max_bits", registry_entries(EXTEND_IDS))
def test_every_registry_entry_at_its_own_size(agx, orc, dev, config, n, max_bits):
    """each entry selected explicitly (AGX_VARIANT_REGBLOCK_BASE + id) under the widest modulus it admits; every one of them holds one
    frame per workgroup, so batch 2 = frames per workgroup + 1"""
    batch = 2
    moduli = moduli_for(orc.find_prime, n, [max_bits] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    shapes = (SINGLE,) if n in (4096, 16384) else (SINGLE, MODUP)      # what the fused kernel serves at this size
    for shape in shapes:
        basis = plan.basis(*shape)
        assert basis.info()[4] == 1, "the entry does not carry the fused kernel"
        basis.close()
        _check(agx, orc, dev, plan, n, moduli, shape, batch, config + shape[1], ("registry id", config, shape), forms=(NTT,))
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
def test_creation_statuses(agx, orc, dev):
    n = 64
    moduli = tuple(agx.find_primes(60, n, 17))
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    B = agx.Basis
    assert status_of(agx, B, plan, 0, 0, 0, 1) == 5 and status_of(agx, B, plan, 0, 1, 0, 0) == 5          # empty ranges
    assert status_of(agx, B, plan, 17, 1, 0, 1) == 5 and status_of(agx, B, plan, 16, 2, 0, 1) == 5        # source past P
    assert status_of(agx, B, plan, 0, 1, 17, 1) == 5 and status_of(agx, B, plan, 0, 1, 1, 17) == 5        # target past P
    assert status_of(agx, B, plan, 0xFFFFFFFF, 2, 0, 1) == 5 and status_of(agx, B, plan, 0, 1, 2, 0xFFFFFFFF) == 5      # first + count wraps
    assert status_of(agx, B, plan, 0, 17, 0, 1) == 5                                                     # more than AGX_BASIS_MAX_SRC sources
    for args in ((0, 16, 0, 17), (1, 16, 0, 17), (16, 1, 0, 17), (0, 1, 16, 1)):
        b = B(plan, *args)
        assert b.info()[:4] == args
        b.close()
    plan.close()
    twice, _ = plan_for_moduli(agx, orc, n, (moduli[0], moduli[1], moduli[0]))
    assert status_of(agx, B, twice, 0, 3, 0, 3) == 3                                                      # two equal source moduli
    B(twice, 0, 2, 0, 3).close()                                                                          # ... not among these sources
    B(twice, 1, 2, 0, 3).close()
    twice.close()


@pytest.mark.parametrize("n,bits", [(64, 60), (4096, 60), (4096, 30)])
def test_rejected_calls_write_nothing(agx, orc, dev, n, bits):
    batch, shape = 2, (1, 2, 0, 3)
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [bits] * 3)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    x, _, _ = _case(orc, n, moduli, shape, batch, 3 * n + bits)
    lx = Layout(n, S, batch, offset=0)
    lo = Layout(n, T, batch, offset=lx.span() + 2 * n)
    arena = arena_for(dev, n, (lx, x), (lo, None))
    before = arena.image()
    px, po, st, w = arena.address(0), arena.address(lo.offset), dev.stream, 8
    E = basis.extend
    for form in FORMS:
        assert status_of(agx, E, 0, po, batch, form, st) == 1 and status_of(agx, E, px, 0, batch, form, st) == 1
        assert status_of(agx, E, px + 4, po, batch, form, st) == 5 and status_of(agx, E, px, po + 4, batch, form, st) == 5      # uint64_t data
        # out of place only; the output (canary words here) must stay as it was
        assert status_of(agx, E, px, px, batch, form, st) == 5                                           # d_out == d_x
        assert status_of(agx, E, px, px + w * (n // 2), batch, form, st) == 5                            # out starts inside x
        assert status_of(agx, E, px, px + w * (S * batch * n - 1), batch, form, st) == 5                 # ... on x's last word
        assert status_of(agx, E, po + w * (n // 2), po, batch, form, st) == 5                            # x starts inside out
        assert status_of(agx, E, po + w * (T * batch * n - 1), po, batch, form, st) == 5                 # ... on out's last word
        E(px, po, 0, form, st)                                                                           # empty batch: nothing launched
    assert status_of(agx, E, px, po, batch, 2, st) == 5 and status_of(agx, E, px, po, batch, -1, st) == 5      # unknown form
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # the ranges may meet end to end
    for form in FORMS:
        E(px, px + w * (S * batch * n), batch, form, st)
    dev.sync()
    basis.close()
    plan.close()


# ---- graph capture, placement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096, 8192, 16384])
def test_calls_are_graph_capturable(agx, orc, dev, n):
    """a call of each form captured one after the other on a side stream (no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    batch, shape = 5, MODUP
    T = shape[3]
    moduli = moduli_for(orc.find_prime, n, [60] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    cases = [_case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0]), _case(orc, n, moduli, shape, batch, n + 99)]
    d_x = dev.to_device(cases[0][0])
    d_out = [dev.empty(T * batch * n) for _ in FORMS]

    def both_forms(s):
        for form in FORMS:
            basis.extend(d_x.data_ptr(), d_out[form].data_ptr(), batch, form, s)

    graph = capture(dev, both_forms, both_forms)
    for x, lazy, want in cases[::-1]:
        for words in (x, lazy):
            d_x.copy_(torch.from_numpy(words.view(np.int64).copy()))
            for d in d_out:
                d.zero_()
            graph.replay()
            dev.sync()
            for form in FORMS:
                got = dev.to_host(d_out[form])
                assert np.array_equal(got, want[form]), ("replay", form)
                assert np.array_equal(got, _extend(dev, basis, words, T * batch * n, batch, form)), ("direct call", form)
    basis.close()
    plan.close()


@pytest.mark.parametrize("n,bits,batch", [(64, 60, 5), (1024, 60, 5), (4096, 60, 5), (4096, 30, 3), (16384, 62, 2), (32768, 61, 2)])
def test_odd_placement_and_guard_bands(agx, orc, dev, n, bits, batch):
    """both buffers at an odd word of one larger allocation (no frame starts on a 16-byte boundary): the right words, x unchanged, and
    every word outside d_out as it was"""
    shape = MODUP
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [bits] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    x, _, want = _case(orc, n, moduli, shape, batch, n + bits)
    lx = Layout(n, S, batch, offset=1)
    lo = Layout(n, T, batch, offset=lx.span() + 5 + (lx.span() + 5 + 1) % 2)
    assert lx.offset % 2 == 1 and lo.offset % 2 == 1
    for form in FORMS:
        arena = arena_for(dev, n, (lx, x), (lo, None))
        basis.extend(arena.address(lx.offset), arena.address(lo.offset), batch, form, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx, x), (lo, None)], img), "a word outside d_out changed"
        assert np.array_equal(arena.frames(lo, img), want[form]), ("form", form)
    basis.close()
    plan.close()


# ---- size ---------------------------------------------------------------------------------------------------------------------------
def _judge_frames(dev, basis, d_x, src, dst, batch, n, frames, orc):
    """both forms of one call each; the listed frames (of every target) against Python integers"""
    S, T = len(src), len(dst)
    xs = dev.to_host(d_x.view(S, batch, n)[:, frames].contiguous()).reshape(S, -1)
    coeff = convert(xs, src, dst)
    want = {COEFF: coeff.reshape(T, len(frames), n), NTT: oracle_forward_set(orc, n, dst, coeff).reshape(T, len(frames), n)}
    for form in FORMS:
        d_out = dev.empty(T * batch * n)
        basis.extend(d_x.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
        got = dev.to_host(d_out.view(T, batch, n)[:, frames].contiguous()).reshape(T, len(frames), n)
        for j in range(T):
            bad = [frames[f] for f in range(len(frames)) if not np.array_equal(got[j, f], want[form][j, f])]
            assert not bad, ("form", form, "target", j, "frames", bad[:8])
        del d_out


def test_generic_kernel_past_one_grid_stride_trip(agx, orc, dev):
    """n = 32, 140,000 frames: 4,480,000 coefficients per slab, more than one thread each of the element-wise kernels' largest grid (today
    16384 workgroups of 256 threads: a second step from frame 131072 on).  Nothing here depends on that figure: every word of the large call
    is compared with the same call made 1,000 frames at a time -- 125 workgroups' worth, one step of any grid that size or larger -- and
    frames across the whole range, the ends included, with Python integers.  The plan has three primes so that the second part has three
    targets."""
    torch = dev.torch
    n, batch, chunk = 32, 140000, 1000
    moduli = moduli_for(orc.find_prime, n, [60] * 3)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    # S = 1, prime 0 -> prime 1, inputs below both moduli: D = q_0, D_0 = 1, so the output is the input
    one = plan.basis(0, 1, 1, 1)
    d_x = device_residues(torch, dev, moduli[:1], batch, n, 1, bound=min(moduli[:2]))
    d_out = dev.empty(batch * n)
    d_out.fill_(-1)
    one.extend(d_x.data_ptr(), d_out.data_ptr(), batch, COEFF, dev.stream)
    dev.sync()
    assert torch.equal(d_out, d_x), "S = 1 under a larger-or-equal residue range must copy"
    one.close()
    del d_out
    # S = 2 -> three targets
    S, T = 2, 3
    two = plan.basis(0, S, 0, T)
    d_x = device_residues(torch, dev, moduli[:S], batch, n, 2)
    d_out = dev.empty(T * batch * n)
    d_out.fill_(-1)
    two.extend(d_x.data_ptr(), d_out.data_ptr(), batch, COEFF, dev.stream)
    assert_equals_chunked_calls(torch, lambda ins, outs, frames: two.extend(ins[0].data_ptr(), outs[0].data_ptr(), frames, COEFF, dev.stream),
                                [d_x.view(S, batch, n)], [d_out.view(T, batch, n)], batch, chunk)
    del d_out
    frames = judged_frames(batch, 48, extra=range(0, batch, 4999))
    _judge_frames(dev, two, d_x, moduli[:S], moduli, batch, n, frames, orc)
    two.close()
    plan.close()


@pytest.mark.parametrize("n,S", [(4096, 2), (4096, 1), (2048, 2)])
def test_ntt_form_at_1100_frames(agx, orc, dev, n, S):
    """1,100 frames, S sources -> three targets: 3,300 workgroups decoded target-fastest where the fused kernel serves (n = 4096 with one
    source, n = 2048 with two); n = 4096 with two sources is the issue's case and runs the route shipped for it, the unfused pair.  Edge
    frames and a thin sample against Python integers"""
    torch = dev.torch
    batch = 1100
    moduli = moduli_for(orc.find_prime, n, [60] * 3)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(0, S, 0, 3)
    assert basis.info()[4] == (1 if _fused_expected(n, 60, S) else 2)
    d_x = device_residues(torch, dev, moduli[:S], batch, n, 3)
    frames = judged_frames(batch, 14)
    _judge_frames(dev, basis, d_x, moduli[:S], moduli, batch, n, frames, orc)
    basis.close()
    plan.close()
