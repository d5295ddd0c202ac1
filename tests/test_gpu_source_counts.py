"""agx_ntt_basis_extend, agx_ntt_basis_mod_down_mode and agx_ntt_basis_mod_down at EVERY source count S = 1 ... 16, on each of their routes.

The coefficient-domain kernels are instantiated per source capacity 1, 2, 4, 8, 16 (with_smax, csrc/ntt_kernels.hip) with guarded, unrolled loops, and the
fused ModDown kernels (csrc/moddown_rb2_body.hpp) walk the sources at run time with a two-buffer prefetch that wraps at the last one: a sweep over S fills
every capacity partly and wholly and ends the prefetch at every parity.  The bases live on a plan of 19 primes (rns_cases.extend_shape, mod_down_shape);
one plan serves a whole sweep, and the launch counts the handles report are asserted so that the route that ran is the route meant.

The expected words come from Python integers (rns_ref.convert, moddown_modes_ref.mod_down_mode) and the CPU oracle's transforms.  Every comparison is word
for word, from reduced inputs and from inputs spread over [0, 4q), into canary-filled outputs, with the inputs checked unchanged."""
import numpy as np
import pytest

from gpu_util import RESCALE_IDS, Layout, arena_for, canary, moduli_for, plan_for_moduli, registry_entries
from moddown_modes_ref import FLOOR, ROUND
from rns_cases import MIXED_WIDTHS, SOURCE_COUNTS, SWEEP_PRIMES, extend_shape, extend_sweep_case, mod_down_shape, mod_down_sweep_case

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
BATCH = 3
T17 = 65537
SETTINGS = ((1, FLOOR), (1, ROUND), (T17, FLOOR), (T17, ROUND))      # (plaintext modulus, mode)
IN_PLACE_AT_1024 = (5, 8, 9, 16)


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


# ---- agx_ntt_basis_extend ---------------------------------------------------------------------------------------------------------------------------
def _check_extend(orc, dev, plan, n, moduli, S, launches, what):
    """both forms, from reduced and from spread inputs, into a canary-filled output; x unchanged; the launch count of the NTT form"""
    x, lazy, want = extend_sweep_case(orc, n, moduli, S, BATCH, 100 * n + S)
    basis = plan.basis(*extend_shape(S))
    assert basis.info() == extend_shape(S) + (launches,), (what, S)
    for form in (COEFF, NTT):
        for name, words in (("reduced", x), ("spread", lazy)):
            d_x, d_out = dev.to_device(words), dev.to_device(canary(0, 3 * BATCH * n))
            basis.extend(d_x.data_ptr(), d_out.data_ptr(), BATCH, form, dev.stream)
            got = dev.to_host(d_out)
            assert np.array_equal(got, want[form]), (what, "S", S, "form", form, name, "first differing words", _first_bad(got, want[form]))
            assert np.array_equal(dev.to_host(d_x), words), (what, "S", S, "x changed")
    basis.close()


@pytest.mark.parametrize("n,bits", [(64, 60), (64, 30), (1024, 60)], ids=["wave-packed-64", "32-bit-64", "auto-1024"])
def test_extend_at_every_source_count(agx, orc, dev, n, bits):
    """sources [0, S), targets [S - 1, S + 2): the first target is the last source, so its coefficient-form words are x_{S-1} mod q.  n = 64 is the
    coefficient-form launch and the plan's forward -- the wave-packed kernels, or the 32-bit ones when every modulus is below 2^31; n = 1024 under
    AGX_VARIANT_AUTO is the fused kernel at S <= 2 and the pair above"""
    moduli = moduli_for(orc.find_prime, n, [bits] * SWEEP_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for S in SOURCE_COUNTS:
        _check_extend(orc, dev, plan, n, moduli, S, 1 if n == 1024 and S <= 2 else 2, (n, bits))
    plan.close()


def test_extend_mixed_widths(agx, orc, dev):
    """19 primes cycling 30, 60, 61, 62 bits at n = 1024: seven and thirteen sources of every width under targets of every width"""
    n = 1024
    moduli = moduli_for(orc.find_prime, n, MIXED_WIDTHS)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for S in (7, 13):
        _check_extend(orc, dev, plan, n, moduli, S, 2, "mixed widths")
    plan.close()


# ---- agx_ntt_basis_mod_down_mode, agx_ntt_basis_mod_down ---------------------------------------------------------------------------------------------
def _mod_down(dev, call, xq, xp, in_place=False):
    """call(d_xq, d_xp, d_out, d_scratch) with an output and a scratch of its own (canary-filled; xq and xp checked unchanged), or with out == xq and
    scratch == xp: the sources given up.  Returns the output words"""
    d_xq, d_xp = dev.to_device(xq), dev.to_device(xp)
    if in_place:
        call(d_xq.data_ptr(), d_xp.data_ptr(), d_xq.data_ptr(), d_xp.data_ptr())
        return dev.to_host(d_xq)
    d_out, d_s = dev.to_device(canary(0, xq.size)), dev.to_device(canary(xq.size, xp.size))
    call(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr())
    got = dev.to_host(d_out)
    assert np.array_equal(dev.to_host(d_xq), xq) and np.array_equal(dev.to_host(d_xp), xp), "an input changed"
    return got


def _check_mod_down(agx, orc, dev, plan, n, moduli, S, launches, what, in_place, batch=BATCH, settings=SETTINGS):
    """every (t, mode): reduced and spread inputs out of place, spread inputs in place where asked; under FLOOR with t = 1 the frozen call too"""
    for t, mode in settings:
        xq, xp, lq, lp, want = mod_down_sweep_case(orc, n, moduli, S, batch, 100 * n + S, t, mode)
        basis = plan.basis(*mod_down_shape(S), t=t)
        assert basis.mod_down_launches() == launches, (what, S, launches)

        def by_mode(q, p, o, s):
            basis.mod_down(q, p, o, s, batch, dev.stream, mode)

        def frozen(q, p, o, s):
            assert agx.lib().agx_ntt_basis_mod_down(basis._h, q, p, o, s, batch, dev.stream) == 0

        runs = [("reduced", by_mode, xq, xp, False), ("spread", by_mode, lq, lp, False)]
        if in_place:
            runs.append(("in place, the sources given up", by_mode, lq, lp, True))
        if (t, mode) == (1, FLOOR):
            runs.append(("agx_ntt_basis_mod_down", frozen, lq, lp, False))
        for name, call, q_words, p_words, alias in runs:
            got = _mod_down(dev, call, q_words, p_words, alias)
            assert np.array_equal(got, want), (what, "S", S, "t", t, "mode", mode, name, "first differing words", _first_bad(got, want))
        basis.close()


@pytest.mark.parametrize("n,bits,launches", [(64, 60, 4), (64, 30, 4), (1024, 60, 2)], ids=["generic-64", "32-bit-64", "fused-1024"])
def test_mod_down_at_every_source_count(agx, orc, dev, n, bits, launches):
    """targets [0, 3), sources [3, 3 + S), FLOOR and ROUND, t = 1 and 65537.  n = 64 is the generic route, four launches: the scaled inverse of the
    sources (wave-packed, or 32-bit) and moddown_coeff_kernel / moddown_coeff_round_kernel at every capacity, partly and wholly filled; n = 1024 under
    AGX_VARIANT_AUTO is the fused route, two launches: the register-blocked scaled inverse and the kernel that walks the sources with its wrapping
    prefetch"""
    moduli = moduli_for(orc.find_prime, n, [bits] * SWEEP_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for S in SOURCE_COUNTS:
        _check_mod_down(agx, orc, dev, plan, n, moduli, S, launches, (n, bits), in_place=n == 64 or S in IN_PLACE_AT_1024)
    plan.close()


def test_mod_down_32_bit_kernels_of_1024_at_every_source_count(agx, orc, dev):
    """every modulus below 2^31 at n = 1024: the generic route again, through the register-blocked 32-bit inverse (scaled) and forward"""
    n = 1024
    moduli = moduli_for(orc.find_prime, n, [30] * SWEEP_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for S in SOURCE_COUNTS:
        _check_mod_down(agx, orc, dev, plan, n, moduli, S, 4, (n, 30), in_place=S in IN_PLACE_AT_1024, settings=((1, FLOOR), (T17, ROUND)))
    plan.close()


def test_mod_down_radix2_route_at_every_source_count(agx, orc, dev):
    """n = 1024 forced onto AGX_VARIANT_LDS_RADIX2: four launches, the radix-2 inverse carrying the scaled constants n^-1 D_i^-1; then the same basis back
    under AGX_VARIANT_AUTO (two launches) writes the same words"""
    n = 1024
    moduli = moduli_for(orc.find_prime, n, [60] * SWEEP_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for S in SOURCE_COUNTS:
        for t, mode in SETTINGS:
            _, _, lq, lp, want = mod_down_sweep_case(orc, n, moduli, S, BATCH, 100 * n + S, t, mode)
            basis = plan.basis(*mod_down_shape(S), t=t)
            for variant, launches in ((agx.VARIANT_LDS_RADIX2, 4), (agx.VARIANT_AUTO, 2)):
                plan.set_variant(variant)
                assert basis.mod_down_launches() == launches, (S, variant)
                got = _mod_down(dev, lambda q, p, o, s: basis.mod_down(q, p, o, s, BATCH, dev.stream, mode), lq, lp)
                assert np.array_equal(got, want), ("S", S, "t", t, "mode", mode, "variant", variant, "first differing words", _first_bad(got, want))
            basis.close()
    plan.close()


@pytest.mark.parametrize("n", [64, 1024])
def test_guard_bands_at_nine_sources(agx, orc, dev, n):
    """ROUND with t = 65537 from nine sources (capacity 16 partly filled; the fused kernel's prefetch ends on an odd source), every buffer at an odd word of
    one guarded allocation: out and scratch of their own, then out == xq and scratch == xp.  The same words both times, xq and xp unchanged where they are
    not given up, and every word outside out and the scratch keeps its value"""
    S, T = 9, 3
    moduli = moduli_for(orc.find_prime, n, [60] * SWEEP_PRIMES)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*mod_down_shape(S), t=T17)
    assert basis.mod_down_launches() == (4 if n == 64 else 2)
    _, _, xq, xp, want = mod_down_sweep_case(orc, n, moduli, S, BATCH, 100 * n + S, T17, ROUND)      # the spread words
    odd = lambda off: off + 1 - off % 2      # noqa: E731
    lq = Layout(n, T, BATCH, offset=1)
    lp = Layout(n, S, BATCH, offset=odd(lq.span() + 6))
    lo = Layout(n, T, BATCH, offset=odd(lp.span() + 10))
    ls = Layout(n, S, BATCH, offset=odd(lo.span() + 14))
    for out_l, scr_l in ((lo, ls), (lq, lp)):
        own = out_l is lo
        arena = arena_for(dev, n, (lq, xq), (lp, xp), *([(lo, None), (ls, None)] if own else []))
        basis.mod_down(arena.address(lq.offset), arena.address(lp.offset), arena.address(out_l.offset), arena.address(scr_l.offset), BATCH, dev.stream, ROUND)
        img = arena.image()
        judged = [(lq, xq), (lp, xp), (lo, None), (ls, None)] if own else [(lq, None), (lp, None)]
        assert not arena.faults(judged, img), ("a word outside out and the scratch changed", "own buffers" if own else "in place")
        assert np.array_equal(arena.frames(out_l, img), want), "own buffers" if own else "in place"
    basis.close()
    plan.close()


@pytest.mark.parametrize("config,n,max_bits", registry_entries([150, 93, 117]))
def test_mod_down_six_sources_on_a_registry_entry_per_size_class(agx, orc, dev, config, n, max_bits):
    """one entry that carries the fused kernel per size class (n = 1024, 4096, 16384), selected explicitly, six sources, two frames"""
    assert config in RESCALE_IDS
    S, batch = 6, 2
    moduli = moduli_for(orc.find_prime, n, [max_bits] * (3 + S))
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    _check_mod_down(agx, orc, dev, plan, n, moduli, S, 2, ("registry id", config), in_place=False, batch=batch, settings=((1, FLOOR), (T17, ROUND)))
    plan.close()
