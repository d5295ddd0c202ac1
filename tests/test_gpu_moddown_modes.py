"""agx_ntt_basis_mod_down_mode, agx_ntt_basis_create_plain and agx_ntt_keyswitch_create_plain on the device: ModDown with a rounding mode and a plaintext
modulus t, by the two-launch route and by the generic one.

The expected words come from Python integers, from the definition (moddown_modes_ref.mod_down_mode): with a_j, p_i the coefficient forms of the slabs,
h = floor(D / 2) under ROUND and 0 under FLOOR, y_i = ((p_i t^-1) + h) D_i^-1 mod q_i, V = sum_i y_i D_i as an integer,
out_j = (a_j - t (V - h)) D^-1 mod q_j; the GPU gets the CPU oracle's forward of a_j and p_i, reduced and spread over [0, 4q), and must return the oracle's
forward of out_j.  Every comparison is word for word."""
import functools

import numpy as np
import pytest

from gpu_util import (RESCALE_IDS, Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, registry_entries, rescale_reference, status_of)
from moddown_modes_ref import (FLOOR, ROUND, add_key_noise, deviation, half, keyswitch_plain_ref, lift_mode, mod_down_mode, mod_down_mode_ntt, plain_bound, sources_for_y,
                               special_sources)
from rns_ref import active_of, mod_down_ntt, oracle_forward_set, product, residues, rotation_key_case, spread

pytestmark = pytest.mark.gpu

# (source first, source count, target first, target count) on a plan of six primes
KEYSWITCH, SINGLE, BELOW = (4, 2, 0, 4), (5, 1, 0, 5), (0, 2, 3, 3)
SHAPES = (KEYSWITCH, SINGLE, BELOW)
SHAPE_IDS = ["keyswitch", "single", "below"]
MODES = (FLOOR, ROUND)
T17 = 65537
T_ABOVE = (1 << 64) - 59      # a prime above every modulus


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(rng, src, dst, batch, n, t, mode):
    """(a [T][batch][n], p [S][batch][n], exact): reduced coefficient-form residues and the (frame, first, last, words) regions whose result is known in
    closed form.  Frame 0 opens with the sources whose X mod D is 0, 1, H - 1, H, H + 1, D - 1 (H = floor(D / 2)) and with every y_i = q_i - 1, under
    random targets; its third quarter is X = D Y + t (V - h) with small random Y >= 1, whose result must be Y.  With five frames, frame 3 is that
    throughout, frame 1 has all-zero sources and frame 2 every source residue q_i - 1."""
    S, T = len(src), len(dst)
    a = np.stack([rng.integers(0, int(q), size=batch * n, dtype=np.uint64) for q in dst]).reshape(T, batch, n)
    p = np.stack([rng.integers(0, int(q), size=batch * n, dtype=np.uint64) for q in src]).reshape(S, batch, n)
    special = special_sources(src, t, mode)
    assert special.shape[1] <= n // 2
    p[:, 0, :special.shape[1]] = special
    if batch >= 5:
        p[:, 1, :] = 0
        p[:, 2, :] = np.array([int(q) - 1 for q in src], dtype=np.uint64)[:, None]
    D, h = product(src), half(src, mode)
    exact = []
    for f, lo, hi in [(0, n // 2, 3 * n // 4)] + ([(3, 0, n)] if batch >= 5 else []):
        V = lift_mode(p[:, f, lo:hi], src, t, mode)
        Y = rng.integers(1, 1 << 20, size=hi - lo).astype(object)
        a[:, f, lo:hi] = residues(D * Y + int(t) * (V - h), dst)
        exact.append((f, lo, hi, residues(Y, dst)))
    return a, p, exact


@functools.lru_cache(maxsize=None)
def _case(orc, n, moduli, shape, batch, seed, t, mode):
    """(xq, xp reduced; xq, xp spread over [0,4q); the expected words [T][batch][n]), all flat, computed once per case (read-only)"""
    sf, S, df, T = shape
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    rng = np.random.default_rng(seed)
    a, p, exact = make_inputs(rng, src, dst, batch, n, t, mode)
    coeff = mod_down_mode(a, p, src, dst, t, mode).reshape(T, batch, n)
    for f, lo, hi, want in exact:      # the closed form holds for the reference itself
        assert np.array_equal(coeff[:, f, lo:hi], want)
    xq, xp = oracle_forward_set(orc, n, dst, a), oracle_forward_set(orc, n, src, p)
    out = (xq.reshape(-1), xp.reshape(-1), spread(rng, xq, dst).reshape(-1), spread(rng, xp, src).reshape(-1), oracle_forward_set(orc, n, dst, coeff).reshape(-1))
    for w in out:
        w.setflags(write=False)
    return out


def _run(dev, basis, xq, xp, batch, mode, call=None):
    """out of place with a scratch of its own; returns the output words"""
    d_xq, d_xp = dev.to_device(xq), dev.to_device(xp)
    d_out, d_s = dev.to_device(canary(0, xq.size)), dev.empty(xp.size)
    if call is None:
        basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream, mode)
    else:
        call(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr())
    return dev.to_host(d_out)


def _check(orc, dev, plan, n, moduli, shape, batch, seed, t, mode, what):
    """from fully reduced inputs and from inputs spread over [0, 4q) on both xq and xp"""
    xq, xp, lq, lp, want = _case(orc, n, moduli, shape, batch, seed, t, mode)
    basis = plan.basis(*shape, t=t)
    for name, q_words, p_words in (("reduced", xq, xp), ("spread", lq, lp)):
        got = _run(dev, basis, q_words, p_words, batch, mode)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, t, mode, name, "first differing words", bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    basis.close()
    return want


# ---- parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_parity_60_bit(agx, orc, dev, n, batch, shape):
    """n = 64 is the generic route, 1024 the smallest size of the two-launch route; both modes, with and without a plaintext modulus"""
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for mode in MODES:
        for t in (1, T17):
            _check(orc, dev, plan, n, moduli, shape, batch, n * 7 + batch + shape[0], t, mode, (n, batch, shape))
    plan.close()


# ---- widths -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_parity_30_bit(agx, orc, dev, n):
    """plans whose moduli are all below 2^31: the generic route through the 32-bit kernels; at n = 64 also a t above every modulus"""
    moduli = moduli_for(orc.find_prime, n, [30] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for mode in MODES:
        for t in (T17, T_ABOVE) if n == 64 else (T17,):
            _check(orc, dev, plan, n, moduli, KEYSWITCH, 5, n + 30, t, mode, (n, "30-bit"))
    plan.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_parity_mixed_widths(agx, orc, dev, shape):
    n = 1024
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 30, 60, 60])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for t in (T17, 2) if shape == KEYSWITCH else (T17,):      # an even t on one case
        _check(orc, dev, plan, n, moduli, shape, 5, 1024 + shape[0], t, ROUND, ("mixed", shape))
    plan.close()


def test_sixteen_sources_of_62_bits(agx, orc, dev):
    """the accumulation edge under ROUND: sixteen 62-bit sources -> one 62-bit target; in the first half of the frame every y_i arrives as q_i - 1, so
    that y_i + c_i wraps modulo q_i for every source; random behind"""
    n, batch = 1024, 1
    moduli = tuple(agx.find_primes(62, n, 17))
    assert all(q > 1 << 61 for q in moduli)
    src, dst = moduli[:16], moduli[16:]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(0, 16, 16, 1)
    rng = np.random.default_rng(62)
    D = product(src)
    p = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in src])
    top = np.array([[q - 1] for q in src], dtype=object)
    p[:, :n // 2] = sources_for_y(top, src, 1, FLOOR)      # y_i = q_i - 1 before c_i is added
    c = [(D // 2) * pow(D // q, -1, q) % q for q in src]
    assert all(ci > 0 for ci in c), "some c_i is 0: nothing wraps"
    assert int(lift_mode(p[:, :1], src, 1, ROUND)[0]) == sum((ci - 1) * (D // q) for ci, q in zip(c, src))      # y_i = c_i - 1: wrapped
    a = rng.integers(0, dst[0], size=(1, n), dtype=np.uint64)
    want = oracle_forward_set(orc, n, dst, mod_down_mode(a, p, src, dst, 1, ROUND)).reshape(-1)
    xq, xp = oracle_forward_set(orc, n, dst, a), oracle_forward_set(orc, n, src, p)
    for q_words, p_words in ((xq, xp), (spread(rng, xq, dst), spread(rng, xp, src))):
        assert np.array_equal(_run(dev, basis, q_words.reshape(-1), p_words.reshape(-1), batch, ROUND), want)
    basis.close()
    plan.close()


@pytest.mark.parametrize("config,n,max_bits", registry_entries(RESCALE_IDS))
def test_every_registry_entry_at_its_own_size(agx, orc, dev, config, n, max_bits):
    """each entry that carries the fused kernel, selected explicitly (AGX_VARIANT_REGBLOCK_BASE + id) under the widest modulus it admits"""
    batch, shape = 2, (2, 2, 0, 2)
    moduli = moduli_for(orc.find_prime, n, [max_bits] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    basis = plan.basis(*shape, t=T17)
    assert basis.mod_down_launches() == 2, "the entry does not carry the fused kernel"
    basis.close()
    _check(orc, dev, plan, n, moduli, shape, batch, config + 2, T17, ROUND, ("registry id", config))
    plan.close()


# ---- equalities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_one_source_at_the_top_level_is_rescale_in_the_same_mode(agx, orc, dev, n):
    batch = 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*SINGLE)
    for mode, rescale_mode in ((ROUND, agx.RESCALE_ROUND), (FLOOR, agx.RESCALE_FLOOR)):
        xq, xp, _, _, want = _case(orc, n, moduli, SINGLE, batch, n * 7 + batch + SINGLE[0], 1, mode)
        d_x = dev.to_device(np.concatenate([xq, xp]))
        d_out, d_s = dev.empty(xq.size), dev.empty(xp.size)
        plan.rescale(d_x.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, rescale_mode, dev.stream)
        assert np.array_equal(dev.to_host(d_out), want), ("rescale differs from the reference", mode)
        assert np.array_equal(_run(dev, basis, xq, xp, batch, mode), want), ("mod_down_mode differs from rescale", mode)
    basis.close()
    plan.close()


@pytest.mark.parametrize("n", [64, 1024])
def test_one_source_one_level_down_is_the_rounded_division(agx, orc, dev, n):
    """sources {3}, targets [0, 3) of six primes: floor((X + h) / q_3) for the X the four residues represent -- the rounding rescale at level 4 of
    one plan, in place on the level's own slabs (d_xq = x, d_xp = d_scratch = x + 3 batch n)"""
    batch = 3
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    level = moduli[:4]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(3, 1, 0, 3)
    rng = np.random.default_rng(n + 3)
    x = np.stack([rng.integers(0, int(q), size=batch * n, dtype=np.uint64) for q in level])
    x[3, :6] = [0, 1, int(level[3]) // 2 - 1, int(level[3]) // 2, int(level[3]) // 2 + 1, int(level[3]) - 1]
    xhat = oracle_forward_set(orc, n, level, x)
    for mode in MODES:
        want = oracle_forward_set(orc, n, level[:3], rescale_reference(x, level, mode)).reshape(-1)
        d_x = dev.to_device(spread(rng, xhat, level).reshape(-1))
        base, last = d_x.data_ptr(), d_x.data_ptr() + 8 * 3 * batch * n
        basis.mod_down(base, last, base, last, batch, dev.stream, mode)
        assert np.array_equal(dev.to_host(d_x)[:3 * batch * n], want), mode
    basis.close()
    plan.close()


@pytest.mark.parametrize("n", [64, 1024])
def test_floor_and_t_1_are_the_ordinary_calls(agx, orc, dev, n):
    """FLOOR on an ordinary basis is Basis.mod_down's call (agx_ntt_basis_mod_down itself, reached through ctypes); a t = 1 plain basis equals the ordinary
    one in both modes; extend on a plain basis (t = 65537) writes what the ordinary one writes, in both forms"""
    batch, shape = 5, KEYSWITCH
    sf, S, df, T = shape
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ordinary, one, plain = plan.basis(*shape), plan.basis(*shape, t=1), plan.basis(*shape, t=T17)
    _, _, lq, lp, want = _case(orc, n, moduli, shape, batch, n + 5, 1, FLOOR)
    assert np.array_equal(want, mod_down_ntt(orc, n, lq, lp, src, dst).reshape(-1)), "the reference with t = 1 and FLOOR is not rns_ref's"

    def frozen(q, p, o, s):
        assert agx.lib().agx_ntt_basis_mod_down(ordinary._h, q, p, o, s, batch, dev.stream) == 0

    assert np.array_equal(_run(dev, ordinary, lq, lp, batch, None, frozen), want)
    assert np.array_equal(_run(dev, ordinary, lq, lp, batch, FLOOR), want)
    assert np.array_equal(_run(dev, one, lq, lp, batch, FLOOR), want)
    rounded = _run(dev, ordinary, lq, lp, batch, ROUND)
    assert np.array_equal(rounded, mod_down_mode_ntt(orc, n, lq, lp, src, dst, 1, ROUND).reshape(-1))
    assert np.array_equal(_run(dev, one, lq, lp, batch, ROUND), rounded)
    # on a plain basis the frozen call is the FLOOR mode with that t
    want_t = mod_down_mode_ntt(orc, n, lq, lp, src, dst, T17, FLOOR).reshape(-1)

    def frozen_plain(q, p, o, s):
        assert agx.lib().agx_ntt_basis_mod_down(plain._h, q, p, o, s, batch, dev.stream) == 0

    assert np.array_equal(_run(dev, plain, lq, lp, batch, None, frozen_plain), want_t)
    rng = np.random.default_rng(n)
    x = np.stack([rng.integers(0, 4 * int(q), size=batch * n, dtype=np.uint64) for q in src]).reshape(-1)
    d_x = dev.to_device(x)
    for form in (agx.FORM_COEFF, agx.FORM_NTT):
        outs = []
        for b in (ordinary, plain):
            d_out = dev.to_device(canary(0, T * batch * n))
            b.extend(d_x.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
            outs.append(dev.to_host(d_out))
        assert np.array_equal(outs[0], outs[1]), ("extend on a plain basis differs", form)
    assert ordinary.info() == plain.info()
    for b in (ordinary, one, plain):
        b.close()
    plan.close()


# ---- aliasing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_aliasing_and_guard_bands(agx, orc, dev, n):
    """ROUND with t = 65537, every buffer at an odd word of one allocation: out and scratch of their own (xq and xp unchanged), out == xq, scratch == xp,
    both: the same words every time, and every word outside out and the scratch keeps its value"""
    batch, shape = 2, KEYSWITCH
    _, S, _, T = shape
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape, t=T17)
    _, _, xq, xp, want = _case(orc, n, moduli, shape, batch, n + 17, T17, ROUND)      # lazy words: the in-place finish reads them where it writes
    odd = lambda off: off + 1 - off % 2      # noqa: E731
    lq = Layout(n, T, batch, offset=1)
    lp = Layout(n, S, batch, offset=odd(lq.span() + 6))
    lo = Layout(n, T, batch, offset=odd(lp.span() + 10))
    ls = Layout(n, S, batch, offset=odd(lo.span() + 14))
    assert all(l.offset % 2 == 1 for l in (lq, lp, lo, ls))
    for out_l, scr_l in ((lo, ls), (lq, ls), (lo, lp), (lq, lp)):
        placed = [(lq, xq), (lp, xp)] + ([(lo, None)] if out_l is lo else []) + ([(ls, None)] if scr_l is ls else [])
        arena = arena_for(dev, n, *placed)
        basis.mod_down(arena.address(lq.offset), arena.address(lp.offset), arena.address(out_l.offset), arena.address(scr_l.offset), batch, dev.stream, ROUND)
        img = arena.image()
        judged = [(lq, None if out_l is lq else xq), (lp, None if scr_l is lp else xp)] + ([(lo, None)] if out_l is lo else []) + ([(ls, None)] if scr_l is ls else [])
        assert not arena.faults(judged, img), ("a word outside out and the scratch changed", out_l is lq, scr_l is lp)
        assert np.array_equal(arena.frames(out_l, img), want), ("in place" if out_l is lq else "out of place", "scratch is xp" if scr_l is lp else "own scratch")
    basis.close()
    plan.close()


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def test_every_route_gives_the_same_words(agx, orc, dev):
    """one basis under ROUND, the plan switched AUTO -> LDS_RADIX2 -> REGBLOCK -> AUTO between its calls; the launch counts are mod_down_launches()'s"""
    n, batch, shape = 1024, 5, KEYSWITCH
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    xq, xp, lq, lp, want = _case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0], T17, ROUND)
    basis = plan.basis(*shape, t=T17)
    for variant, launches in ((agx.VARIANT_AUTO, 2), (agx.VARIANT_LDS_RADIX2, 4), (agx.VARIANT_REGBLOCK, 2), (agx.VARIANT_AUTO, 2)):
        plan.set_variant(variant)
        assert basis.mod_down_launches() == launches, (variant, launches)
        for q_words, p_words in ((xq, xp), (lq, lp)):
            assert np.array_equal(_run(dev, basis, q_words, p_words, batch, ROUND), want), ("variant", variant)
    basis.close()
    plan.close()


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_the_call_is_graph_capturable(agx, orc, dev):
    """one ROUND call captured on a side stream (no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    n, batch, shape = 4096, 5, KEYSWITCH
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape, t=T17)
    cases = [_case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0], T17, ROUND), _case(orc, n, moduli, shape, batch, n + 99, T17, ROUND)]
    d_xq, d_xp = dev.to_device(cases[0][0]), dev.to_device(cases[0][1])
    d_out, d_s = dev.empty(cases[0][0].size), dev.empty(cases[0][1].size)

    def call(s):
        basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, s, ROUND)

    graph = capture(dev, call, call)
    for xq, xp, lq, lp, want in cases[::-1]:
        for q_words, p_words in ((xq, xp), (lq, lp)):
            d_xq.copy_(torch.from_numpy(q_words.view(np.int64).copy()))
            d_xp.copy_(torch.from_numpy(p_words.view(np.int64).copy()))
            d_out.zero_()
            graph.replay()
            dev.sync()
            assert np.array_equal(dev.to_host(d_out), want), "replay"
    basis.close()
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_rejected_calls_write_nothing(agx, orc, dev, n):
    import ctypes

    batch, shape = 2, (2, 2, 0, 2)
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape, t=T17)
    xq, xp, _, _, want = _case(orc, n, moduli, shape, batch, 3 * n + 60, T17, ROUND)
    lq = Layout(n, T, batch, offset=0)
    lp = Layout(n, S, batch, offset=lq.span() + 2 * n)
    lo = Layout(n, T, batch, offset=lp.span() + 2 * n)
    ls = Layout(n, S, batch, offset=lo.span() + 2 * n)
    arena = arena_for(dev, n, (lq, xq), (lp, xp), (lo, None), (ls, None))
    before = arena.image()
    q, p, o, s = (arena.address(l.offset) for l in (lq, lp, lo, ls))
    st, w, qw, pw = dev.stream, 8, T * batch * n, S * batch * n
    M = lambda *args: basis.mod_down(*args, ROUND)      # noqa: E731
    for mode in (7, 2, -1):      # a mode other than the two
        assert status_of(agx, basis.mod_down, q, p, o, s, batch, st, mode) == 5
    assert status_of(agx, basis.mod_down, 0, p, o, s, batch, st, 7) == 1      # the NULL rule comes first
    for k in range(4):      # NULL pointers
        args = [q, p, o, s]
        args[k] = 0
        assert status_of(agx, M, *args, batch, st) == 1
    for k in range(4):      # uint64_t data
        args = [q, p, o, s]
        args[k] += 4
        assert status_of(agx, M, *args, batch, st) == 5
    assert status_of(agx, M, q, p, o, s, 1 << 40, st) == 5                           # a batch past the grid limit
    if basis.mod_down_launches() == 2:      # the two-launch route: T workgroups per frame, 2 (2^30 + 1) of them are past 2^31 - 1
        assert status_of(agx, M, q, p, o, s, (1 << 30) + 1, st) == 5
    assert status_of(agx, M, q, p, q + w * (n // 2), s, batch, st) == 5              # out partially over xq
    assert status_of(agx, M, q + w * (n // 2), p, q, s, batch, st) == 5              # xq starts inside out
    assert status_of(agx, M, q, p, p, s, batch, st) == 5                             # out touching xp
    assert status_of(agx, M, q, p, p - w * (qw - 1), s, batch, st) == 5              # out's last word is xp's first
    assert status_of(agx, M, q, p, s, s, batch, st) == 5                             # out touching the scratch
    assert status_of(agx, M, q, p, o, o + w * (qw - 1), batch, st) == 5
    assert status_of(agx, M, q, p, q, p - w, batch, st) == 5                         # in place, the scratch over xp without being it
    assert status_of(agx, M, q, p, o, q, batch, st) == 5                             # the scratch touching xq
    assert status_of(agx, M, q, p, o, p + w * (n // 2), batch, st) == 5              # the scratch partially over xp
    overlapping = plan.basis(0, 2, 1, 2, t=T17)      # a target modulus that is a source modulus: the basis exists, the call refuses
    assert status_of(agx, overlapping.mod_down, q, p, o, s, batch, st, ROUND) == 3
    overlapping.close()
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    no_inverse = fwd_only.basis(*shape, t=T17)
    assert status_of(agx, no_inverse.mod_down, q, p, o, s, batch, st, ROUND) == 9
    no_inverse.close()
    fwd_only.close()
    # creation: t = 0 is a bad argument; t = a source modulus, or twice it, a bad modulus; a target modulus is fine; the out-pointer stays NULL
    L = agx.lib()
    for t, status in ((0, 5), (moduli[2], 3), (2 * moduli[3], 3), (3 * moduli[2], 3)):
        h = ctypes.c_void_p(0x1234)
        assert L.agx_ntt_basis_create_plain(ctypes.byref(h), plan._h, *shape, t) == status and h.value is None, t
        assert status_of(agx, plan.basis, *shape, t) == status
    assert status_of(agx, plan.basis, 0, 0, 0, 2, 0) == 5 and status_of(agx, plan.basis, 0, 1, 0, 5, T17) == 5      # basis_create's range rules stand
    plan.basis(*shape, t=moduli[0]).close()
    # the key switch: Q = primes [0, 2), special primes [2, 4)
    for t, status in ((0, 5), (moduli[3], 3), (2 * moduli[2], 3)):
        h = ctypes.c_void_p(0x1234)
        assert L.agx_ntt_keyswitch_create_plain(ctypes.byref(h), plan._h, 2, 2, 2, 2, t) == status and h.value is None, t
        assert status_of(agx, plan.keyswitch, 2, 2, 2, 2, t) == status
    assert status_of(agx, plan.keyswitch, 0, 2, 2, 2, 0) == 5 and status_of(agx, plan.keyswitch, 2, 1, 2, 2, T17) == 5      # keyswitch_create's rules stand
    plan.keyswitch(2, 2, 2, 2, t=moduli[0]).close()      # t = 0 modulo a prime of Q only: the special primes decide
    M(q, p, o, s, 0, st)      # empty batch: nothing launched
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    M(q, p, o, s, batch, st)
    assert np.array_equal(arena.frames(lo), want)
    basis.close()
    plan.close()


# ---- the BGV key switch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 4, 2, 2), (3, 4, 2, 2)], ids=["top", "lower"])
@pytest.mark.parametrize("n", [64, 1024])
def test_bgv_key_switch(agx, orc, dev, n, shape):
    """a handle of agx_ntt_keyswitch_create_plain with t = 65537: apply (g = 1) and decompose + apply_decomposed (g = 5), word for word against the
    reference key switch; with a key carrying noise t e the deviation out_0 + out_1 s - c s' is 0 modulo t on every coefficient and far from wrapping
    modulo Q; with a noise-free key it is within t p_count (1 + ||s||_1), asserted of the reference first"""
    batch, t = 2, T17
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    Qp = product(active_of(moduli, shape)[:shape[0]])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape, t=t)
    q_count = shape[0]
    for g in (1, 5):
        chat, clean, s, shat = rotation_key_case(orc, n, moduli, shape, g, batch, n + g + shape[0])
        noisy = add_key_noise(orc, n, moduli, shape, clean, t, np.random.default_rng(n + g))
        for key, is_noisy in ((clean, False), (noisy, True)):
            want = keyswitch_plain_ref(orc, n, moduli, shape, chat, key, batch, t, g)
            dv = deviation(orc, n, moduli, shape, g, batch, chat, shat, want)      # of the reference, on the CPU, first
            assert all(int(x) % t == 0 for x in dv), "the reference's deviation is not 0 modulo t"
            assert max(abs(int(x)) for x in dv) < Qp >> 64, "the reference's deviation wraps modulo Q"
            if not is_noisy:
                assert max(abs(int(x)) for x in dv) <= plain_bound(shape, s, t)
            d_chat, d_key = dev.to_device(chat.reshape(-1)), dev.to_device(np.asarray(key).reshape(-1))
            d_out = dev.to_device(canary(0, 2 * q_count * batch * n))
            if g == 1:
                d_s = dev.empty(ks.scratch_words(batch))
                ks.apply(d_chat.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream)
            else:
                ext_words, dec_words, app_words = ks.hoisted_words(batch)
                d_ext, d_dec, d_app = dev.empty(ext_words), dev.empty(dec_words), dev.empty(app_words)
                ks.decompose(d_chat.data_ptr(), d_ext.data_ptr(), d_dec.data_ptr(), batch, dev.stream)
                ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_app.data_ptr(), batch, g, dev.stream)
            got = dev.to_host(d_out)
            assert np.array_equal(got, want.reshape(-1)), ("g", g, "noisy" if is_noisy else "noise-free")
            dv = deviation(orc, n, moduli, shape, g, batch, chat, shat, got)
            assert all(int(x) % t == 0 for x in dv) and max(abs(int(x)) for x in dv) < Qp >> 64
            if not is_noisy:
                assert max(abs(int(x)) for x in dv) <= plain_bound(shape, s, t)
    ks.close()
    plan.close()
