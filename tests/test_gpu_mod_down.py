"""agx_ntt_basis_mod_down on the device: ModDown of a hybrid key switch on NTT-form frames, by the two-launch route and by the generic one.

The expected words come from Python integers, from the definition (rns_ref.mod_down): with a_j, p_i the coefficient forms of the slabs,
y_i = p_i (D_i^-1 mod q_i) mod q_i, V = sum_i y_i D_i as an integer, out_j = (a_j - V) (D^-1 mod q_j) mod q_j; the GPU gets the CPU oracle's forward
of a_j and p_i and must return the oracle's forward of out_j.  Every comparison is word for word."""
import functools

import numpy as np
import pytest

from gpu_util import RESCALE_IDS, Layout, arena_for, assert_equals_chunked_calls, canary, capture, judged_frames, moduli_for, plan_for_moduli, registry_entries, status_of
from rns_ref import device_residues, lift, mod_down, mod_down_ntt, oracle_forward_set, product, residues, special_values, spread

pytestmark = pytest.mark.gpu

# (source first, source count, target first, target count) on a plan of six primes
KEYSWITCH, DROPPED, SINGLE, BELOW = (4, 2, 0, 4), (4, 2, 0, 2), (5, 1, 0, 5), (0, 2, 3, 3)
SHAPES = (KEYSWITCH, DROPPED, SINGLE, BELOW)
SHAPE_IDS = ["keyswitch", "dropped", "single", "below"]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(rng, src, dst, batch, n):
    """(a [T][batch][n], p [S][batch][n], exact): reduced coefficient-form residues and the (frame, first, last, kind) regions whose result is
    known in closed form.  Frame 0 opens with the special values of the sources under random targets; its third quarter is X = D Y + V with small
    random Y (the result must be Y mod q_j), its last quarter has a_j = V mod q_j (the result must be zero).  With five frames, frame 1 has
    all-zero sources, frame 2 every source residue q_i - 1, frame 3 is X = D Y + V throughout and frame 4 a_j = V mod q_j throughout."""
    S, T = len(src), len(dst)
    a = np.stack([rng.integers(0, int(q), size=batch * n, dtype=np.uint64) for q in dst]).reshape(T, batch, n)
    p = np.stack([rng.integers(0, int(q), size=batch * n, dtype=np.uint64) for q in src]).reshape(S, batch, n)
    special = residues(special_values(src), src)
    k = min(n // 2, special.shape[1])
    p[:, 0, :k] = special[:, :k]
    if batch >= 5:
        p[:, 1, :] = 0
        p[:, 2, :] = np.array([int(q) - 1 for q in src], dtype=np.uint64)[:, None]
    D = product(src)
    regions = [(0, n // 2, 3 * n // 4, "quotient"), (0, 3 * n // 4, n, "zero")] + ([(3, 0, n, "quotient"), (4, 0, n, "zero")] if batch >= 5 else [])
    exact = []
    for f, lo, hi, kind in regions:
        V = lift(p[:, f, lo:hi], src)
        Y = rng.integers(0, 1 << 20, size=hi - lo).astype(object) if kind == "quotient" else np.zeros(hi - lo, dtype=object)
        a[:, f, lo:hi] = residues(D * Y + V, dst)
        exact.append((f, lo, hi, residues(Y, dst)))
    return a, p, exact


@functools.lru_cache(maxsize=None)
def _case(orc, n, moduli, shape, batch, seed):
    """(xq, xp reduced; xq, xp spread over [0,4q); the expected words [T][batch][n]), all flat, computed once per case (read-only)"""
    sf, S, df, T = shape
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    rng = np.random.default_rng(seed)
    a, p, exact = make_inputs(rng, src, dst, batch, n)
    coeff = mod_down(a, p, src, dst).reshape(T, batch, n)
    for f, lo, hi, want in exact:      # the closed forms hold for the reference itself
        assert np.array_equal(coeff[:, f, lo:hi], want)
    xq, xp = oracle_forward_set(orc, n, dst, a), oracle_forward_set(orc, n, src, p)
    out = (xq.reshape(-1), xp.reshape(-1), spread(rng, xq, dst).reshape(-1), spread(rng, xp, src).reshape(-1), oracle_forward_set(orc, n, dst, coeff).reshape(-1))
    for w in out:
        w.setflags(write=False)
    return out


def _run(dev, basis, xq, xp, batch):
    """out of place with a scratch of its own; returns the output words"""
    d_xq, d_xp = dev.to_device(xq), dev.to_device(xp)
    d_out, d_s = dev.to_device(canary(0, xq.size)), dev.empty(xp.size)
    basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    return dev.to_host(d_out)


def _check(orc, dev, plan, n, moduli, shape, batch, seed, what):
    """from fully reduced inputs and from inputs spread over [0, 4q) on both xq and xp"""
    xq, xp, lq, lp, want = _case(orc, n, moduli, shape, batch, seed)
    basis = plan.basis(*shape)
    for name, q_words, p_words in (("reduced", xq, xp), ("spread", lq, lp)):
        got = _run(dev, basis, q_words, p_words, batch)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, name, "first differing words", bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    basis.close()
    return want


# ---- parity -------------------------------------------------------------------------------------------------------------------------
SIZES = [8, 64, 512, 1024, 4096, 16384, 32768]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", SIZES)
def test_parity_60_bit(agx, orc, dev, n, batch, shape):
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    want = _check(orc, dev, plan, n, moduli, shape, batch, n * 7 + batch + shape[0], (n, batch, shape))
    if shape == SINGLE:      # S = 1 is agx_ntt_rescale(..., AGX_RESCALE_FLOOR) on the same words
        xq, xp, _, _, _ = _case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0])
        d_x = dev.to_device(np.concatenate([xq, xp]))
        d_out, d_s = dev.empty(xq.size), dev.empty(xp.size)
        plan.rescale(d_x.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, agx.RESCALE_FLOOR, dev.stream)
        assert np.array_equal(dev.to_host(d_out), want), "S = 1 differs from rescale in floor mode"
    plan.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_parity_30_bit(agx, orc, dev, n, shape):
    """plans whose moduli are all below 2^31: the generic route through the 32-bit kernels, whose inverse takes the scaled constants too"""
    moduli = moduli_for(orc.find_prime, n, [30] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(orc, dev, plan, n, moduli, shape, 5, n + 30 + shape[0], (n, "30-bit", shape))
    plan.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_parity_mixed_widths(agx, orc, dev, shape):
    n = 1024
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 30, 60, 60])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check(orc, dev, plan, n, moduli, shape, 5, 1024 + shape[0], ("mixed", shape))
    plan.close()


def test_sixteen_sources_of_62_bits(agx, orc, dev):
    """the accumulation edge: sixteen 62-bit sources -> one 62-bit target with every y_i = q_i - 1 (the largest sum) in the first half of the
    frame, random behind"""
    n, batch = 1024, 1
    moduli = tuple(agx.find_primes(62, n, 17))
    assert all(q > 1 << 61 for q in moduli)
    src, dst = moduli[:16], moduli[16:]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(0, 16, 16, 1)
    rng = np.random.default_rng(62)
    D = product(src)
    p = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in src])
    p[:, :n // 2] = np.array([(q - 1) * (D // q) % q for q in src], dtype=np.uint64)[:, None]
    assert lift(p[:, :1], src)[0] == sum((q - 1) * (D // q) for q in src)
    a = rng.integers(0, dst[0], size=(1, n), dtype=np.uint64)
    want = oracle_forward_set(orc, n, dst, mod_down(a, p, src, dst)).reshape(-1)
    xq, xp = oracle_forward_set(orc, n, dst, a), oracle_forward_set(orc, n, src, p)
    for q_words, p_words in ((xq, xp), (spread(rng, xq, dst), spread(rng, xp, src))):
        assert np.array_equal(_run(dev, basis, q_words.reshape(-1), p_words.reshape(-1), batch), want)
    basis.close()
    plan.close()


# ---- aliasing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096, 32768])
def test_aliasing_and_guard_bands(agx, orc, dev, n):
    """out and scratch of their own (xq and xp unchanged), out == xq, scratch == xp, both: the same words every time, and every word outside
    out and the scratch keeps its value"""
    batch, shape = 2, KEYSWITCH
    _, S, _, T = shape
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    _, _, xq, xp, want = _case(orc, n, moduli, shape, batch, n + 17)      # lazy words: the in-place finish reads them where it writes
    lq = Layout(n, T, batch, offset=0)
    lp = Layout(n, S, batch, offset=lq.span() + 6)
    lo = Layout(n, T, batch, offset=lp.span() + 10)
    ls = Layout(n, S, batch, offset=lo.span() + 14)
    for out_l, scr_l in ((lo, ls), (lq, ls), (lo, lp), (lq, lp)):
        placed = [(lq, xq), (lp, xp)] + ([(lo, None)] if out_l is lo else []) + ([(ls, None)] if scr_l is ls else [])
        arena = arena_for(dev, n, *placed)
        basis.mod_down(arena.address(lq.offset), arena.address(lp.offset), arena.address(out_l.offset), arena.address(scr_l.offset), batch, dev.stream)
        img = arena.image()
        judged = [(lq, None if out_l is lq else xq), (lp, None if scr_l is lp else xp)] + ([(lo, None)] if out_l is lo else []) + ([(ls, None)] if scr_l is ls else [])
        assert not arena.faults(judged, img), ("a word outside out and the scratch changed", out_l is lq, scr_l is lp)
        assert np.array_equal(arena.frames(out_l, img), want), ("in place" if out_l is lq else "out of place", "scratch is xp" if scr_l is lp else "own scratch")
    basis.close()
    plan.close()


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def _fused_expected(n, bits, S):
    """the route shipped (profiles/r09_mod_down.md): the two-launch route serves 64-bit plans of n >= 1024 at every source count measured
    (S = 1, 2, 4, 8, 16)"""
    return n >= 1024 and bits > 31


def test_launch_counts_follow_the_route(agx, orc, dev):
    """two launches where the fused kernel serves under AGX_VARIANT_AUTO; four elsewhere, seven where the radix-2 transforms take two each"""
    for n, bits in [(1024, 60), (2048, 61), (4096, 60), (8192, 62), (16384, 60), (32768, 60), (8, 60), (64, 60), (512, 60), (64, 30), (1024, 30), (4096, 30)]:
        plan, _ = plan_for_moduli(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 6))
        for S in (1, 2, 3, 4):
            basis = plan.basis(2, S, 0, 2)
            fused = _fused_expected(n, bits, S)
            assert basis.mod_down_launches() == (2 if fused else 4), (n, bits, S)
            plan.set_variant(agx.VARIANT_LDS_RADIX2)      # computed at the info call: the basis follows the plan's variant
            assert basis.mod_down_launches() == (4 if n <= 16384 else 7), (n, bits, S, "radix-2")
            plan.set_variant(agx.VARIANT_AUTO)
            if fused:
                plan.set_variant(agx.VARIANT_REGBLOCK)
                assert basis.mod_down_launches() == 2, (n, bits, S, "regblock")
                plan.set_variant(agx.VARIANT_AUTO)
            assert basis.mod_down_launches() == (2 if fused else 4), (n, bits, S, "auto again")
            basis.close()
        plan.close()


@pytest.mark.parametrize("n", [1024, 4096, 16384, 32768])
def test_every_route_gives_the_same_words(agx, orc, dev, n):
    """one basis, the plan switched AUTO -> LDS_RADIX2 -> REGBLOCK -> AUTO between its calls"""
    batch, shape = 5, KEYSWITCH
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    xq, xp, lq, lp, want = _case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0])
    basis = plan.basis(*shape)
    for variant, launches in ((agx.VARIANT_AUTO, 2), (agx.VARIANT_LDS_RADIX2, 4 if n <= 16384 else 7), (agx.VARIANT_REGBLOCK, 2), (agx.VARIANT_AUTO, 2)):
        plan.set_variant(variant)
        assert basis.mod_down_launches() == launches, (variant, launches)
        for q_words, p_words in ((xq, xp), (lq, lp)):
            assert np.array_equal(_run(dev, basis, q_words, p_words, batch), want), ("variant", variant)
    basis.close()
    plan.close()


@pytest.mark.parametrize("config,n,max_bits", registry_entries(RESCALE_IDS))
def test_every_registry_entry_at_its_own_size(agx, orc, dev, config, n, max_bits):
    """each entry selected explicitly (AGX_VARIANT_REGBLOCK_BASE + id) under the widest modulus it admits; every one of them holds one frame
    per workgroup, so batch 2 = frames per workgroup + 1; one source and two"""
    batch = 2
    moduli = moduli_for(orc.find_prime, n, [max_bits] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    for shape in ((3, 1, 0, 3), (2, 2, 0, 2)):
        basis = plan.basis(*shape)
        assert basis.mod_down_launches() == 2, "the entry does not carry the fused kernel"
        basis.close()
        _check(orc, dev, plan, n, moduli, shape, batch, config + shape[1], ("registry id", config, shape))
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits", [(64, 60), (4096, 60), (4096, 30)])
def test_rejected_calls_write_nothing(agx, orc, dev, n, bits):
    batch, shape = 2, (2, 2, 0, 2)
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [bits] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    xq, xp, _, _, want = _case(orc, n, moduli, shape, batch, 3 * n + bits)
    lq = Layout(n, T, batch, offset=0)
    lp = Layout(n, S, batch, offset=lq.span() + 2 * n)
    lo = Layout(n, T, batch, offset=lp.span() + 2 * n)
    ls = Layout(n, S, batch, offset=lo.span() + 2 * n)
    arena = arena_for(dev, n, (lq, xq), (lp, xp), (lo, None), (ls, None))
    before = arena.image()
    q, p, o, s = (arena.address(l.offset) for l in (lq, lp, lo, ls))
    st, w, qw, pw = dev.stream, 8, T * batch * n, S * batch * n
    M = basis.mod_down
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
    assert status_of(agx, M, q, p, q + w * (qw - 1), s, batch, st) == 5              # ... on its last word
    assert status_of(agx, M, q + w * (n // 2), p, q, s, batch, st) == 5              # xq starts inside out
    assert status_of(agx, M, q, p, p, s, batch, st) == 5                             # out touching xp
    assert status_of(agx, M, q, p, p + w * (pw - 1), s, batch, st) == 5
    assert status_of(agx, M, q, p, p - w * (qw - 1), s, batch, st) == 5              # out's last word is xp's first
    assert status_of(agx, M, q, p, s, s, batch, st) == 5                             # out touching the scratch
    assert status_of(agx, M, q, p, o, o + w * (qw - 1), batch, st) == 5
    assert status_of(agx, M, q, p, o, o - w * (pw - 1), batch, st) == 5
    assert status_of(agx, M, q, p, q, p - w, batch, st) == 5                         # in place, the scratch over xp without being it
    assert status_of(agx, M, q, p, o, q, batch, st) == 5                             # the scratch touching xq
    assert status_of(agx, M, q, p, o, q + w * (qw - 1), batch, st) == 5
    assert status_of(agx, M, q, p, q, q, batch, st) == 5
    assert status_of(agx, M, q, p, o, p + w * (n // 2), batch, st) == 5              # the scratch partially over xp
    assert status_of(agx, M, q, p, o, p - w * (pw - 1), batch, st) == 5
    # a target modulus that is a source modulus: the basis exists (agx_ntt_basis_extend serves it), the call refuses
    for ranges in ((0, 2, 1, 2), (0, 2, 0, 2), (1, 1, 0, 2)):
        overlapping = plan.basis(*ranges)
        assert status_of(agx, overlapping.mod_down, q, p, o, s, batch, st) == 3, ranges
        overlapping.close()
    twice, _ = plan_for_moduli(agx, orc, n, (moduli[0], moduli[1], moduli[0]))
    equal = twice.basis(2, 1, 0, 2)      # disjoint ranges, but q_0 == q_2
    assert status_of(agx, equal.mod_down, q, p, o, s, 1, st) == 3
    equal.close()
    twice.close()
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    no_inverse = fwd_only.basis(*shape)
    assert status_of(agx, no_inverse.mod_down, q, p, o, s, batch, st) == 9
    no_inverse.close()
    fwd_only.close()
    M(q, p, o, s, 0, st)      # empty batch: nothing launched
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # ranges that meet end to end are accepted: xq | xp | out | scratch back to back
    packed = arena_for(dev, n, (Layout(n, T, batch, offset=0), xq), (Layout(n, S, batch, offset=qw), xp), (Layout(n, T, batch, offset=qw + pw), None),
                       (Layout(n, S, batch, offset=2 * qw + pw), None))
    b = packed.address(0)
    M(b, b + w * qw, b + w * (qw + pw), b + w * (2 * qw + pw), batch, st)
    assert np.array_equal(packed.frames(Layout(n, T, batch, offset=qw + pw)), want)
    basis.close()
    plan.close()


# ---- graph capture, placement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096, 16384])
def test_calls_are_graph_capturable(agx, orc, dev, n):
    """one call captured on a side stream (no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    batch, shape = 5, KEYSWITCH
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    cases = [_case(orc, n, moduli, shape, batch, n * 7 + batch + shape[0]), _case(orc, n, moduli, shape, batch, n + 99)]
    d_xq, d_xp = dev.to_device(cases[0][0]), dev.to_device(cases[0][1])
    d_out, d_s = dev.empty(cases[0][0].size), dev.empty(cases[0][1].size)

    def call(s):
        basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, s)

    graph = capture(dev, call, call)
    for xq, xp, lq, lp, want in cases[::-1]:
        for q_words, p_words in ((xq, xp), (lq, lp)):
            d_xq.copy_(torch.from_numpy(q_words.view(np.int64).copy()))
            d_xp.copy_(torch.from_numpy(p_words.view(np.int64).copy()))
            d_out.zero_()
            graph.replay()
            dev.sync()
            assert np.array_equal(dev.to_host(d_out), want), "replay"
            assert np.array_equal(_run(dev, basis, q_words, p_words, batch), want), "direct call"
    basis.close()
    plan.close()


@pytest.mark.parametrize("n,bits,batch", [(64, 60, 5), (1024, 60, 5), (4096, 60, 5), (4096, 30, 3), (16384, 62, 2), (32768, 61, 2)])
def test_odd_placement_and_guard_bands(agx, orc, dev, n, bits, batch):
    """all four buffers at an odd word of one larger allocation (no frame starts on a 16-byte boundary): the right words, xq and xp unchanged,
    and every word outside d_out and the scratch as it was"""
    shape = KEYSWITCH
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [bits] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(*shape)
    xq, xp, _, _, want = _case(orc, n, moduli, shape, batch, n + bits)
    odd = lambda off: off + 1 - off % 2      # noqa: E731
    lq = Layout(n, T, batch, offset=1)
    lp = Layout(n, S, batch, offset=odd(lq.span() + 5))
    lo = Layout(n, T, batch, offset=odd(lp.span() + 5))
    ls = Layout(n, S, batch, offset=odd(lo.span() + 5))
    assert all(l.offset % 2 == 1 for l in (lq, lp, lo, ls))
    arena = arena_for(dev, n, (lq, xq), (lp, xp), (lo, None), (ls, None))
    basis.mod_down(arena.address(lq.offset), arena.address(lp.offset), arena.address(lo.offset), arena.address(ls.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lq, xq), (lp, xp), (lo, None), (ls, None)], img), "a word outside d_out and the scratch changed"
    assert np.array_equal(arena.frames(lo, img), want)
    basis.close()
    plan.close()


# ---- size ---------------------------------------------------------------------------------------------------------------------------
def _judge_frames(orc, dev, d_xq, d_xp, d_out, src, dst, batch, n, frames):
    """the listed frames (of every target) against Python integers"""
    S, T = len(src), len(dst)
    pick = lambda d, k: dev.to_host(d.view(k, batch, n)[:, frames].contiguous()).reshape(k, -1)      # noqa: E731
    want = mod_down_ntt(orc, n, pick(d_xq, T), pick(d_xp, S), src, dst).reshape(T, len(frames), n)
    got = pick(d_out, T).reshape(T, len(frames), n)
    bad = [(j, frames[f]) for j in range(T) for f in range(len(frames)) if not np.array_equal(got[j, f], want[j, f])]
    assert not bad, ("(target, frame)", bad[:8])


def test_1100_frames_at_4096(agx, orc, dev):
    """1,100 frames, two sources -> three targets: 3,300 workgroups decoded target-fastest; edge frames and a thin sample against Python integers"""
    torch = dev.torch
    n, batch, S, T = 4096, 1100, 2, 3
    moduli = moduli_for(orc.find_prime, n, [60] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(3, S, 0, T)
    assert basis.mod_down_launches() == (2 if _fused_expected(n, 60, S) else 4)
    d_xq, d_xp = device_residues(torch, dev, moduli[:T], batch, n, 3), device_residues(torch, dev, moduli[3:], batch, n, 4)
    d_out, d_s = dev.empty(T * batch * n), dev.empty(S * batch * n)
    d_out.fill_(-1)
    basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    frames = judged_frames(batch, 14)
    _judge_frames(orc, dev, d_xq, d_xp, d_out, moduli[3:], moduli[:T], batch, n, frames)
    basis.close()
    plan.close()


def test_generic_kernel_past_one_grid_stride_trip(agx, orc, dev):
    """n = 32, 140,000 frames: 4,480,000 coefficients per slab, more than one thread each of the element-wise kernels' largest grid (today 16384
    workgroups of 256 threads: a second step from frame 131072 on).  Nothing here depends on that figure: every word of the large call is
    compared with the same call made 1,000 frames at a time, and frames across the whole range, the ends included, with Python integers."""
    torch = dev.torch
    n, batch, chunk, S, T = 32, 140000, 1000, 2, 3
    moduli = moduli_for(orc.find_prime, n, [60] * 5)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    basis = plan.basis(3, S, 0, T)
    assert basis.mod_down_launches() == 4
    d_xq, d_xp = device_residues(torch, dev, moduli[:T], batch, n, 5), device_residues(torch, dev, moduli[3:], batch, n, 6)
    d_out, d_s = dev.empty(T * batch * n), dev.empty(S * batch * n)
    d_out.fill_(-1)
    basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    part_s = dev.empty(S * chunk * n)
    assert_equals_chunked_calls(torch, lambda ins, outs, frames: basis.mod_down(ins[0].data_ptr(), ins[1].data_ptr(), outs[0].data_ptr(), part_s.data_ptr(), frames, dev.stream),
                                [d_xq.view(T, batch, n), d_xp.view(S, batch, n)], [d_out.view(T, batch, n)], batch, chunk)
    frames = judged_frames(batch, 48, extra=range(0, batch, 4999))
    _judge_frames(orc, dev, d_xq, d_xp, d_out, moduli[3:], moduli[:T], batch, n, frames)
    basis.close()
    plan.close()
