"""agx_ntt_rescale on the device: exact division by the plan's last modulus q_L on NTT-form frames.

The expected words come from Python integers, here: X is drawn per coefficient in [0, q_0 ... q_{P-1}), its residues are transformed by
the CPU oracle's forward and handed to the GPU, and the GPU's output must equal, word for word, the oracle's forward of Y mod q_i with
Y = floor(X / q_L) (floor mode) or floor((X + h) / q_L), h = (q_L - 1) / 2 (round mode).  No tolerance anywhere."""
import functools

import numpy as np
import pytest

from gpu_util import (RESCALE_IDS, Layout, arena_for, capture, group_of_two, moduli_for, oracle_tables, plan_for_moduli, registry_entries,
                      status_of)

pytestmark = pytest.mark.gpu

FLOOR, ROUND = 0, 1
MODES = (FLOOR, ROUND)


# ---- the reference: Python integers ---------------------------------------------------------------------------------------------
def _boundary_values(rng, moduli):
    """X with X mod q_L in {0, 1, h-1, h, h+1, q_L-1} under a random quotient, X in {0, Q-1} (Q-1: every residue q_i - 1), and, for every
    prime, X = -1 (mod q_i) under a random cofactor (that residue q_i - 1)"""
    Q = int(np.prod([int(q) for q in moduli], dtype=object))
    qL = moduli[-1]
    h = (qL - 1) // 2
    rest = Q // qL
    out = [0, Q - 1]
    for r in (0, 1, h - 1, h, h + 1, qL - 1):
        out += [_big(rng, rest) * qL + r, (rest - 1) * qL + r, r]
    for q in moduli:
        out.append((_big(rng, Q // q) + 1) * q - 1)
    return out


def _big(rng, bound):
    """a seeded Python integer in [0, bound), bound < 2^256"""
    limbs = rng.integers(0, 1 << 63, size=5, dtype=np.uint64)
    v = 0
    for w in limbs:
        v = (v << 63) | int(w)
    return v % bound


def _draw(rng, moduli, count, boundary_only=False):
    Q = int(np.prod([int(q) for q in moduli], dtype=object))
    special = _boundary_values(rng, moduli)
    if boundary_only:
        return [special[int(i)] for i in rng.integers(0, len(special), size=count)]
    limbs = rng.integers(0, 1 << 63, size=(count, 5), dtype=np.uint64).tolist()
    X = [((((a << 63 | b) << 63 | c) << 63 | d) << 63 | e) % Q for a, b, c, d, e in limbs]
    X[:len(special)] = special[:count]      # frame 0 opens with the boundary values; every frame of a case is compared
    return X


@functools.lru_cache(maxsize=None)
def _case(orc, n, moduli, batch, seed, boundary_only=False):
    """(residues [P][batch][n] in coefficient form, their transform xhat, {mode: expected words [P-1][batch][n]}); computed once per
    case and shared by the tests that need it (treat as read-only)"""
    rng = np.random.default_rng(seed)
    X = _draw(rng, moduli, batch * n, boundary_only)
    qL = moduli[-1]
    h = (qL - 1) // 2
    tabs = [oracle_tables(orc, n, q) for q in moduli]
    res = [np.array([x % q for x in X], dtype=np.uint64) for q in moduli]
    xhat = np.concatenate([orc.forward(r, q, tw, pre, n) for r, (q, _, tw, pre) in zip(res, tabs)])
    want = {}
    for mode in MODES:
        Y = [(x + (h if mode == ROUND else 0)) // qL for x in X]
        want[mode] = np.concatenate([orc.forward(np.array([y % q for y in Y], dtype=np.uint64), q, tw, pre, n) for (q, _, tw, pre) in tabs[:-1]])
    for a in (xhat, *want.values()):
        a.setflags(write=False)
    return np.concatenate(res), xhat, want


def _run(dev, plan, xhat, batch, n, mode, d_x=None):
    """out of place with a scratch of its own; returns the output words"""
    P = plan.num_primes
    d_x = dev.to_device(xhat) if d_x is None else d_x
    d_out, d_s = dev.empty((P - 1) * batch * n), dev.empty(batch * n)
    plan.rescale(d_x.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, mode, dev.stream)
    return dev.to_host(d_out)


def _check_plan(agx, orc, dev, plan, n, moduli, batch, seed, what, boundary_only=False):
    """both modes, from fully reduced inputs and from what forward_lazy of the plan writes"""
    res, xhat, want = _case(orc, n, moduli, batch, seed, boundary_only)
    d_res, d_lazy = dev.to_device(res), dev.empty(res.size)
    plan.forward_lazy(d_res.data_ptr(), d_lazy.data_ptr(), batch, dev.stream)
    for mode in MODES:
        assert np.array_equal(_run(dev, plan, xhat, batch, n, mode), want[mode]), (what, "mode", mode, "reduced inputs")
        assert np.array_equal(_run(dev, plan, None, batch, n, mode, d_x=d_lazy), want[mode]), (what, "mode", mode, "lazy inputs")
    return want


# ---- parity ---------------------------------------------------------------------------------------------------------------------
SIZES = [8, 64, 512, 1024, 4096, 16384, 32768]
PARITY = [(n, 60, P, b) for n in SIZES for P in (2, 4) for b in (1, 5)] + [(n, 30, P, b) for n in (64, 1024, 4096) for P in (2, 4) for b in (1, 5)]


@pytest.mark.parametrize("n,bits,primes,batch", PARITY)
def test_parity_both_modes(agx, orc, dev, n, bits, primes, batch):
    """every kernel family and both inverse forms of the large sizes (60-bit primes: the fused route from n = 1024 on, the generic route
    below; 30-bit plans: the generic route through the 32-bit kernels); batch 5 leaves the last workgroup partly filled wherever a
    workgroup holds more than one frame"""
    moduli = moduli_for(orc.find_prime, n, [bits] * primes)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_plan(agx, orc, dev, plan, n, moduli, batch, n * 13 + bits + primes + batch, (n, bits, primes, batch))
    plan.close()


def _mixed_plans(agx, orc, n):
    """[60, 30, 61]: q_L > 4 q_1; [61, 60, 30]: q_L far below the others; the three largest 62-bit-class primes: the exact-arithmetic entries"""
    return [moduli_for(orc.find_prime, n, [60, 30, 61]), moduli_for(orc.find_prime, n, [61, 60, 30]), tuple(agx.find_primes(62, n, 3))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_mixed_widths(agx, orc, dev, which):
    n, batch = 1024, 3
    moduli = _mixed_plans(agx, orc, n)[which]
    if which == 0:
        assert moduli[2] > 4 * moduli[1]
    if which == 2:
        assert all(q > 1 << 61 for q in moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_plan(agx, orc, dev, plan, n, moduli, batch, 77 + which, ("mixed", moduli))
    plan.close()


@pytest.mark.parametrize("n,spec", [(64, [60, 60, 60]), (1024, [60, 60, 60, 60]), (1024, [62, 62]), (1024, [60, 30, 61]), (1024, [61, 60, 30]),
                                    (4096, [60, 60]), (4096, [30, 30, 30]), (16384, [61, 61]), (32768, [60, 60])])
def test_boundary_coefficients(agx, orc, dev, n, spec):
    """frames made of nothing but boundary values: X mod q_L in {0, 1, h-1, h, h+1, q_L-1}, X in {0, Q-1}, residues q_i - 1"""
    moduli = moduli_for(orc.find_prime, n, spec)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_plan(agx, orc, dev, plan, n, moduli, 2, n + len(spec), ("boundary", n, spec), boundary_only=True)
    plan.close()


@pytest.mark.parametrize("config,n,max_bits", registry_entries(RESCALE_IDS))
def test_every_registry_entry_at_its_own_size(agx, orc, dev, config, n, max_bits):
    """each entry selected explicitly (AGX_VARIANT_REGBLOCK_BASE + id) under the widest modulus it admits, three primes, a ragged batch"""
    batch = 3
    moduli = moduli_for(orc.find_prime, n, [max_bits] * 3)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    _check_plan(agx, orc, dev, plan, n, moduli, batch, config, ("registry id", config))
    plan.close()


@pytest.mark.parametrize("bits", [60, 62])
def test_radix2_plans_take_the_generic_route_and_match_the_fused_one(agx, orc, dev, bits):
    n, batch, primes = 4096, 5, 3
    moduli = moduli_for(orc.find_prime, n, [bits] * primes)
    res, xhat, want = _case(orc, n, moduli, batch, 4096 + bits)
    fused, _ = plan_for_moduli(agx, orc, n, moduli)
    generic, _ = plan_for_moduli(agx, orc, n, moduli)
    generic.set_variant(agx.VARIANT_LDS_RADIX2)
    for mode in MODES:
        a, b = _run(dev, fused, xhat, batch, n, mode), _run(dev, generic, xhat, batch, n, mode)
        assert np.array_equal(a, b), ("fused and generic routes differ", mode)
        assert np.array_equal(b, want[mode]), ("generic route", mode)
    fused.close()
    generic.close()


# ---- aliasing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits,primes,batch", [(64, 60, 3, 5), (1024, 60, 2, 5), (4096, 60, 4, 5), (4096, 30, 3, 3), (4096, 62, 2, 3), (16384, 60, 3, 2), (32768, 61, 2, 2)])
def test_aliasing_and_guard_bands(agx, orc, dev, n, bits, primes, batch):
    """in place (out == x, scratch = x's last slab), out distinct with its own scratch, out distinct with x's last slab as the scratch:
    the same words every time; every word outside out and the scratch keeps its value (x included when the scratch is separate).
    The operands sit at odd element offsets, so no frame starts on a 16-byte boundary."""
    moduli = moduli_for(orc.find_prime, n, [bits] * primes)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, xhat, want = _case(orc, n, moduli, batch, n + bits + primes)
    slab = batch * n
    lx = Layout(n, primes, batch, offset=1)
    lx_head, lx_last = Layout(n, primes - 1, batch, offset=1), Layout(n, 1, batch, offset=1 + (primes - 1) * slab)
    lo = Layout(n, primes - 1, batch, offset=lx.span() + 5)
    ls = Layout(n, 1, batch, offset=lo.span() + 7)
    head = xhat[:(primes - 1) * slab]
    for mode in MODES:
        # out distinct, a scratch of its own: x unchanged
        arena = arena_for(dev, n, (lx, xhat), (lo, None), (ls, None))
        plan.rescale(arena.address(lx.offset), arena.address(lo.offset), arena.address(ls.offset), batch, mode, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx, xhat), (lo, None), (ls, None)], img), "separate scratch: a word outside out and the scratch changed"
        assert np.array_equal(arena.frames(lo, img), want[mode]), ("separate scratch", mode)
        # out distinct, x's last slab as the scratch: slabs 0 .. P-2 of x unchanged
        arena = arena_for(dev, n, (lx, xhat), (lo, None))
        plan.rescale(arena.address(lx.offset), arena.address(lo.offset), arena.address(lx_last.offset), batch, mode, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx_head, head), (lx_last, None), (lo, None)], img), "last slab as scratch: a word outside out and that slab changed"
        assert np.array_equal(arena.frames(lo, img), want[mode]), ("last slab as scratch", mode)
        # in place
        arena = arena_for(dev, n, (lx, xhat))
        plan.rescale(arena.address(lx.offset), arena.address(lx.offset), arena.address(lx_last.offset), batch, mode, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx_head, None), (lx_last, None)], img), "in place: a word outside x changed"
        assert np.array_equal(arena.frames(lx_head, img), want[mode]), ("in place", mode)
        # in place with a scratch of its own: the last slab survives
        arena = arena_for(dev, n, (lx, xhat), (ls, None))
        plan.rescale(arena.address(lx.offset), arena.address(lx.offset), arena.address(ls.offset), batch, mode, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx_head, None), (lx_last, xhat[(primes - 1) * slab:]), (ls, None)], img), "in place, separate scratch"
        assert np.array_equal(arena.frames(lx_head, img), want[mode]), ("in place, separate scratch", mode)
    plan.close()


# ---- rejections -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits", [(64, 60), (4096, 60), (4096, 30)])
def test_rejections_write_nothing(agx, orc, dev, n, bits):
    primes, batch = 3, 2
    moduli = moduli_for(orc.find_prime, n, [bits] * primes)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, xhat, _ = _case(orc, n, moduli, batch, 5 * n + bits)
    slab = batch * n
    lx = Layout(n, primes, batch, offset=0)
    lo = Layout(n, primes - 1, batch, offset=lx.span() + 2 * n)
    ls = Layout(n, 1, batch, offset=lo.span() + 2 * n)
    arena = arena_for(dev, n, (lx, xhat), (lo, None), (ls, None))
    before = arena.image()
    x, out, scr, last = arena.address(0), arena.address(lo.offset), arena.address(ls.offset), arena.address((primes - 1) * slab)
    R, st, w = plan.rescale, dev.stream, 8
    assert status_of(agx, R, x, out, scr, batch, 2, st) == 5 and status_of(agx, R, x, out, scr, batch, -1, st) == 5      # mode
    assert status_of(agx, R, x, x + w * (n // 2), scr, batch, ROUND, st) == 5                  # out partially over x
    assert status_of(agx, R, x, x + w * slab, scr, batch, ROUND, st) == 5                      # out = x one slab later: its slab 0 is x's slab 1
    assert status_of(agx, R, x, last, scr, batch, ROUND, st) == 5                              # out starts on x's last slab
    assert status_of(agx, R, x, out, out, batch, ROUND, st) == 5                               # out touching the scratch
    assert status_of(agx, R, x, out, out + w * ((primes - 1) * slab - n // 2), batch, ROUND, st) == 5
    assert status_of(agx, R, x, out, out - w * (slab - 1), batch, ROUND, st) == 5              # the scratch's last word is out's first
    assert status_of(agx, R, x, last, last, batch, ROUND, st) == 5
    assert status_of(agx, R, x, out, x, batch, ROUND, st) == 5                                 # the scratch on slabs 0 .. P-2 of x
    assert status_of(agx, R, x, out, last - w * (n // 2), batch, ROUND, st) == 5
    assert status_of(agx, R, x, x, x + w * slab, batch, ROUND, st) == 5
    assert status_of(agx, R, x, out, last + w * (n // 2), batch, ROUND, st) == 5               # the scratch over the last slab without being it
    assert status_of(agx, R, x, out, last - w, batch, ROUND, st) == 5
    assert status_of(agx, R, 0, out, scr, batch, ROUND, st) == 1 and status_of(agx, R, x, 0, scr, batch, ROUND, st) == 1
    assert status_of(agx, R, x, out, 0, batch, ROUND, st) == 1
    assert status_of(agx, R, x + 4, out, scr, batch, ROUND, st) == 5 and status_of(agx, R, x, out + 4, scr, batch, ROUND, st) == 5      # uint64_t data
    assert status_of(agx, R, x, out, scr + 4, batch, ROUND, st) == 5
    one, _ = plan_for_moduli(agx, orc, n, moduli[:1])
    assert status_of(agx, one.rescale, x, out, scr, batch, ROUND, st) == 5                     # P == 1
    one.close()
    twice, _ = plan_for_moduli(agx, orc, n, (moduli[0], moduli[1], moduli[0]))                         # q_0 == q_L: the plan exists, the call refuses
    assert status_of(agx, twice.rescale, x, out, scr, batch, ROUND, st) == 3
    assert status_of(agx, twice.rescale, x, out, scr, batch, FLOOR, st) == 3
    twice.close()
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    assert status_of(agx, fwd_only.rescale, x, out, scr, batch, ROUND, st) == 9
    fwd_only.close()
    R(x, out, scr, 0, ROUND, st)      # empty batch: nothing happens
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    plan.close()


# ---- graph capture, groups ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 16384])
def test_calls_are_graph_capturable(agx, orc, dev, n):
    """a floor and a round call captured one after the other on a side stream (no parallel branches), replayed twice on new data"""
    torch = dev.torch
    primes, batch = 3, 5
    moduli = moduli_for(orc.find_prime, n, [60] * primes)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    cases = [_case(orc, n, moduli, batch, n + k) for k in (1, 2)]
    d_x = dev.to_device(cases[0][1])
    d_out = [dev.empty((primes - 1) * batch * n) for _ in MODES]
    d_s = dev.empty(batch * n)

    def both_modes(s):
        for mode in MODES:
            plan.rescale(d_x.data_ptr(), d_out[mode].data_ptr(), d_s.data_ptr(), batch, mode, s)

    graph = capture(dev, lambda s: plan.rescale(d_x.data_ptr(), d_out[0].data_ptr(), d_s.data_ptr(), batch, FLOOR, s), both_modes)
    for _, xhat, want in cases:
        d_x.copy_(torch.from_numpy(xhat.view(np.int64).copy()))
        for d in d_out:
            d.zero_()
        graph.replay()
        dev.sync()
        for mode in MODES:
            assert np.array_equal(dev.to_host(d_out[mode]), want[mode]), ("replay", mode)
            assert np.array_equal(_run(dev, plan, xhat, batch, n, mode), want[mode]), ("eager", mode)
    plan.close()


def test_group_equals_the_single_plan(agx, orc, dev):
    """DeviceGroup.rescale on devices [0, 0]: an odd frame count dealt to two shards, against Plan.rescale on the same words"""
    torch = dev.torch
    n, primes, frames = 4096, 3, 7
    moduli = moduli_for(orc.find_prime, n, [60] * primes)
    grp, plan, batches = group_of_two(agx, orc, n, moduli, frames)
    d_x, d_out, d_s, wants = [], [], [], []
    for i, bt in enumerate(batches):
        _, xhat, want = _case(orc, n, moduli, bt, 900 + i)
        d_x.append(dev.to_device(xhat))
        d_out.append(dev.empty((primes - 1) * bt * n))
        d_s.append(dev.empty(bt * n))
        wants.append(want)
    for mode in MODES:
        single = [_run(dev, plan, None, bt, n, mode, d_x=d_x[i]) for i, bt in enumerate(batches)]
        torch.cuda.synchronize()
        grp.rescale([d.data_ptr() for d in d_x], [d.data_ptr() for d in d_out], [d.data_ptr() for d in d_s], batches, mode)
        grp.synchronize()
        for i in range(2):
            got = dev.to_host(d_out[i])
            assert np.array_equal(got, single[i]), f"shard {i} differs from the single plan"
            assert np.array_equal(got, wants[i][mode]), f"shard {i} differs from the reference"
    grp.close()
    plan.close()
