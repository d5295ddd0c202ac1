"""agx_ntt_basis_quotient, agx_ntt_forward_range and agx_ntt_inverse_range on the device.  The quotient word for word against the Python-integer model
(tests/quotient_ref.py on tests/bfv_conv_ref.py): tiny moduli with every alpha, class-edge moduli on both sides of every capacity step with both centring
edges at a wide m, reduced and lazy inputs; against the six-call composition it replaces, on the same device words, under both variants, with the scratch
apart and with the scratch the operand; odd 8-byte-only placement with guard bands; the creation and call statuses in their order, rejected calls writing
nothing; an empty batch; graph capture; the launch count; the other calls of such a basis against the basis with an auxiliary prime.  The range transforms
against a plan over those primes and against the whole-plan calls, with their rules.  And a whole BFV multiplication on the new listing of
INTEGRATION.md: one plan, two bases, every coefficient decrypted."""
import functools

import numpy as np
import pytest

import bfv_conv_ref as ref
import quotient_ref as qref
from gpu_util import Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, status_of
from modulus_cases import MIXES, edge_moduli, prime_below
from rns_ref import oracle_forward_set, oracle_inverse_set

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
T_SMALL, T_HUGE = 65537, 2**64 - 59
B_COUNTS = (1, 2, 3, 4, 5, 8, 9, 16)      # both sides of every step of the kernel's capacity for the z_j (1, 2, 4, 8, 16)
L_FOR = {1: 16, 2: 5, 3: 16, 4: 9, 5: 4, 8: 8, 9: 2, 16: 3}      # the Q count that goes with each: both sides of the same steps, up to 16, within 20 moduli


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _ranges(moduli, shape):
    """(Q, B, m) of shape = (b_first, K, q_first, L, aux_prime), the arguments of Plan.basis_quotient without t"""
    bf, K, qf, L, aux = shape
    return tuple(moduli[qf:qf + L]), tuple(moduli[bf:bf + K]), moduli[aux]


@functools.lru_cache(maxsize=None)
def _case(orc, Q, B, m, t, batch, n, seed, wanted):
    """d_x [L + K + 1][batch n] in NTT form, reduced and spread over the lazy range, from coefficient rows whose auxiliary row is built for the wanted
    alphas; the model's d_out; the model's alphas"""
    rng = np.random.default_rng(seed)
    every = Q + B + (m,)
    rows = qref.rows_with_alphas(rng, Q, B, m, t, batch * n, wanted)
    x = oracle_forward_set(orc, n, every, _u64(rows))
    lazy = x + _u64([[int(k) * q for k in rng.integers(0, 4, size=batch * n)] for q in every])
    out = {"x": x.reshape(-1), "lazy_x": lazy.reshape(-1), "out": oracle_forward_set(orc, n, Q, _u64(qref.quotient(rows, Q, B, m, t))).reshape(-1),
           "alphas": tuple(qref.alphas(rows, Q, B, m, t))}
    for a in (out["x"], out["lazy_x"], out["out"]):
        a.setflags(write=False)
    return out


def _quotient(dev, basis, x, words, out_words, batch, in_place=False):
    """(d_out, d_x afterwards) of one call; the scratch apart, or the operand itself"""
    d_x, d_out = dev.to_device(x), dev.to_device(canary(0, out_words))
    d_scratch = d_x if in_place else dev.to_device(canary(7, words))
    basis.quotient(d_x.data_ptr(), d_out.data_ptr(), d_scratch.data_ptr(), batch, dev.stream)
    return dev.to_host(d_out), dev.to_host(d_x)


def _check(dev, orc, plan, shape, t, batch, seed, wanted, what):
    n = plan.n
    bf, K, qf, L, aux = shape
    Q, B, m = _ranges(plan.moduli, shape)
    case = _case(orc, Q, B, m, t, batch, n, seed, wanted)
    basis = plan.basis_quotient(*shape, t)
    assert basis.quotient_info()[:2] == (True, t) and basis.aux_info()[:2] == (True, aux) and basis.info()[:4] == (bf, K, qf, L)
    words = (L + K + 1) * batch * n
    for name in ("x", "lazy_x"):
        for in_place in (False, True):
            got, after = _quotient(dev, basis, case[name], words, L * batch * n, batch, in_place)
            bad = np.flatnonzero(got != case["out"])
            assert bad.size == 0, (what, name, in_place, "first differing words", bad[:4].tolist(), got[bad[:4]].tolist(), case["out"][bad[:4]].tolist())
            assert in_place or np.array_equal(after, case[name]), (what, name, "d_x changed")
    basis.close()
    return case


def _plan(agx, orc, n, moduli, inverse=True):
    return plan_for_moduli(agx, orc, n, moduli, inverse)[0]


@functools.lru_cache(maxsize=None)
def _edge_list(orc, n):
    moduli = tuple(dict.fromkeys(edge_moduli(orc, n).values()))
    assert len(moduli) >= 20 and max(moduli) > 1 << 61 and min(moduli) < 1 << 30
    return moduli


# ---- word for word against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,shape", [("m first", (1, 2, 3, 3, 0)), ("m first", (4, 3, 1, 3, 0)), ("m first", (1, 5, 6, 1, 0)), ("m first", (6, 1, 1, 5, 0)),
                                         ("m behind B", (0, 2, 3, 4, 2)), ("m behind B", (1, 1, 3, 2, 2))], ids=str)
def test_tiny_moduli_every_alpha(agx, orc, dev, order, shape):
    """n = 8, batch 6, the six smallest admitted primes (17, 97, 113, 193, 241, 257) and one below 400, m = 17: every alpha in [-8, 8] occurs"""
    n = 8
    moduli = tuple(MIXES(orc, n)["tiny"]) + (prime_below(orc, 400, n),)
    assert moduli[0] == 17 and len(set(moduli)) == 7
    if order == "m behind B":
        moduli = moduli[1:3] + moduli[:1] + moduli[3:]
    assert moduli[shape[4]] == 17
    plan = _plan(agx, orc, n, moduli)
    case = _check(dev, orc, plan, shape, T_SMALL, 6, 8 + sum(shape), tuple(range(-8, 9)), ("tiny", order, shape))
    assert set(case["alphas"]) == set(range(-8, 9))
    plan.close()


@pytest.mark.parametrize("K", B_COUNTS)
def test_class_edge_moduli_on_both_sides_of_every_capacity_step(agx, orc, dev, K):
    """n = 64, batch 3, the class-edge moduli of modulus_cases.py: narrow and 62-bit moduli meet in B and in Q, m is a wide prime right behind B, and the
    auxiliary coefficients are built so that both centring edges +-(m - 1) / 2 occur"""
    n, L = 64, L_FOR[K]
    edges = _edge_list(orc, n)
    r = next(r for r in range(len(edges)) if edges[(r + K) % len(edges)] > 1 << 59)      # rotate until m is wide
    moduli = tuple(edges[(r + k) % len(edges)] for k in range(K + 1 + L))
    m = moduli[K]
    half = (m - 1) // 2
    wanted = (half, -half, 0, None, 1, -1, half - 1, -half + 1, None, None)
    plan = _plan(agx, orc, n, moduli)
    case = _check(dev, orc, plan, (0, K, K + 1, L, K), T_HUGE if K % 2 else T_SMALL, 3, 64 * K + L, wanted, ("edges", K, L))
    assert {half, -half, 0} <= set(case["alphas"])
    plan.close()
    if K == 2:      # Q in front of B with m behind it; and m in front of both, away from B: one more inverse launch
        for moduli, shape in ((moduli[K + 1:] + moduli[:K + 1], (L, K, 0, L, L + K)), (moduli[K:K + 1] + moduli[K + 1:] + moduli[:K], (1 + L, K, 1, L, 0))):
            plan = _plan(agx, orc, n, moduli)
            assert moduli[shape[4]] == m
            case = _check(dev, orc, plan, shape, T_SMALL, 3, 9 + shape[0], wanted, ("edges, other orders", shape))
            assert {half, -half} <= set(case["alphas"])
            plan.close()


# ---- against the six calls it replaces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radix2", [False, True], ids=["auto", "lds_radix2"])
def test_against_the_six_call_composition(agx, orc, dev, radix2):
    """n = 1024, batch 3, L = 2, K = 3: mul_add_galois by a frame of t's, mod_down on the fast-floor basis, the inverse on Bsk through a second plan,
    extend_exact to NTT form -- on the same device words; and both against the model"""
    n, batch, L, K, t = 1024, 3, 2, 3, T_SMALL
    W, slab, st = L + K + 1, batch * n, dev.stream
    moduli = moduli_for(orc.find_prime, n, [45, 52, 60, 57, 54, 59])
    Q, Bsk = moduli[:L], moduli[L:]
    plan, plan_bsk = _plan(agx, orc, n, moduli), _plan(agx, orc, n, Bsk)
    if radix2:
        plan.set_variant(agx.VARIANT_LDS_RADIX2), plan_bsk.set_variant(agx.VARIANT_LDS_RADIX2)
    rng = np.random.default_rng(n + radix2)
    x = np.stack([rng.integers(0, 4 * q, size=slab, dtype=np.uint64) for q in moduli]).reshape(-1)      # any words are NTT-form words
    # the old listing, steps 4 to 7
    fast_floor, to_q = plan.basis(0, L, L, K + 1), plan.basis_aux(L, K, 0, L, L + K)
    d, d_t = dev.to_device(x), dev.to_device(np.full(W * n, t, dtype=np.uint64))
    d_floor, d_floor_coeff, d_want = dev.empty((K + 1) * slab), dev.empty((K + 1) * slab), dev.empty(L * slab)
    p = d.data_ptr()
    plan.mul_add_galois(d_t.data_ptr(), p, p, batch, 1, 1, False, 0, W, st)
    fast_floor.mod_down(p + 8 * L * slab, p, d_floor.data_ptr(), p, batch, st)
    plan_bsk.inverse(d_floor.data_ptr(), d_floor_coeff.data_ptr(), batch, st)
    to_q.extend_exact(d_floor_coeff.data_ptr(), d_floor_coeff.data_ptr() + 8 * K * slab, d_want.data_ptr(), batch, NTT, st)
    want = dev.to_host(d_want)
    rows = oracle_inverse_set(orc, n, moduli, x.reshape(W, -1)).tolist()
    assert np.array_equal(want, oracle_forward_set(orc, n, Q, _u64(qref.quotient(rows, Q, moduli[L:L + K], moduli[L + K], t))).reshape(-1)), "the composition is not the model"
    basis = plan.basis_quotient(L, K, 0, L, L + K, t)
    for in_place in (False, True):
        got, after = _quotient(dev, basis, x, W * slab, L * slab, batch, in_place)
        assert np.array_equal(got, want), ("quotient against the composition", in_place)
        assert in_place or np.array_equal(after, x), "d_x changed"
    for h in (fast_floor, to_q, basis, plan_bsk, plan):
        h.close()


# ---- placement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5])
def test_odd_placement_and_guard_bands(agx, orc, dev, K):
    """every buffer at an odd word of one larger allocation (8-byte alignment only): the right words, d_x unchanged, and every word outside d_out and the
    scratch as it was; then with the scratch the operand"""
    n, batch, L = 64, 3, 3
    moduli = _edge_list(orc, n)[2:2 + K + 1 + L]
    shape = (0, K, K + 1, L, K)
    plan = _plan(agx, orc, n, moduli)
    Q, B, m = _ranges(plan.moduli, shape)
    case = _case(orc, Q, B, m, T_SMALL, batch, n, 11 + K, (None,))
    basis = plan.basis_quotient(*shape, T_SMALL)
    W = L + K + 1
    lx = Layout(n, W, batch, offset=1)
    ls = Layout(n, W, batch, offset=lx.span() + 6)
    lo = Layout(n, L, batch, offset=ls.span() + 4)
    assert lx.offset % 2 == 1 and ls.offset % 2 == 1 and lo.offset % 2 == 1
    arena = arena_for(dev, n, (lx, case["lazy_x"]), (ls, None), (lo, None))
    basis.quotient(arena.address(lx.offset), arena.address(lo.offset), arena.address(ls.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lx, case["lazy_x"]), (ls, None), (lo, None)], img), "a word outside d_out and the scratch changed"
    assert np.array_equal(arena.frames(lo, img), case["out"])
    arena = arena_for(dev, n, (lx, case["lazy_x"]), (lo, None))
    basis.quotient(arena.address(lx.offset), arena.address(lo.offset), arena.address(lx.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lx, None), (lo, None)], img), "a word outside d_out and d_x changed"
    assert np.array_equal(arena.frames(lo, img), case["out"])
    basis.close()
    plan.close()


# ---- argument rules ------------------------------------------------------------------------------------------------------------------------
def test_creation_statuses(agx, orc, dev):
    n = 64
    a, b, c, d, e = moduli_for(orc.find_prime, n, [60, 60, 45, 30, 54])
    plan = _plan(agx, orc, n, (a, b, c, d, e), inverse=False)      # creation needs no inverse tables
    C = agx.Basis.with_quotient
    t = T_SMALL
    assert status_of(agx, C, plan, 0, 0, 1, 1, 3, t) == 5 and status_of(agx, C, plan, 0, 1, 1, 0, 3, t) == 5 and status_of(agx, C, plan, 4, 2, 0, 1, 2, t) == 5      # create's rules
    assert status_of(agx, C, plan, 0, 1, 1, 2, 5, t) == 5 and status_of(agx, C, plan, 0, 2, 2, 1, 1, t) == 5 and status_of(agx, C, plan, 0, 1, 1, 2, 2, t) == 5      # create_aux's
    assert status_of(agx, C, plan, 0, 2, 1, 2, 4, t) == 5 and status_of(agx, C, plan, 1, 2, 0, 2, 4, t) == 5 and status_of(agx, C, plan, 0, 3, 1, 1, 4, t) == 5      # overlap
    assert status_of(agx, C, plan, 0, 1, 1, 2, 3, 0) == 5      # t = 0
    for args in ((0, 1, 1, 2, 3), (1, 2, 3, 1, 0), (3, 1, 0, 3, 4), (2, 2, 0, 2, 4)):
        for tt in (1, 2, t, T_HUGE, a, d):      # any t but 0, a modulus of the plan included
            basis = C(plan, *args, tt)
            assert basis.quotient_info()[:2] == (True, tt) and basis.aux_info()[:2] == (True, args[4]) and basis.info()[:4] == args[:4]
            basis.close()
    for other in (plan.basis(0, 1, 1, 2), plan.basis(0, 1, 1, 2, 65537), plan.basis_aux(0, 1, 1, 2, 3)):
        assert other.quotient_info()[:2] == (False, 0)
        other.close()
    plan.close()
    twice = _plan(agx, orc, n, (a, b, a, c, d), inverse=False)
    assert status_of(agx, C, twice, 0, 3, 3, 1, 4, t) == 3      # two equal moduli in B: create's rule
    assert status_of(agx, C, twice, 0, 1, 3, 1, 2, t) == 3      # m is B's modulus: create_aux's rule
    assert status_of(agx, C, twice, 3, 1, 0, 3, 4, t) == 3      # two equal moduli in Q
    assert status_of(agx, C, twice, 2, 1, 0, 2, 4, t) == 3      # a modulus of Q is one of B
    assert status_of(agx, C, twice, 0, 2, 1, 2, 4, 0) == 5      # overlap is judged before the moduli and before t
    assert status_of(agx, C, twice, 2, 1, 0, 2, 4, 0) == 3      # the moduli before t
    C(twice, 1, 1, 3, 2, 0, t).close()                          # the repeated modulus as m and in neither range: fine
    twice.close()
    many = _plan(agx, orc, n, _edge_list(orc, n)[:19], inverse=False)
    assert status_of(agx, C, many, 17, 1, 0, 17, 18, t) == 5    # more than 16 primes in Q
    C(many, 16, 1, 0, 16, 17, t).close()
    many.close()


def test_status_rules_in_order_and_rejected_calls_write_nothing(agx, orc, dev):
    n, batch, shape, t = 64, 2, (2, 3, 0, 2, 5), T_SMALL
    K, L = shape[1], shape[3]
    W = L + K + 1
    moduli = moduli_for(orc.find_prime, n, [45, 52, 60, 57, 54, 59])
    plan, forward_only = _plan(agx, orc, n, moduli), _plan(agx, orc, n, moduli, inverse=False)
    Q, B, m = _ranges(plan.moduli, shape)
    case = _case(orc, Q, B, m, t, batch, n, 77, (None,))
    basis, aux, lame = plan.basis_quotient(*shape, t), plan.basis_aux(*shape), forward_only.basis_quotient(*shape, t)
    slab, w, st = batch * n, 8, dev.stream
    lx = Layout(n, W, batch, offset=0)
    ls = Layout(n, W, batch, offset=W * slab)                  # the scratch right behind d_x, d_out right behind the scratch: they meet end to end
    lo = Layout(n, L, batch, offset=2 * W * slab)
    far = Layout(n, L, batch, offset=2 * W * slab + L * slab + 2 * n)
    arena = arena_for(dev, n, (lx, case["x"]), (ls, None), (lo, None), (far, None))
    before = arena.image()
    px, ps, po, pf = (arena.address(l.offset) for l in (lx, ls, lo, far))
    Qt = basis.quotient
    assert [status_of(agx, Qt, *a, batch, st) for a in ((0, po, ps), (px, 0, ps), (px, po, 0))] == [1, 1, 1]                   # NULL
    assert status_of(agx, aux.quotient, px, 0, ps, batch, st) == 1 and status_of(agx, aux.quotient, px, po, ps, batch, st) == 5      # then a basis without the constants
    assert status_of(agx, aux.quotient, px + 4, po, ps, batch, st) == 5
    assert [status_of(agx, Qt, *a, batch, st) for a in ((px + 4, po, ps), (px, po + 4, ps), (px, po, ps + 4))] == [5, 5, 5]      # uint64_t data
    assert status_of(agx, Qt, px, po, ps, (1 << 64) - 1, st) == 5 and status_of(agx, Qt, px, po, ps, 1 << 40, st) == 5         # a batch past the grid limit
    for scratch in (px + w, px + w * (n // 2), px + w * (W * slab - 1), px - w * (W * slab - 1)):      # a scratch that straddles d_x: not d_x itself, not apart
        assert status_of(agx, Qt, px, pf, scratch, batch, st) == 5
    for out in (px, px + w * (n // 2), px + w * (W * slab - 1), ps, ps + w * (W * slab - 1), px - w * (L * slab - 1) + w * W * slab):      # d_out touches d_x or the scratch
        assert status_of(agx, Qt, px, out, ps, batch, st) == 5
    assert status_of(agx, Qt, px, px + w * slab, px, batch, st) == 5      # ... also where the scratch is d_x
    # a plan without inverse tables: behind the argument rules, in front of the empty batch
    assert status_of(agx, lame.quotient, px + 4, po, ps, batch, st) == 5 and status_of(agx, lame.quotient, px, px, ps, batch, st) == 5
    assert status_of(agx, lame.quotient, px, po, ps, batch, st) == 9 and status_of(agx, lame.quotient, px, po, ps, 0, st) == 9
    Qt(px, po, ps, 0, st)      # an empty batch: nothing launched
    Qt(px, po, px, 0, st)
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # allowed: ranges that meet end to end
    Qt(px, po, ps, batch, st)
    img = arena.image()
    assert np.array_equal(arena.frames(lo, img), case["out"]) and np.array_equal(arena.frames(lx, img), case["x"])
    assert not arena.faults([(lx, case["x"]), (ls, None), (lo, None), (far, None)], img)
    for h in (basis, aux, lame, plan, forward_only):
        h.close()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_the_call_is_graph_capturable(agx, orc, dev, n):
    """captured on a side stream with the scratch apart and then with the scratch the operand of a second buffer, replayed on fresh inputs: the eager result"""
    torch = dev.torch
    batch, shape, t = 3, (2, 3, 0, 2, 5), T_SMALL
    K, L = shape[1], shape[3]
    W = L + K + 1
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan = _plan(agx, orc, n, moduli)
    basis = plan.basis_quotient(*shape, t)
    rng = np.random.default_rng(n)
    inputs = [np.stack([rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64) for q in moduli]).reshape(-1) for _ in range(2)]
    d_x, d_y, d_scratch = dev.to_device(inputs[0]), dev.to_device(inputs[0]), dev.empty(W * batch * n)
    d_out = [dev.empty(L * batch * n) for _ in range(2)]

    def both(s):
        basis.quotient(d_x.data_ptr(), d_out[0].data_ptr(), d_scratch.data_ptr(), batch, s)
        basis.quotient(d_y.data_ptr(), d_out[1].data_ptr(), d_y.data_ptr(), batch, s)

    graph = capture(dev, both, both)
    for x in inputs[::-1]:
        for d in (d_x, d_y):
            d.copy_(torch.from_numpy(x.view(np.int64).copy()))
        for d in d_out:
            d.zero_()
        graph.replay()
        dev.sync()
        want, _ = _quotient(dev, basis, x, W * batch * n, L * batch * n, batch)
        assert np.array_equal(dev.to_host(d_out[0]), want) and np.array_equal(dev.to_host(d_out[1]), want), n
        assert np.array_equal(dev.to_host(d_x), x)
        if n == 64:
            Q, B, m = _ranges(plan.moduli, shape)
            rows = oracle_inverse_set(orc, n, Q + B + (m,), x.reshape(W, -1)).tolist()
            assert np.array_equal(want, oracle_forward_set(orc, n, Q, _u64(qref.quotient(rows, Q, B, m, t))).reshape(-1))
    basis.close()
    plan.close()


# ---- the launch count ----------------------------------------------------------------------------------------------------------------------
def test_launch_count_is_two_inverses_the_kernel_and_the_forward(agx, orc, dev):
    """2 x inverse + 1 + forward where m stands right behind B, one inverse more where it does not, under the current variant.  The plan's own counts come
    from the calls that already report them: aux_info is 1 + forward; mod_down_info is inverse + 1 on the two-launch route and 2 x inverse + 1 + forward
    on the generic one.  A registry entry is one launch (pinned here at n = 1024 and 4096: four launches in all); the LDS radix-2 kernels take one, two
    at n = 32768 (seven in all)."""
    for n, bits in [(8, 60), (64, 60), (1024, 60), (4096, 60), (32768, 60), (1024, 30)]:
        plan = _plan(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 6))
        near, away = plan.basis_quotient(2, 2, 0, 2, 4, T_SMALL), plan.basis_quotient(2, 2, 0, 2, 5, T_SMALL)
        for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_AUTO):
            plan.set_variant(variant)
            fwd, down = near.aux_info()[2] - 1, near.mod_down_launches()
            inv = down - 1 if down <= 3 else (down - 1 - fwd) // 2
            assert fwd in (1, 2) and inv in (1, 2), (n, bits, variant, fwd, down)
            if variant == agx.VARIANT_LDS_RADIX2:
                assert (fwd, inv) == ((1, 1) if n <= 16384 else (2, 2)), (n, fwd, inv)
            elif n in (1024, 4096):
                assert (fwd, inv) == (1, 1), (n, bits, fwd, inv)
            assert near.quotient_info() == (True, T_SMALL, 2 * inv + 1 + fwd), (n, bits, variant)
            assert away.quotient_info() == (True, T_SMALL, 3 * inv + 1 + fwd), (n, bits, variant)
        near.close(), away.close()
        plan.close()


# ---- the other calls of such a basis -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_the_other_calls_equal_the_basis_with_an_auxiliary_prime_word_for_word(agx, orc, dev, n):
    batch, shape = 3, (3, 2, 0, 3, 5)
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54, 61, 59])
    plan = _plan(agx, orc, n, moduli)
    quot, aux = plan.basis_quotient(*shape, T_HUGE), plan.basis_aux(*shape)
    assert quot.info() == aux.info() and quot.aux_info() == aux.aux_info() and quot.mod_down_launches() == aux.mod_down_launches()
    rng = np.random.default_rng(n)
    xp = np.stack([rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64) for q in moduli[3:5]]).reshape(-1)
    xq = np.stack([rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64) for q in moduli[0:3]]).reshape(-1)
    r = rng.integers(0, 4 * moduli[5], size=batch * n, dtype=np.uint64)
    d_xp, d_xq, d_r = dev.to_device(xp), dev.to_device(xq), dev.to_device(r)

    def pair(call):
        outs = []
        for basis in (quot, aux):
            d_out = dev.to_device(canary(0, T * batch * n))
            call(basis, d_out)
            outs.append(dev.to_host(d_out))
        return outs

    for form in (COEFF, NTT):
        assert np.array_equal(*pair(lambda b, o: b.extend(d_xp.data_ptr(), o.data_ptr(), batch, form, dev.stream))), ("extend", form)
        assert np.array_equal(*pair(lambda b, o: b.extend_exact(d_xp.data_ptr(), d_r.data_ptr(), o.data_ptr(), batch, form, dev.stream))), ("extend_exact", form)
        assert np.array_equal(*pair(lambda b, o: b.extend_mont(d_xp.data_ptr(), o.data_ptr(), batch, form, dev.stream))), ("extend_mont", form)
    for mode in (agx.RESCALE_FLOOR, agx.RESCALE_ROUND):
        d_scratch = dev.empty(S * batch * n)
        assert np.array_equal(*pair(lambda b, o: b.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), o.data_ptr(), d_scratch.data_ptr(), batch, dev.stream, mode))), ("mod_down", mode)
    quot.close(), aux.close()
    plan.close()


# ---- transforms on a range of the plan's primes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radix2", [False, True], ids=["auto", "lds_radix2"])
@pytest.mark.parametrize("n", [64, 1024])
def test_range_transforms_are_a_plan_over_those_primes(agx, orc, dev, n, radix2):
    batch, st = 3, dev.stream
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54, 61])
    P = len(moduli)
    plan = _plan(agx, orc, n, moduli)
    if radix2:
        plan.set_variant(agx.VARIANT_LDS_RADIX2)
    rng = np.random.default_rng(n)
    for first, count in ((0, 2), (1, 3), (3, 2), (4, 1), (0, P)):      # front, middle, end, the last prime alone, the whole plan
        sub = _plan(agx, orc, n, moduli[first:first + count])
        if radix2:
            sub.set_variant(agx.VARIANT_LDS_RADIX2)
        assert all(sub.psi(k) == plan.psi(first + k) for k in range(count))
        x = np.stack([rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64) for q in moduli[first:first + count]]).reshape(-1)
        for name in ("forward", "inverse"):
            d_in, d_want = dev.to_device(x), dev.empty(x.size)
            getattr(sub, name)(d_in.data_ptr(), d_want.data_ptr(), batch, st)
            want = dev.to_host(d_want)
            d_out = dev.to_device(canary(0, x.size))
            getattr(plan, name + "_range")(d_in.data_ptr(), d_out.data_ptr(), batch, first, count, st)
            assert np.array_equal(dev.to_host(d_out), want) and np.array_equal(dev.to_host(d_in), x), (name, first, count, "out of place")
            getattr(plan, name + "_range")(d_in.data_ptr(), d_in.data_ptr(), batch, first, count, st)
            assert np.array_equal(dev.to_host(d_in), want), (name, first, count, "in place")
            if count == P:
                d_whole = dev.to_device(x)
                getattr(plan, name)(d_whole.data_ptr(), d_whole.data_ptr(), batch, st)
                assert np.array_equal(dev.to_host(d_whole), want), (name, "the whole-plan call")
        want = oracle_forward_set(orc, n, moduli[first:first + count], x.reshape(count, -1) % _u64(moduli[first:first + count])[:, None]).reshape(-1)
        d_in = dev.to_device(x)
        plan.forward_range(d_in.data_ptr(), d_in.data_ptr(), batch, first, count, st)
        assert np.array_equal(dev.to_host(d_in), want), (first, count, "against the oracle")
        sub.close()
    plan.close()


def test_range_transform_rules(agx, orc, dev):
    n, batch, st, w = 64, 2, dev.stream, 8
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54])
    plan, forward_only = _plan(agx, orc, n, moduli), _plan(agx, orc, n, moduli, inverse=False)
    slab = batch * n
    lin = Layout(n, 2, batch, offset=0)
    lout = Layout(n, 2, batch, offset=2 * slab)      # right behind the input: they meet end to end
    x = np.stack([np.random.default_rng(3).integers(0, q, size=slab, dtype=np.uint64) for q in moduli[1:3]]).reshape(-1)
    arena = arena_for(dev, n, (lin, x), (lout, None))
    before = arena.image()
    pi, po = arena.address(0), arena.address(lout.offset)
    for call in (plan.forward_range, plan.inverse_range):
        assert status_of(agx, call, 0, po, batch, 1, 2, st) == 1 and status_of(agx, call, pi, 0, batch, 1, 2, st) == 1 and status_of(agx, call, 0, 0, batch, 9, 0, st) == 1
        for first, count in ((0, 0), (1, 0), (4, 1), (3, 2), (0, 5), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF)):      # the range rule
            assert status_of(agx, call, pi, po, batch, first, count, st) == 5, (first, count)
        assert status_of(agx, call, pi + 4, po, batch, 1, 2, st) == 5 and status_of(agx, call, pi, po + 4, batch, 1, 2, st) == 5      # uint64_t data
        assert status_of(agx, call, pi, po, (1 << 64) - 1, 1, 2, st) == 5      # a batch past the grid limit
        for out in (pi + w, pi + w * (n // 2), pi + w * (2 * slab - 1)):      # an output that straddles the input
            assert status_of(agx, call, pi, out, batch, 1, 2, st) == 5
        call(pi, po, 0, 1, 2, st)      # an empty batch
    assert status_of(agx, forward_only.inverse_range, pi, po, batch, 1, 2, st) == 9 and status_of(agx, forward_only.inverse_range, pi, po, batch, 1, 9, st) == 5
    assert status_of(agx, forward_only.inverse_range, pi, po, 0, 1, 2, st) == 9
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    forward_only.forward_range(pi, po, batch, 1, 2, st)
    img = arena.image()
    assert np.array_equal(arena.frames(lout, img), oracle_forward_set(orc, n, moduli[1:3], x).reshape(-1)) and not arena.faults([(lin, x), (lout, None)], img)
    plan.close(), forward_only.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_a_bfv_multiplication_on_the_new_listing_decrypts(agx, orc, dev):
    """The INTEGRATION.md listing on inverse_range, extend_mont, tensor and quotient at n = 64, batch 2, with the parameters of
    test_a_bfv_multiplication_on_library_calls_decrypts: ONE plan, two bases.  Every coefficient of both frames decrypts to m1 m2 mod t, and d_out is
    the oracle's forward of the model's "out"."""
    n, batch = 64, 2
    w = ref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    B = tuple(prime_below(orc, 1 << b, n) for b in w["B"])
    m_sk, m_tilde, t = prime_below(orc, 1 << w["m_sk"], n), prime_below(orc, 1 << w["m_tilde"], n), ref.BFV_T
    L, K = len(Q), len(B)
    Bsk, W = B + (m_sk,), L + K + 1
    moduli = Q + Bsk + (m_tilde,)      # Q = [0, L), B = [L, L + K), m_sk = L + K, m~ = L + K + 1
    rng = ref.Rng(2016)
    s = ref.keygen(rng, n)
    msgs = [[[rng.below(t) for _ in range(n)] for _ in range(2)] for _ in range(batch)]
    cts = [[ref.encrypt(rng, msg, s, Q, t) for msg in pair] for pair in msgs]      # [frame][operand][component][L][n]
    model = [ref.multiply(pair[0], pair[1], Q, B, m_sk, m_tilde, t) for pair in cts]
    plan = _plan(agx, orc, n, moduli)
    slab, st = batch * n, dev.stream
    ops = np.zeros((2, 2, W, batch, n), dtype=np.uint64)
    for o in range(2):
        for c in range(2):
            coeff = _u64([[cts[f][o][c][j] for f in range(batch)] for j in range(L)])      # [L][batch][n]
            ops[o, c, :L] = oracle_forward_set(orc, n, Q, coeff).reshape(L, batch, n)
    d_ops = [dev.to_device(ops[o].reshape(-1)) for o in range(2)]
    at = lambda d, words: d.data_ptr() + 8 * words      # noqa: E731
    to_bsk = plan.basis_aux(0, L, L, K + 1, L + K + 1)
    divide = plan.basis_quotient(L, K, 0, L, L + K, t)
    assert divide.quotient_info()[:2] == (True, t)
    d_coeff = dev.empty(L * slab)
    for o in range(2):
        for c in range(2):
            plan.inverse_range(at(d_ops[o], c * W * slab), d_coeff.data_ptr(), batch, 0, L, st)                                 # 1
            to_bsk.extend_mont(d_coeff.data_ptr(), at(d_ops[o], (c * W + L) * slab), batch, NTT, st)                           # 2
    d_tensor, d_out = dev.empty(3 * W * slab), dev.empty(3 * L * slab)
    plan.tensor(d_ops[0].data_ptr(), d_ops[1].data_ptr(), d_tensor.data_ptr(), batch, 0, W, st)                                # 3
    for k in range(3):
        d = at(d_tensor, k * W * slab)
        divide.quotient(d, at(d_out, k * L * slab), d, batch, st)                                                              # 4 to 7: the component is given up
    out = dev.to_host(d_out).reshape(3, L, batch, n)
    for k in range(3):
        want = _u64([[model[f]["out"][k][j] for f in range(batch)] for j in range(L)])
        assert np.array_equal(out[k], oracle_forward_set(orc, n, Q, want).reshape(L, batch, n)), ("component", k)
    for f in range(batch):
        coeff = [oracle_inverse_set(orc, n, Q, out[k][:, f]).tolist() for k in range(3)]
        assert ref.decrypt(coeff, s, Q, t) == ref.negacyclic(msgs[f][0], msgs[f][1], t), ("frame", f)
    for h in (to_bsk, divide, plan):
        h.close()
