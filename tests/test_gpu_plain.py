"""agx_ntt_plain_scale_up, _lift and _scale_down on the device, word for word against the Python-integer model (tests/plain_ref.py): tiny moduli with every
centring edge and both signs of h - rho; class-edge moduli on both sides of every capacity step; the generic and the register-blocked inverse under both
variants, a plan of narrow moduli, reduced and lazy inputs, the scratch apart and the scratch the operand; AGX_FORM_NTT against agx_ntt_forward_range of the
coefficient form; odd 8-byte-only placement with guard bands; the creation and call statuses in their order, rejected calls writing nothing; the launch
counts; graph capture; and BFV end to end on the listing of INTEGRATION.md: encryption from scale_up, a multiplication, decryption by inner_product and
scale_down, add-plain and multiply-plain."""
import functools

import numpy as np
import pytest

import bfv_conv_ref as ref
import plain_ref as pref
from gpu_util import Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, status_of
from modulus_cases import MIXES, edge_moduli, prime_below
from rns_ref import oracle_forward_set, oracle_inverse_set

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
T_ODD61 = (1 << 61) - 1
Q_COUNTS = (1, 2, 3, 4, 5, 8, 9, 16)      # both sides of every step of the scale-down kernel's capacity (1, 2, 4, 8, 16)


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _plan(agx, orc, n, moduli, inverse=True):
    return plan_for_moduli(agx, orc, n, moduli, inverse)[0]


@functools.lru_cache(maxsize=None)
def _edge_list(orc, n):
    moduli = tuple(dict.fromkeys(edge_moduli(orc, n).values()))
    assert len(moduli) >= 20 and max(moduli) > 1 << 61 and min(moduli) < 1 << 30
    return moduli


def _messages(rng, t, count):
    """`count` plaintext words: the words next to every sign change of h - rho and of the centred lift, words past t, any 64-bit words"""
    fixed = [0, 1, t - 1, t, t + 1, t // 2, t // 2 + 1, (t + 1) // 2, (t + 1) // 2 - 1, 2**64 - 1, 2**63, 2**64 - t]
    assert count >= len(fixed)
    m = rng.integers(0, 2**64, size=count, dtype=np.uint64)
    m[-len(fixed):] = _u64(fixed)
    return m


@functools.lru_cache(maxsize=None)
def _case(orc, Q, gamma, t, batch, n, seed):
    """one shape's inputs and the model's outputs, computed once and read-only: m and its scale_up / lift in both forms; coefficient rows, their NTT form
    reduced and spread over the lazy range, and the model's scale_down"""
    rng = np.random.default_rng(seed)
    count, L = batch * n, len(Q)
    m = _messages(rng, t, count)
    out = {"m": m}
    for name, fn in (("up", pref.scale_up), ("lift", pref.lift)):
        coeff = _u64(fn(m.tolist(), Q, t))
        out[name + "_coeff"], out[name + "_ntt"] = coeff.reshape(-1), oracle_forward_set(orc, n, Q, coeff).reshape(-1)
    rows = _u64([[0, q - 1, 1] + [int(v) for v in rng.integers(0, q, size=count - 3, dtype=np.uint64)] for q in Q])
    x = oracle_forward_set(orc, n, Q, rows)
    lazy = x + _u64([[int(k) * q for k in rng.integers(0, 4, size=count)] for q in Q])
    parts = pref.scale_down_parts(rows.tolist(), Q, gamma, t)
    out.update(x=x.reshape(-1), lazy_x=lazy.reshape(-1), down=_u64([p[4] for p in parts]), s_gamma=tuple(p[2] for p in parts))
    h = t // 2
    values = [h - ((ref.product(Q) % t) * (v % t) + h) % t for v in m.tolist()]      # h - rho
    out["signs"] = frozenset((v > 0) - (v < 0) for v in values)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    assert L * count == out["x"].size
    return out


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


def _check(dev, orc, plan, shape, t, batch, seed, what, forms=(COEFF, NTT)):
    """every call of one handle against the model: scale_up and lift in `forms`, d_m unchanged; scale_down of reduced and lazy words with the scratch apart
    (d_x unchanged) and the scratch the operand"""
    n = plan.n
    q_first, L, gamma_prime = shape
    Q, gamma = tuple(plan.moduli[q_first:q_first + L]), plan.moduli[gamma_prime]
    case = _case(orc, Q, gamma, t, batch, n, seed)
    plain = plan.plain(q_first, L, gamma_prime, t)
    assert plain.info()[:4] == (q_first, L, gamma_prime, t)
    count, st = batch * n, dev.stream
    d_m = dev.to_device(case["m"])
    for name, call in (("up", plain.scale_up), ("lift", plain.lift)):
        for form in forms:
            d_out = dev.to_device(canary(0, L * count))
            call(d_m.data_ptr(), d_out.data_ptr(), batch, form, st)
            got, want = dev.to_host(d_out), case[name + ("_ntt" if form == NTT else "_coeff")]
            assert np.array_equal(got, want), (what, name, form, "first differing words", _first_bad(got, want))
    assert np.array_equal(dev.to_host(d_m), case["m"]), (what, "d_m changed")
    for name in ("x", "lazy_x"):
        for in_place in (False, True):
            d_x, d_got = dev.to_device(case[name]), dev.to_device(canary(0, count))
            d_scratch = d_x if in_place else dev.to_device(canary(7, L * count))
            plain.scale_down(d_x.data_ptr(), d_got.data_ptr(), d_scratch.data_ptr(), batch, st)
            got = dev.to_host(d_got)
            assert np.array_equal(got, case["down"]), (what, name, in_place, "first differing words", _first_bad(got, case["down"]))
            assert in_place or np.array_equal(dev.to_host(d_x), case[name]), (what, name, "d_x changed")
    plain.close()
    return case


# ---- word for word against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [2, 5, 65536])
@pytest.mark.parametrize("shape", [(1, 3, 0), (1, 1, 0), (2, 4, 0), (0, 2, 2)], ids=str)
def test_tiny_moduli_every_centre_edge(agx, orc, dev, shape, t):
    """n = 8, batch 48, the six smallest admitted primes (17, 97, 113, 193, 241, 257), gamma = 17: s_gamma takes every value, both centring edges (8 and 9)
    among them, and h - rho both signs (t = 2: both values, it is never negative there).  The rounding property does not hold here: only the formula is
    compared.  t = 65536 lies above every modulus: |h - rho| exceeds q_i."""
    n = 8
    moduli = tuple(MIXES(orc, n)["tiny"])
    assert moduli[0] == 17
    if shape[2] == 2:
        moduli = moduli[1:3] + moduli[:1] + moduli[3:]
    assert moduli[shape[2]] == 17
    plan = _plan(agx, orc, n, moduli)
    case = _check(dev, orc, plan, shape, t, 48, 8 + sum(shape) + t, ("tiny", shape, t))
    assert set(case["s_gamma"]) == set(range(17))
    assert case["signs"] == ({0, 1} if t == 2 else {-1, 0, 1})      # h - rho = 0 is m' = 0
    plan.close()


@pytest.mark.parametrize("L", Q_COUNTS)
def test_class_edge_moduli_on_both_sides_of_every_capacity_step(agx, orc, dev, L):
    """n = 64, batch 3, the class-edge moduli of modulus_cases.py: narrow and 62-bit moduli meet in Q, gamma is a wide prime right behind Q; t walks through
    2, 3, 65536, 65537 and a 61-bit odd t, above every narrow modulus"""
    n = 64
    edges = _edge_list(orc, n)
    r = next(r for r in range(len(edges)) if edges[(r + L) % len(edges)] > 1 << 59)      # rotate until gamma is wide
    moduli = tuple(edges[(r + k) % len(edges)] for k in range(L + 1))
    t = (2, 3, 65536, 65537, T_ODD61)[Q_COUNTS.index(L) % 5]
    assert all(t % q for q in moduli)
    plan = _plan(agx, orc, n, moduli)
    _check(dev, orc, plan, (0, L, L), t, 3, 64 * L, ("edges", L, t))
    if L == 3:      # gamma in front of Q, and the 61-bit t on the same moduli
        plan.close()
        plan = _plan(agx, orc, n, moduli[L:] + moduli[:L])
        _check(dev, orc, plan, (1, L, 0), T_ODD61, 3, 65 * L, ("edges, gamma first", L))
    plan.close()


@pytest.mark.parametrize("radix2", [False, True], ids=["auto", "lds_radix2"])
@pytest.mark.parametrize("n,bits", [(64, 60), (1024, 60), (4096, 60), (1024, 30)])
def test_routes(agx, orc, dev, n, bits, radix2):
    """the generic inverse (n = 64), the register-blocked scaled inverse (n = 1024, 4096) and the 32-bit kernels (every modulus below 2^31), each under AUTO
    and AGX_VARIANT_LDS_RADIX2: Q is the middle of a plan of five, gamma its last prime"""
    moduli = moduli_for(orc.find_prime, n, [bits] * 5)
    plan = _plan(agx, orc, n, moduli)
    if radix2:
        plan.set_variant(agx.VARIANT_LDS_RADIX2)
    _check(dev, orc, plan, (1, 3, 4), 65537 if bits == 60 else 65536, 3, n + bits, ("routes", n, bits, radix2))
    plan.close()


# ---- layout and placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_ntt_form_is_forward_range_of_the_coefficient_form(agx, orc, dev, n):
    batch, L, t, st = 3, 3, 65537, dev.stream
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54, 61])
    plan = _plan(agx, orc, n, moduli)
    plain = plan.plain(1, L, 0, t)
    d_m = dev.to_device(_messages(np.random.default_rng(n), t, batch * n))
    for call in (plain.scale_up, plain.lift):
        d_coeff, d_ntt = dev.empty(L * batch * n), dev.empty(L * batch * n)
        call(d_m.data_ptr(), d_coeff.data_ptr(), batch, COEFF, st)
        call(d_m.data_ptr(), d_ntt.data_ptr(), batch, NTT, st)
        plan.forward_range(d_coeff.data_ptr(), d_coeff.data_ptr(), batch, 1, L, st)
        assert np.array_equal(dev.to_host(d_ntt), dev.to_host(d_coeff))
    plain.close()
    plan.close()


@pytest.mark.parametrize("L", [2, 5])
def test_odd_placement_and_guard_bands(agx, orc, dev, L):
    """every buffer at an odd word of one larger allocation (8-byte alignment only): the right words, the inputs unchanged, and every word outside the outputs
    and the scratch as it was; scale_down then with the scratch the operand"""
    n, batch, t = 64, 3, 65537
    moduli = _edge_list(orc, n)[2:2 + L + 1]
    plan = _plan(agx, orc, n, moduli)
    case = _case(orc, tuple(moduli[:L]), moduli[L], t, batch, n, 11 + L)
    plain = plan.plain(0, L, L, t)
    lm = Layout(n, 1, batch, offset=1)
    lo = Layout(n, L, batch, offset=lm.span() + 6)
    assert lm.offset % 2 == 1 and lo.offset % 2 == 1
    for name, call in (("up", plain.scale_up), ("lift", plain.lift)):
        for form in (COEFF, NTT):
            arena = arena_for(dev, n, (lm, case["m"]), (lo, None))
            call(arena.address(lm.offset), arena.address(lo.offset), batch, form, dev.stream)
            img = arena.image()
            assert not arena.faults([(lm, case["m"]), (lo, None)], img), (name, form, "a word outside d_out changed")
            assert np.array_equal(arena.frames(lo, img), case[name + ("_ntt" if form == NTT else "_coeff")]), (name, form)
    lx = Layout(n, L, batch, offset=1)
    ls = Layout(n, L, batch, offset=lx.span() + 6)
    ld = Layout(n, 1, batch, offset=ls.span() + 4)
    assert ls.offset % 2 == 1 and ld.offset % 2 == 1
    arena = arena_for(dev, n, (lx, case["lazy_x"]), (ls, None), (ld, None))
    plain.scale_down(arena.address(lx.offset), arena.address(ld.offset), arena.address(ls.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lx, case["lazy_x"]), (ls, None), (ld, None)], img), "a word outside d_m and the scratch changed"
    assert np.array_equal(arena.frames(ld, img), case["down"])
    arena = arena_for(dev, n, (lx, case["lazy_x"]), (ld, None))
    plain.scale_down(arena.address(lx.offset), arena.address(ld.offset), arena.address(lx.offset), batch, dev.stream)
    img = arena.image()
    assert not arena.faults([(lx, None), (ld, None)], img), "a word outside d_m and d_x changed"
    assert np.array_equal(arena.frames(ld, img), case["down"])
    plain.close()
    plan.close()


# ---- argument rules ------------------------------------------------------------------------------------------------------------------------
def test_creation_statuses(agx, orc, dev):
    n = 64
    a, b, c, d, e = moduli_for(orc.find_prime, n, [60, 60, 45, 30, 54])
    plan = _plan(agx, orc, n, (a, b, c, d, e), inverse=False)      # creation needs no inverse tables
    C, t = agx.Plain, 65537
    for args in ((0, 0, 3), (4, 2, 0), (5, 1, 0), (0, 6, 0), (0xFFFFFFFF, 2, 0), (2, 0xFFFFFFFF, 0), (0, 2, 5), (0, 2, 0xFFFFFFFF), (0, 2, 0), (0, 2, 1), (1, 3, 3)):
        assert status_of(agx, C, plan, *args, t) == 5, args      # the range, gamma's place
        assert status_of(agx, C, plan, *args, 0) == 5, args
    for bad_t in (0, 1, 1 << 62, (1 << 64) - 1):
        assert status_of(agx, C, plan, 0, 2, 3, bad_t) == 5, bad_t
    assert status_of(agx, C, plan, 0, 2, 3, 2 * a) == 3 and status_of(agx, C, plan, 0, 2, 3, 3 * b) == 3      # q_i | t
    assert status_of(agx, C, plan, 0, 2, 3, 4 * d) == 3 and status_of(agx, C, plan, 0, 2, 3, d) == 3          # gamma | t
    assert status_of(agx, C, plan, 0, 2, 3, e) == 0 and status_of(agx, C, plan, 0, 2, 3, 5 * c) == 0          # a plan modulus outside Q and gamma: fine
    for args in ((0, 1, 1), (1, 2, 0), (3, 2, 0), (0, 4, 4), (2, 1, 4)):
        for tt in (2, 3, 65536, t, T_ODD61, (1 << 62) - 1 if args != (3, 2, 0) else 6):      # 2^62 - 1 = 3 x ...: coprime to these primes
            plain = C(plan, *args, tt)
            assert plain.info()[:4] == args + (tt,)
            plain.close()
    plan.close()
    twice = _plan(agx, orc, n, (a, b, a, c, d), inverse=False)
    assert status_of(agx, C, twice, 0, 3, 3, t) == 3      # two equal moduli in Q
    assert status_of(agx, C, twice, 0, 2, 2, t) == 3      # gamma is a modulus of Q
    assert status_of(agx, C, twice, 0, 3, 3, 0) == 3 and status_of(agx, C, twice, 0, 2, 2, 1 << 62) == 3      # the moduli before t's range
    assert status_of(agx, C, twice, 0, 3, 1, 0) == 5      # the place before the moduli
    assert status_of(agx, C, twice, 1, 1, 3, 0) == 5 and status_of(agx, C, twice, 1, 1, 3, 2 * b) == 3 and status_of(agx, C, twice, 1, 1, 3, 4 * c) == 3      # t's range, then its factors
    C(twice, 1, 1, 0, t).close(), C(twice, 2, 2, 1, t).close()      # the repeated modulus as gamma and outside the call, or once in Q: fine
    twice.close()
    many = _plan(agx, orc, n, _edge_list(orc, n)[:18], inverse=False)
    assert status_of(agx, C, many, 0, 17, 17, t) == 5     # more than 16 primes in Q
    C(many, 0, 16, 17, t).close(), C(many, 1, 16, 0, t).close()
    many.close()


def test_status_rules_in_order_and_rejected_calls_write_nothing(agx, orc, dev):
    n, batch, L, t = 64, 2, 3, 65537
    moduli = moduli_for(orc.find_prime, n, [45, 52, 60, 57])
    plan, forward_only = _plan(agx, orc, n, moduli), _plan(agx, orc, n, moduli, inverse=False)
    case = _case(orc, tuple(moduli[:L]), moduli[L], t, batch, n, 77)
    plain, lame = plan.plain(0, L, L, t), forward_only.plain(0, L, L, t)
    slab, w, st = batch * n, 8, dev.stream
    lx = Layout(n, L, batch, offset=0)
    ls = Layout(n, L, batch, offset=L * slab)                  # the scratch right behind d_x, d_m right behind the scratch: they meet end to end
    lm = Layout(n, 1, batch, offset=2 * L * slab)
    lo = Layout(n, L, batch, offset=2 * L * slab + slab)       # scale_up's output right behind d_m
    arena = arena_for(dev, n, (lx, case["x"]), (ls, None), (lm, case["m"]), (lo, None))
    before = arena.image()
    px, ps, pm, po = (arena.address(l.offset) for l in (lx, ls, lm, lo))
    for call in (plain.scale_up, plain.lift, lame.scale_up):
        assert [status_of(agx, call, *a, batch, form, st) for a in ((0, po), (pm, 0)) for form in (COEFF, NTT, 7)] == [1] * 6      # NULL, before the form
        assert status_of(agx, call, pm, po, batch, 2, st) == 5 and status_of(agx, call, pm + 4, po, batch, -1, st) == 5          # an unknown form
        for form in (COEFF, NTT):
            assert status_of(agx, call, pm + 4, po, batch, form, st) == 5 and status_of(agx, call, pm, po + 4, batch, form, st) == 5      # uint64_t data
            assert status_of(agx, call, pm, po, (1 << 64) - 1, form, st) == 5 and status_of(agx, call, pm, po, 1 << 40, form, st) == 5  # the grid limit
            for out in (pm, pm + w, pm + w * (slab - 1), pm - w * (L * slab - 1)):      # d_out touches d_m: out of place only
                assert status_of(agx, call, pm, out, batch, form, st) == 5, (form, out - pm)
            call(pm, po, 0, form, st)      # an empty batch: nothing launched
    D = plain.scale_down
    assert [status_of(agx, D, *a, batch, st) for a in ((0, pm, ps), (px, 0, ps), (px, pm, 0))] == [1, 1, 1]                    # NULL
    assert [status_of(agx, D, *a, batch, st) for a in ((px + 4, pm, ps), (px, pm + 4, ps), (px, pm, ps + 4))] == [5, 5, 5]       # uint64_t data
    assert status_of(agx, D, px, pm, ps, (1 << 64) - 1, st) == 5 and status_of(agx, D, px, pm, ps, 1 << 40, st) == 5           # a batch past the grid limit
    for scratch in (px + w, px + w * (n // 2), px + w * (L * slab - 1), px - w * (L * slab - 1)):      # a scratch that straddles d_x: not d_x itself, not apart
        assert status_of(agx, D, px, po, scratch, batch, st) == 5
    for out in (px, px + w * (n // 2), px + w * (L * slab - 1), ps, ps + w * (L * slab - 1), px - w * (slab - 1)):      # d_m touches d_x or the scratch
        assert status_of(agx, D, px, out, ps, batch, st) == 5
    assert status_of(agx, D, px, px + w * slab, px, batch, st) == 5      # ... also where the scratch is d_x
    # a plan without inverse tables: behind the argument rules, in front of the empty batch
    assert status_of(agx, lame.scale_down, px + 4, pm, ps, batch, st) == 5 and status_of(agx, lame.scale_down, px, px, ps, batch, st) == 5
    assert status_of(agx, lame.scale_down, px, pm, ps, batch, st) == 9 and status_of(agx, lame.scale_down, px, pm, ps, 0, st) == 9
    D(px, pm, ps, 0, st)      # an empty batch: nothing launched
    D(px, pm, px, 0, st)
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # allowed: ranges that meet end to end; a forward-only plan serves scale_up and lift
    lame.scale_up(pm, po, batch, NTT, st)
    img = arena.image()
    assert np.array_equal(arena.frames(lo, img), case["up_ntt"]) and not arena.faults([(lx, case["x"]), (ls, None), (lm, case["m"]), (lo, None)], img)
    assert np.array_equal(arena.frames(ls, img), arena.frames(ls, before))
    lm2 = Layout(n, 1, batch, offset=lm.offset)
    arena2 = arena_for(dev, n, (lx, case["x"]), (ls, None), (lm2, None))
    D(arena2.address(0), arena2.address(lm2.offset), arena2.address(ls.offset), batch, st)
    img = arena2.image()
    assert np.array_equal(arena2.frames(lm2, img), case["down"]) and np.array_equal(arena2.frames(lx, img), case["x"])
    assert not arena2.faults([(lx, case["x"]), (ls, None), (lm2, None)], img)
    for h in (plain, lame, plan, forward_only):
        h.close()


def test_launch_counts_under_both_variants(agx, orc, dev):
    """launches_scale_down = the plan's inverse launches + 1, launches_ntt_form = 1 + its forward launches, under the current variant.  The plan's own counts
    come from a basis of the same plan: aux_info is 1 + forward; mod_down_info is inverse + 1 on the two-launch route, 2 x inverse + 1 + forward otherwise."""
    for n, bits in [(8, 60), (64, 60), (1024, 60), (4096, 60), (32768, 60), (1024, 30)]:
        plan = _plan(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 4))
        plain, basis = plan.plain(0, 2, 3, 65536), plan.basis_aux(0, 2, 2, 1, 3)
        for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_AUTO):
            plan.set_variant(variant)
            fwd, down = basis.aux_info()[2] - 1, basis.mod_down_launches()
            inv = down - 1 if down <= 3 else (down - 1 - fwd) // 2
            assert fwd in (1, 2) and inv in (1, 2), (n, bits, variant, fwd, down)
            if variant == agx.VARIANT_LDS_RADIX2:
                assert (fwd, inv) == ((1, 1) if n <= 16384 else (2, 2)), (n, fwd, inv)
            assert plain.info() == (0, 2, 3, 65536, inv + 1, 1 + fwd), (n, bits, variant)
        plain.close(), basis.close()
        plan.close()


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_the_calls_are_graph_capturable(agx, orc, dev, n):
    """all three calls captured on a side stream -- scale_up to NTT form, lift to coefficient form, scale_down with the scratch apart and with the scratch the
    operand of a second buffer -- and replayed on fresh inputs: the eager result"""
    torch = dev.torch
    batch, L, t = 3, 3, 65537
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan = _plan(agx, orc, n, moduli)
    plain = plan.plain(0, L, L, t)
    rng = np.random.default_rng(n)
    count = batch * n
    xs = [np.stack([rng.integers(0, 4 * q, size=count, dtype=np.uint64) for q in moduli[:L]]).reshape(-1) for _ in range(2)]
    ms = [rng.integers(0, 2**64, size=count, dtype=np.uint64) for _ in range(2)]
    d_x, d_y, d_scratch, d_m = dev.to_device(xs[0]), dev.to_device(xs[0]), dev.empty(L * count), dev.to_device(ms[0])
    d_up, d_lift, d_down = dev.empty(L * count), dev.empty(L * count), [dev.empty(count) for _ in range(2)]

    def every(s):
        plain.scale_up(d_m.data_ptr(), d_up.data_ptr(), batch, NTT, s)
        plain.lift(d_m.data_ptr(), d_lift.data_ptr(), batch, COEFF, s)
        plain.scale_down(d_x.data_ptr(), d_down[0].data_ptr(), d_scratch.data_ptr(), batch, s)
        plain.scale_down(d_y.data_ptr(), d_down[1].data_ptr(), d_y.data_ptr(), batch, s)

    graph = capture(dev, every, every)
    for x, m in zip(xs[::-1], ms[::-1]):
        for d in (d_x, d_y):
            d.copy_(torch.from_numpy(x.view(np.int64).copy()))
        d_m.copy_(torch.from_numpy(m.view(np.int64).copy()))
        for d in [d_up, d_lift] + d_down:
            d.zero_()
        graph.replay()
        dev.sync()
        got = [dev.to_host(d) for d in [d_up, d_lift] + d_down]
        e_m, e_x = dev.to_device(m), dev.to_device(x)
        e_up, e_lift, e_down, e_scratch = dev.empty(L * count), dev.empty(L * count), dev.empty(count), dev.empty(L * count)
        plain.scale_up(e_m.data_ptr(), e_up.data_ptr(), batch, NTT, dev.stream)
        plain.lift(e_m.data_ptr(), e_lift.data_ptr(), batch, COEFF, dev.stream)
        plain.scale_down(e_x.data_ptr(), e_down.data_ptr(), e_scratch.data_ptr(), batch, dev.stream)
        want = [dev.to_host(d) for d in (e_up, e_lift, e_down, e_down)]
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), n
        assert np.array_equal(dev.to_host(d_x), x) and np.array_equal(dev.to_host(d_m), m)
        if n == 64:
            Q = tuple(moduli[:L])
            assert np.array_equal(want[0], oracle_forward_set(orc, n, Q, _u64(pref.scale_up(m.tolist(), Q, t))).reshape(-1))
            assert np.array_equal(want[1], _u64(pref.lift(m.tolist(), Q, t)).reshape(-1))
            rows = oracle_inverse_set(orc, n, Q, x.reshape(L, -1)).tolist()
            assert np.array_equal(want[2], _u64(pref.scale_down(rows, Q, moduli[L], t)))
    plain.close()
    plan.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_bfv_end_to_end_on_library_calls(agx, orc, dev):
    """The INTEGRATION.md listing "BFV encryption, plain operands and decryption" at n = 64, batch 2, BFV_WIDTHS / BFV_T, ONE plan, gamma = the first prime of
    B: two messages per frame encrypted from scale_up, multiplied by the quotient listing, the three-component result decrypted by inner_product and
    scale_down to negacyclic(m1, m2, t) on every coefficient; ciphertexts of bfv_conv_ref.encrypt decrypt too; add-plain and multiply-plain through
    scale_up / lift decrypt to m + m' and m m' mod t."""
    n, batch = 64, 2
    w = ref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    B = tuple(prime_below(orc, 1 << b, n) for b in w["B"])
    m_sk, m_tilde, t = prime_below(orc, 1 << w["m_sk"], n), prime_below(orc, 1 << w["m_tilde"], n), ref.BFV_T
    L, K = len(Q), len(B)
    W = L + K + 1
    moduli = Q + B + (m_sk, m_tilde)      # Q = [0, L), B = [L, L + K), m_sk = L + K, m~ = L + K + 1
    P = len(moduli)
    plan = _plan(agx, orc, n, moduli)
    plain = plan.plain(0, L, L, t)
    slab, st = batch * n, dev.stream
    at = lambda d, words: d.data_ptr() + 8 * words      # noqa: E731
    rng = ref.Rng(1999)
    nprng = np.random.default_rng(1999)
    s = ref.keygen(rng, n)
    s2 = [ref.negacyclic([v % q for v in s], [v % q for v in s], q) for q in Q]
    ones = [[1] + [0] * (n - 1)] * L
    # (1^, s^, s^2^) under every plan prime, the slabs outside Q zero: agx_ntt_inner_product takes operands over the whole plan
    key = np.zeros((3, P, n), dtype=np.uint64)
    key[0, :L] = oracle_forward_set(orc, n, Q, _u64(ones))
    key[1, :L] = oracle_forward_set(orc, n, Q, _u64([[v % q for v in s] for q in Q]))
    key[2, :L] = oracle_forward_set(orc, n, Q, _u64(s2))
    d_key, d_shat = dev.to_device(key.reshape(-1)), dev.to_device(key[1, :L].reshape(-1))

    def decrypt(components):
        """components: device tensors of [L][batch][n] NTT-form slabs, two or three -> [batch][n] messages: the phase by one inner product, then scale_down"""
        terms = len(components)
        d_a = dev.to_device(np.zeros(terms * P * slab, dtype=np.uint64))
        for k, c in enumerate(components):
            d_a[k * P * slab:k * P * slab + L * slab].copy_(c)      # the Q slabs of term k
        d_phase, d_msg = dev.empty(P * slab), dev.to_device(canary(0, slab))
        plan.inner_product(d_a.data_ptr(), d_key.data_ptr(), d_phase.data_ptr(), batch, terms, 1, 1, st)
        plain.scale_down(d_phase.data_ptr(), d_msg.data_ptr(), d_phase.data_ptr(), batch, st)
        return dev.to_host(d_msg).reshape(batch, n).tolist()

    def encrypt(msgs):
        """msgs [batch][n] -> a device ciphertext [2][L][batch][n] in NTT form: c_1 = a uniform, c_0 = scale_up(m) - a s + e, on library calls"""
        d_ct, d_m, d_e = dev.empty(2 * L * slab), dev.to_device(_u64(msgs).reshape(-1)), dev.empty(L * slab)
        a = np.stack([nprng.integers(0, q, size=slab, dtype=np.uint64) for q in Q])      # uniform NTT-form words are a uniform a
        e = nprng.integers(-8, 9, size=slab)
        d_ct[L * slab:].copy_(dev.to_device(a.reshape(-1)))
        d_e.copy_(dev.to_device(_u64([[int(v) % q for v in e] for q in Q]).reshape(-1)))
        plan.forward_range(d_e.data_ptr(), d_e.data_ptr(), batch, 0, L, st)
        plain.scale_up(d_m.data_ptr(), d_ct.data_ptr(), batch, NTT, st)                                              # Delta m
        d_as = dev.empty(L * slab)
        plan.mul_add_galois(d_shat.data_ptr(), at(d_ct, L * slab), d_as.data_ptr(), batch, 1, 1, False, 0, L, st)    # a s
        plan.sub(d_ct.data_ptr(), d_as.data_ptr(), d_ct.data_ptr(), batch, 0, L, st)
        plan.add(d_ct.data_ptr(), d_e.data_ptr(), d_ct.data_ptr(), batch, 0, L, st)                                  # + e
        return d_ct

    msgs = [[[rng.below(t) for _ in range(n)] for _ in range(batch)] for _ in range(2)]      # [operand][frame][n]
    cts = [encrypt(msgs[o]) for o in range(2)]
    for o in range(2):
        assert decrypt([cts[o][:L * slab], cts[o][L * slab:]]) == msgs[o], ("a fresh ciphertext", o)
    # ciphertexts of the reference's encrypt decrypt too
    host = [ref.encrypt(rng, msgs[0][f], s, Q, t) for f in range(batch)]      # [frame][component][L][n]
    d_host = dev.to_device(np.stack([oracle_forward_set(orc, n, Q, _u64([[host[f][c][j] for f in range(batch)] for j in range(L)])) for c in range(2)]).reshape(-1))
    assert decrypt([d_host[:L * slab], d_host[L * slab:]]) == msgs[0], "a ciphertext of bfv_conv_ref.encrypt"
    # add-plain: c_0 + scale_up(m'); multiply-plain: (c_0, c_1) o lift(m')
    other = [[rng.below(t) for _ in range(n)] for _ in range(batch)]
    d_other, d_plain, d_sum, d_prod = dev.to_device(_u64(other).reshape(-1)), dev.empty(L * slab), dev.empty(L * slab), dev.empty(2 * L * slab)
    plain.scale_up(d_other.data_ptr(), d_plain.data_ptr(), batch, NTT, st)
    plan.add(cts[0].data_ptr(), d_plain.data_ptr(), d_sum.data_ptr(), batch, 0, L, st)
    assert decrypt([d_sum, cts[0][L * slab:]]) == [[(u + v) % t for u, v in zip(msgs[0][f], other[f])] for f in range(batch)], "add-plain"
    plain.lift(d_other.data_ptr(), d_plain.data_ptr(), batch, NTT, st)
    for c in range(2):
        plan.mul_add_galois(d_plain.data_ptr(), at(cts[0], c * L * slab), at(d_prod, c * L * slab), batch, 1, None, False, 0, L, st)
    assert decrypt([d_prod[:L * slab], d_prod[L * slab:]]) == [ref.negacyclic(msgs[0][f], other[f], t) for f in range(batch)], "multiply-plain"
    # the multiplication by the quotient listing, then the three-component result decrypted
    to_bsk, divide = plan.basis_aux(0, L, L, K + 1, L + K + 1), plan.basis_quotient(L, K, 0, L, L + K, t)
    d_ops = [dev.to_device(np.zeros(2 * W * slab, dtype=np.uint64)) for _ in range(2)]
    d_coeff = dev.empty(L * slab)
    for o in range(2):
        for c in range(2):
            d_ops[o][c * W * slab:c * W * slab + L * slab].copy_(cts[o][c * L * slab:(c + 1) * L * slab])
            plan.inverse_range(at(d_ops[o], c * W * slab), d_coeff.data_ptr(), batch, 0, L, st)
            to_bsk.extend_mont(d_coeff.data_ptr(), at(d_ops[o], (c * W + L) * slab), batch, NTT, st)
    d_tensor, d_out = dev.empty(3 * W * slab), dev.empty(3 * L * slab)
    plan.tensor(d_ops[0].data_ptr(), d_ops[1].data_ptr(), d_tensor.data_ptr(), batch, 0, W, st)
    for k in range(3):
        d = at(d_tensor, k * W * slab)
        divide.quotient(d, at(d_out, k * L * slab), d, batch, st)
    got = decrypt([d_out[k * L * slab:(k + 1) * L * slab] for k in range(3)])
    assert got == [ref.negacyclic(msgs[0][f], msgs[1][f], t) for f in range(batch)], "the product"
    # ... and as the big-integer division decrypts it
    out = dev.to_host(d_out).reshape(3, L, batch, n)
    for f in range(batch):
        coeff = [oracle_inverse_set(orc, n, Q, out[k][:, f]).tolist() for k in range(3)]
        assert ref.decrypt(coeff, s, Q, t) == got[f], ("frame", f)
    for h in (to_bsk, divide, plain, plan):
        h.close()
