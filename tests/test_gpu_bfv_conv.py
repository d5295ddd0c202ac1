"""agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont on the device, word for word against the Python-integer model (tests/bfv_conv_ref.py): the
coefficient form at tiny and class-edge moduli, at every source count on both sides of a register-capacity step, with lazy inputs and at odd 8-byte-only
placement; the NTT form against agx_ntt_forward of the coefficient form; the status rules in their order with guard words; an empty batch; graph capture;
the other calls of a basis with an auxiliary prime against the ordinary basis; the launch count; and a whole BFV multiplication by the seven steps of
INTEGRATION.md, "BFV multiplication (BEHZ)", every coefficient decrypted and the intermediate words compared with the model's."""
import functools

import numpy as np
import pytest

import bfv_conv_ref as ref
from gpu_util import Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, status_of
from modulus_cases import MIXES, edge_moduli, prime_below
from rns_ref import oracle_forward_set, oracle_inverse_set

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
SOURCE_COUNTS = (1, 2, 3, 4, 5, 8, 9, 16)      # both sides of every step of the kernels' source capacity (1, 2, 4, 8, 16)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _deltas(m, batch, n):
    """u - k per coefficient.  Every frame opens with 0 (r = V mod m), None (replaced below by u + 1 or u + 2: X' negative) and both centring edges; behind
    them the frames walk through the edges' neighbours or, for m = 17, through every value in [-8, 8]"""
    half = (m - 1) // 2
    pool = list(range(-half, half + 1)) if m <= 17 else [1, -1, half - 1, -half + 1, 2, -2, None, half, -half, 0]
    out = []
    for f in range(batch):
        out += [0, None, half, -half] + [pool[(f * (n - 4) + e) % len(pool)] for e in range(n - 4)]
    return out


@functools.lru_cache(maxsize=None)
def _case(src, dst, m, batch, n, seed):
    """x [S][batch n] reduced, r [batch n] reduced, the same spread over the lazy range, and the model's words of both calls; every frame holds every kind
    of r: V mod m, r for a negative X', r at both centring edges"""
    rng = np.random.default_rng(seed)
    count = batch * n
    x = [[int(v) for v in rng.integers(0, q, size=count, dtype=np.uint64)] for q in src]
    for i, q in enumerate(src):      # the ends of the residue range in every frame
        x[i][0::n] = [0] * batch
        x[i][1::n] = [q - 1] * batch
    D = ref.product(src)
    V = ref.lift(x, src)
    r, negative = [], 0
    for e, (v, delta) in enumerate(zip(V, _deltas(m, batch, n))):
        if delta is None:
            delta = v // D + 1 + e % 2      # k = -1, -2: X' = X - D, X - 2D
        negative += v % D + (v // D - delta) * D < 0
        r.append((v - delta * D) % m)
    assert negative >= batch
    exact = ref.extend_exact(x, r, src, dst, m)
    alphas = ref.alpha_exact(x, r, src, m)[1]
    assert {-(m - 1) // 2, (m - 1) // 2, 0} <= set(alphas) and (m != 17 or set(alphas) == set(range(-8, 9)))
    lazy_x = [[v + int(k) * q for v, k in zip(row, rng.integers(0, 4, size=count))] for row, q in zip(x, src)]
    lazy_r = [v + int(k) * m for v, k in zip(r, rng.integers(0, 4, size=count))]
    out = {"x": _u64(x).reshape(-1), "r": _u64(r), "lazy_x": _u64(lazy_x).reshape(-1), "lazy_r": _u64(lazy_r), "exact": _u64(exact).reshape(-1),
           "mont": _u64(ref.extend_mont(x, src, dst, m)).reshape(-1)}
    for a in out.values():
        a.setflags(write=False)
    return out


def _ranges(moduli, sf, S, df, T, aux):
    return tuple(moduli[sf:sf + S]), tuple(moduli[df:df + T]), moduli[aux]


def _run(dev, basis, kind, x, r, out_words, batch, form):
    d_x, d_r, d_out = dev.to_device(x), dev.to_device(r), dev.to_device(canary(0, out_words))
    if kind == "exact":
        basis.extend_exact(d_x.data_ptr(), d_r.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
    else:
        basis.extend_mont(d_x.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
    return dev.to_host(d_out)


def _check_coeff(dev, plan, shape, batch, seed, what):
    n = plan.n
    sf, S, df, T, aux = shape
    case = _case(*_ranges(plan.moduli, *shape), batch, n, seed)
    basis = plan.basis_aux(*shape)
    assert basis.aux_info()[:2] == (True, aux) and basis.info()[:4] == (sf, S, df, T)
    for kind in ("exact", "mont"):
        for name, x, r in (("reduced", case["x"], case["r"]), ("lazy", case["lazy_x"], case["lazy_r"])):
            got = _run(dev, basis, kind, x, r, T * batch * n, batch, COEFF)
            bad = np.flatnonzero(got != case[kind])
            assert bad.size == 0, (what, kind, name, "first differing words", bad[:4].tolist(), got[bad[:4]].tolist(), case[kind][bad[:4]].tolist())
    basis.close()


@functools.lru_cache(maxsize=None)
def _edge_list(orc, n):
    moduli = tuple(dict.fromkeys(edge_moduli(orc, n).values()))
    assert len(moduli) >= 20 and max(moduli) > 1 << 61 and min(moduli) < 1 << 30
    return moduli


# ---- coefficient form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 3, 3, 0), (1, 2, 4, 2, 3), (2, 1, 3, 1, 0), (0, 3, 4, 2, 3), (1, 5, 0, 1, 6)], ids=str)
def test_tiny_moduli_every_alpha(agx, orc, dev, shape):
    """n = 8, the six smallest admitted primes (17, 97, 113, 193, 241, 257) and one below 400: with m = 17 (auxiliary prime 0) every alpha in [-8, 8] occurs"""
    n = 8
    moduli = tuple(MIXES(orc, n)["tiny"]) + (prime_below(orc, 400, n),)
    assert moduli[0] == 17 and len(set(moduli)) == 7
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _check_coeff(dev, plan, shape, 6, 8 + sum(shape), ("tiny", shape))
    plan.close()


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("S", SOURCE_COUNTS)
def test_class_edge_moduli_at_every_source_count(agx, orc, dev, S, T):
    """n = 64, batch 3, the class-edge moduli of modulus_cases.py in one plan: narrow and 62-bit moduli meet in one source set, and the auxiliary prime
    comes from another class with every S"""
    n = 64
    moduli = _edge_list(orc, n)
    P = len(moduli)
    sf = (5 * S) % (P - S - T)      # sources, then the targets, then the auxiliary prime
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)      # a forward-only plan serves
    _check_coeff(dev, plan, (sf, S, sf + S, T, sf + S + T), 3, 64 * S + T, ("edges", S, T))
    if S == 2:      # the auxiliary prime in front of both ranges, the targets in front of the sources
        _check_coeff(dev, plan, (P - 2, 2, 1, T, 0), 3, 7 + T, ("edges, reversed", T))
    plan.close()


@pytest.mark.parametrize("S", [2, 5])
def test_odd_placement_and_guard_bands(agx, orc, dev, S):
    """every buffer at an odd word of one larger allocation (8-byte alignment only): the right words, the inputs unchanged, and every word outside d_out as it was"""
    n, batch, T = 64, 3, 3
    moduli = _edge_list(orc, n)
    shape = (3, S, 3 + S, T, 3 + S + T)
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    case = _case(*_ranges(plan.moduli, *shape), batch, n, 11 + S)
    basis = plan.basis_aux(*shape)
    lx = Layout(n, S, batch, offset=1)
    lr = Layout(n, 1, batch, offset=lx.span() + 6)
    lo = Layout(n, T, batch, offset=lr.span() + 4)
    assert lx.offset % 2 == 1 and lr.offset % 2 == 1 and lo.offset % 2 == 1
    for kind in ("exact", "mont"):
        arena = arena_for(dev, n, (lx, case["lazy_x"]), (lr, case["lazy_r"]), (lo, None))
        if kind == "exact":
            basis.extend_exact(arena.address(lx.offset), arena.address(lr.offset), arena.address(lo.offset), batch, COEFF, dev.stream)
        else:
            basis.extend_mont(arena.address(lx.offset), arena.address(lo.offset), batch, COEFF, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx, case["lazy_x"]), (lr, case["lazy_r"]), (lo, None)], img), "a word outside d_out changed"
        assert np.array_equal(arena.frames(lo, img), case[kind]), kind
    basis.close()
    plan.close()


# ---- NTT form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radix2", [False, True], ids=["auto", "lds_radix2"])
@pytest.mark.parametrize("n", [64, 1024])
def test_ntt_form_is_the_forward_of_the_coefficient_form(agx, orc, dev, n, radix2):
    batch, shape = 3, (0, 2, 2, 3, 5)
    sf, S, df, T, aux = shape
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54, 61, 59, 50])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    if radix2:
        plan.set_variant(agx.VARIANT_LDS_RADIX2)
    P, slab = len(moduli), batch * n
    case = _case(*_ranges(plan.moduli, *shape), batch, n, n + 5)
    basis = plan.basis_aux(*shape)
    for kind in ("exact", "mont"):
        coeff = _run(dev, basis, kind, case["lazy_x"], case["lazy_r"], T * slab, batch, COEFF)
        assert np.array_equal(coeff, case[kind]), kind
        whole = np.zeros(P * slab, dtype=np.uint64)
        whole[df * slab:(df + T) * slab] = coeff
        d_whole = dev.to_device(whole)
        plan.forward(d_whole.data_ptr(), d_whole.data_ptr(), batch, dev.stream)
        want = dev.to_host(d_whole)[df * slab:(df + T) * slab]
        got = _run(dev, basis, kind, case["lazy_x"], case["lazy_r"], T * slab, batch, NTT)
        assert np.array_equal(got, want), (kind, "NTT form")
        assert np.array_equal(got, oracle_forward_set(orc, n, moduli[df:df + T], case[kind]).reshape(-1)), (kind, "against the oracle")
    basis.close()
    plan.close()


def test_launch_count_is_one_more_than_the_forward(agx, orc, dev):
    """aux_info's count against the unfused pair's of an ordinary basis with three sources (the coefficient-form launch and the plan's forward), which
    tests/test_gpu_basis_extend.py pins: two launches, three at n = 32768 under AGX_VARIANT_LDS_RADIX2; an ordinary basis reports no auxiliary prime"""
    for n, bits in [(8, 60), (64, 60), (1024, 60), (4096, 60), (32768, 60), (1024, 30)]:
        plan, _ = plan_for_moduli(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * 5), inverse=False)
        aux, plain = plan.basis_aux(0, 1, 1, 3, 4), plan.basis(0, 3, 0, 4)
        assert plain.aux_info()[0] is False
        for variant, want in ((agx.VARIANT_AUTO, 2), (agx.VARIANT_LDS_RADIX2, 2 if n <= 16384 else 3), (agx.VARIANT_AUTO, 2)):
            plan.set_variant(variant)
            assert aux.aux_info() == (True, 4, want) and plain.info()[4] == want and plain.aux_info()[2] == want, (n, bits, variant)
        aux.close(), plain.close()
        plan.close()


# ---- argument rules --------------------------------------------------------------------------------------------------------------------------
def test_creation_statuses(agx, orc, dev):
    n = 64
    a, b, c, d = moduli_for(orc.find_prime, n, [60, 60, 45, 30])
    plan, _ = plan_for_moduli(agx, orc, n, (a, b, c, d), inverse=False)
    A = agx.Basis.with_aux
    assert status_of(agx, A, plan, 0, 0, 1, 1, 3) == 5 and status_of(agx, A, plan, 0, 1, 1, 0, 3) == 5 and status_of(agx, A, plan, 3, 2, 0, 1, 2) == 5      # create's rules
    assert status_of(agx, A, plan, 0, 1, 1, 2, 4) == 5 and status_of(agx, A, plan, 0, 1, 1, 2, 0xFFFFFFFF) == 5      # the auxiliary prime past P
    assert status_of(agx, A, plan, 0, 2, 2, 1, 0) == 5 and status_of(agx, A, plan, 0, 2, 2, 1, 1) == 5               # ... inside the source range
    assert status_of(agx, A, plan, 0, 1, 1, 2, 1) == 5 and status_of(agx, A, plan, 0, 1, 1, 2, 2) == 5               # ... inside the target range
    assert status_of(agx, A, plan, 0, 3, 1, 3, 2) == 5                                                                 # ... inside both
    for args in ((0, 1, 1, 2, 3), (1, 2, 3, 1, 0), (0, 1, 0, 1, 2), (1, 1, 3, 1, 2)):
        basis = A(plan, *args)
        assert basis.aux_info()[:2] == (True, args[4]) and basis.info()[:4] == args[:4]
        basis.close()
    plan.close()
    twice, _ = plan_for_moduli(agx, orc, n, (a, b, a, c), inverse=False)
    assert status_of(agx, A, twice, 0, 3, 3, 1, 99) == 3      # two equal source moduli: create's rule, in front of the auxiliary prime's
    assert status_of(agx, A, twice, 0, 1, 1, 1, 2) == 3       # m is a source's modulus
    assert status_of(agx, A, twice, 1, 1, 2, 2, 0) == 3       # m is a target's modulus
    A(twice, 1, 1, 3, 1, 0).close()                           # the repeated modulus as m, neither a source's nor a target's: fine
    A(twice, 1, 1, 3, 1, 2).close()
    twice.close()


def test_status_rules_in_order_and_rejected_calls_write_nothing(agx, orc, dev):
    n, batch, shape = 64, 2, (0, 2, 2, 3, 5)
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54, 61, 59])
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    case = _case(*_ranges(plan.moduli, *shape), batch, n, 77)
    aux, plain = plan.basis_aux(*shape), plan.basis(*shape[:4])
    slab, w, st = batch * n, 8, dev.stream
    lx = Layout(n, S, batch, offset=0)
    lr = Layout(n, 1, batch, offset=S * slab)      # the auxiliary slab follows the source slabs, as in a BFV multiplication
    lo = Layout(n, T, batch, offset=(S + 1) * slab + 2 * n)
    arena = arena_for(dev, n, (lx, case["x"]), (lr, case["r"]), (lo, None))
    before = arena.image()
    px, pr, po = arena.address(0), arena.address(lr.offset), arena.address(lo.offset)
    E, M = aux.extend_exact, aux.extend_mont
    for form in (COEFF, NTT, 2, -1):      # the NULL rule first, whatever the form
        assert [status_of(agx, E, *a, batch, form, st) for a in ((0, pr, po), (px, 0, po), (px, pr, 0))] == [1, 1, 1]
        assert [status_of(agx, M, *a, batch, form, st) for a in ((0, po), (px, 0))] == [1, 1]
        assert status_of(agx, plain.extend_exact, px, 0, po, batch, form, st) == 1 and status_of(agx, plain.extend_mont, px, 0, batch, form, st) == 1
        # a basis without an auxiliary prime
        assert status_of(agx, plain.extend_exact, px, pr, po, batch, form, st) == 5 and status_of(agx, plain.extend_mont, px, po, batch, form, st) == 5
    for form in (2, -1, 7):      # an unknown form
        assert status_of(agx, E, px, pr, po, batch, form, st) == 5 and status_of(agx, M, px, po, batch, form, st) == 5
    for form in (COEFF, NTT):
        # uint64_t data
        assert [status_of(agx, E, *a, batch, form, st) for a in ((px + 4, pr, po), (px, pr + 4, po), (px, pr, po + 4))] == [5, 5, 5]
        assert [status_of(agx, M, *a, batch, form, st) for a in ((px + 4, po), (px, po + 4))] == [5, 5]
        # out of place only: d_out touches neither d_x ...
        for out in (px, px + w * (n // 2), px + w * (S * slab - 1)):      # d_out == d_x, inside it, on its last word
            assert status_of(agx, E, px, po, out, batch, form, st) == 5 and status_of(agx, M, px, out, batch, form, st) == 5
        for x in (po + w * (n // 2), po + w * (T * slab - 1)):             # d_x starts inside d_out, on its last word
            assert status_of(agx, E, x, pr, po, batch, form, st) == 5 and status_of(agx, M, x, po, batch, form, st) == 5
        # ... nor d_xaux
        for out in (pr, pr + w * (slab - 1), pr - w * (T * slab - 1)):     # d_out == d_xaux, on its last word, d_out's last word on its first
            assert status_of(agx, E, px + w * 8 * slab, pr, out, batch, form, st) == 5      # a d_x that d_out does not touch
        E(px, pr, po, 0, form, st)      # an empty batch: nothing launched
        M(px, po, 0, form, st)
    assert status_of(agx, E, px, pr, po, (1 << 64) - 1, COEFF, st) == 5 and status_of(agx, M, px, po, 1 << 40, NTT, st) == 5      # a batch past the grid limit
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # allowed: d_xaux inside d_x, and ranges that meet end to end (d_out right behind d_xaux, d_xaux right behind d_x)
    src, dst, m = _ranges(plan.moduli, *shape)
    x = case["x"].reshape(S, -1)
    behind = Layout(n, T, batch, offset=lr.offset + slab)
    E(px, pr, pr + w * slab, batch, COEFF, st)
    assert np.array_equal(arena.frames(behind), case["exact"]), "d_out right behind d_xaux"
    for form in (COEFF, NTT):
        E(px, px, pr + w * slab, batch, form, st)
        got = arena.frames(behind)
        want = _u64(ref.extend_exact(x.tolist(), x[0].tolist(), src, dst, m))
        assert np.array_equal(got, (want if form == COEFF else oracle_forward_set(orc, n, dst, want)).reshape(-1)), ("d_xaux is d_x's first slab", form)
        E(px, px + w * (slab // 2), pr + w * slab, batch, form, st)      # a d_xaux that straddles two source slabs
        M(px, px + w * S * slab, batch, form, st)
    dev.sync()
    aux.close(), plain.close()
    plan.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_calls_are_graph_capturable(agx, orc, dev, n):
    """both calls in both forms captured one after the other on a side stream (no parallel branches), replayed on fresh inputs"""
    torch = dev.torch
    batch, shape = 3, (0, 2, 2, 3, 5)
    T = shape[3]
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    basis = plan.basis_aux(*shape)
    cases = [_case(*_ranges(plan.moduli, *shape), batch, n, n + k) for k in (1, 2)]
    d_x, d_r = dev.to_device(cases[0]["x"]), dev.to_device(cases[0]["r"])
    d_out = {(kind, form): dev.empty(T * batch * n) for kind in ("exact", "mont") for form in (COEFF, NTT)}

    def all_calls(s):
        for form in (COEFF, NTT):
            basis.extend_exact(d_x.data_ptr(), d_r.data_ptr(), d_out["exact", form].data_ptr(), batch, form, s)
            basis.extend_mont(d_x.data_ptr(), d_out["mont", form].data_ptr(), batch, form, s)

    graph = capture(dev, all_calls, all_calls)
    for case in cases[::-1]:
        d_x.copy_(torch.from_numpy(case["lazy_x"].view(np.int64).copy()))
        d_r.copy_(torch.from_numpy(case["lazy_r"].view(np.int64).copy()))
        for d in d_out.values():
            d.zero_()
        graph.replay()
        dev.sync()
        for (kind, form), d in d_out.items():
            got = dev.to_host(d)
            if form == COEFF:
                assert np.array_equal(got, case[kind]), ("replay", kind)
            assert np.array_equal(got, _run(dev, basis, kind, case["lazy_x"], case["lazy_r"], T * batch * n, batch, form)), ("direct call", kind, form)
    basis.close()
    plan.close()


# ---- the other calls of such a basis -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_the_other_calls_equal_the_ordinary_basis_word_for_word(agx, orc, dev, n):
    batch, shape = 3, (3, 2, 0, 3, 5)
    S, T = shape[1], shape[3]
    moduli = moduli_for(orc.find_prime, n, [60, 45, 60, 54, 61, 59])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    aux, plain = plan.basis_aux(*shape), plan.basis(*shape[:4])
    assert aux.info() == plain.info() and aux.mod_down_launches() == plain.mod_down_launches()
    rng = np.random.default_rng(n)
    xp = np.stack([rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64) for q in moduli[3:5]]).reshape(-1)
    xq = np.stack([rng.integers(0, 4 * q, size=batch * n, dtype=np.uint64) for q in moduli[0:3]]).reshape(-1)
    d_xp, d_xq = dev.to_device(xp), dev.to_device(xq)
    for form in (COEFF, NTT):
        outs = []
        for basis in (aux, plain):
            d_out = dev.to_device(canary(0, T * batch * n))
            basis.extend(d_xp.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
            outs.append(dev.to_host(d_out))
        assert np.array_equal(*outs), ("extend", form)
    for mode in (agx.RESCALE_FLOOR, agx.RESCALE_ROUND):
        outs = []
        for basis in (aux, plain):
            d_out, d_scratch = dev.to_device(canary(0, T * batch * n)), dev.empty(S * batch * n)
            basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_scratch.data_ptr(), batch, dev.stream, mode)
            outs.append(dev.to_host(d_out))
        assert np.array_equal(*outs), ("mod_down", mode)
    aux.close(), plain.close()
    plan.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def test_a_bfv_multiplication_on_library_calls_decrypts(agx, orc, dev):
    """The INTEGRATION.md listing step by step at n = 64, batch 2, with the parameters of the model's test T5; keys and ciphertexts are made in Python.  Every
    coefficient of both frames decrypts to m1 m2 mod t, and the Bsk words behind step 2, the Bsk words behind step 6 and the Q words behind step 7 are the model's."""
    n, batch = 64, 2
    w = ref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    B = tuple(prime_below(orc, 1 << b, n) for b in w["B"])
    m_sk, m_tilde, t = prime_below(orc, 1 << w["m_sk"], n), prime_below(orc, 1 << w["m_tilde"], n), ref.BFV_T
    L, K = len(Q), len(B)
    Bsk, W = B + (m_sk,), L + K + 1
    moduli = Q + Bsk + (m_tilde,)      # Q = [0, L), B = [L, L + K), m_sk = L + K, m~ = L + K + 1
    assert len(set(moduli)) == W + 1
    rng = ref.Rng(2016)
    s = ref.keygen(rng, n)
    msgs = [[[rng.below(t) for _ in range(n)] for _ in range(2)] for _ in range(batch)]
    cts = [[ref.encrypt(rng, msg, s, Q, t) for msg in pair] for pair in msgs]      # [frame][operand][component][L][n]
    model = [ref.multiply(pair[0], pair[1], Q, B, m_sk, m_tilde, t) for pair in cts]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan_q, _ = plan_for_moduli(agx, orc, n, Q)          # transforms of a prime range: a plan over those primes with the same roots
    plan_bsk, _ = plan_for_moduli(agx, orc, n, Bsk)
    for sub, first in ((plan_q, 0), (plan_bsk, L)):
        assert all(sub.psi(k) == plan.psi(first + k) for k in range(sub.num_primes))
    slab, st = batch * n, dev.stream
    # the operands [2][L + K + 1][batch][n] in NTT form, their Bsk slabs still empty
    ops = np.zeros((2, 2, W, batch, n), dtype=np.uint64)
    for o in range(2):
        for c in range(2):
            coeff = _u64([[cts[f][o][c][j] for f in range(batch)] for j in range(L)])      # [L][batch][n]
            ops[o, c, :L] = oracle_forward_set(orc, n, Q, coeff).reshape(L, batch, n)
    d_ops = [dev.to_device(ops[o].reshape(-1)) for o in range(2)]
    at = lambda d, words: d.data_ptr() + 8 * words      # noqa: E731
    to_bsk = plan.basis_aux(0, L, L, K + 1, L + K + 1)
    d_coeff = dev.empty(L * slab)
    for o in range(2):
        for c in range(2):
            plan_q.inverse(at(d_ops[o], c * W * slab), d_coeff.data_ptr(), batch, st)                                         # 1
            to_bsk.extend_mont(d_coeff.data_ptr(), at(d_ops[o], (c * W + L) * slab), batch, NTT, st)                           # 2
    for o in range(2):
        got = dev.to_host(d_ops[o]).reshape(2, W, batch, n)
        for c in range(2):
            want = _u64([[model[f]["operands"][o][c][L + j] for f in range(batch)] for j in range(K + 1)])
            assert np.array_equal(got[c, L:], oracle_forward_set(orc, n, Bsk, want).reshape(K + 1, batch, n)), ("step 2", o, c)
            assert np.array_equal(got[c, :L], ops[o, c, :L]), "the Q slabs changed"
    d_tensor = dev.empty(3 * W * slab)
    plan.tensor(d_ops[0].data_ptr(), d_ops[1].data_ptr(), d_tensor.data_ptr(), batch, 0, W, st)                                # 3
    d_t = dev.to_device(np.full(W * n, t, dtype=np.uint64))
    d_floor, d_floor_coeff, d_out = dev.empty((K + 1) * slab), dev.empty((K + 1) * slab), dev.empty(L * slab)
    fast_floor = plan.basis(0, L, L, K + 1)
    to_q = plan.basis_aux(L, K, 0, L, L + K)
    out = np.empty((3, L, batch, n), dtype=np.uint64)
    for k in range(3):
        d = at(d_tensor, k * W * slab)
        plan.mul_add_galois(d_t.data_ptr(), d, d, batch, 1, 1, False, 0, W, st)                                                # 4
        fast_floor.mod_down(d + 8 * L * slab, d, d_floor.data_ptr(), d, batch, st)                                             # 5: the Q slabs are given up as the scratch
        plan_bsk.inverse(d_floor.data_ptr(), d_floor_coeff.data_ptr(), batch, st)                                              # 6
        want = _u64([[model[f]["floor"][k][j] for f in range(batch)] for j in range(K + 1)])
        assert np.array_equal(dev.to_host(d_floor_coeff), want.reshape(-1)), ("step 6", k)
        to_q.extend_exact(d_floor_coeff.data_ptr(), at(d_floor_coeff, K * slab), d_out.data_ptr(), batch, NTT, st)             # 7
        out[k] = dev.to_host(d_out).reshape(L, batch, n)
        want = _u64([[model[f]["out"][k][j] for f in range(batch)] for j in range(L)])
        assert np.array_equal(out[k], oracle_forward_set(orc, n, Q, want).reshape(L, batch, n)), ("step 7", k)
    for f in range(batch):
        coeff = [oracle_inverse_set(orc, n, Q, out[k][:, f]).tolist() for k in range(3)]
        assert ref.decrypt(coeff, s, Q, t) == ref.negacyclic(msgs[f][0], msgs[f][1], t), ("frame", f)
    for h in (to_bsk, fast_floor, to_q, plan_q, plan_bsk, plan):
        h.close()
