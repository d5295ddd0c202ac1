"""Every call at moduli away from the top of their arithmetic class (tests/modulus_cases.py): the primes next to each bound a class predicate compares
against, mid-width primes (36 ... 54 bits), the smallest admitted primes, and plans of six that mix them -- a 5-bit prime next to a 62-bit one, estimate
and four-step primes in one 16q-lazy launch, narrow-looking plans that the 64-bit kernels must serve.

The expected words come from the CPU oracle (transforms) and from Python integers (rns_ref.py, ring_cases.py); every comparison is word for word.  Inputs
are spread over [0, 4q) wherever the call admits lazy inputs (over [0, 3q) under a prime above 2^61), and every prime's first frame opens with 0, q - 1
and the top of that range.  Plans come from the oracle's tables; once per mix and size also from the library's own, and both must write the same words."""
import functools

import numpy as np
import pytest

from gpu_util import (PRODUCT_IDS, Q60C_REGISTRY, REGISTRY, canary, ntt_pi, oracle_forward_rns, oracle_polymul, oracle_tables, plan_for_moduli, radix2_twin,
                      rescale_reference, sigma)
from modulus_cases import MIX_NAMES, MIXES, edge_bounds, edge_moduli, expected_class
from ring_cases import add_galois_ref, add_ref, neg_ref, ring_operands, sub_ref, tensor_ref
from rns_cases import LOWER, TOP, keyswitch_case, run_keyswitch
from rns_ref import (apply_decomposed_ref, convert, decompose_ref, inner_ref, mod_down_ntt, oracle_forward_set, oracle_inverse_set)

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
FLOOR, ROUND = 0, 1
EDGE_NAMES = tuple(edge_bounds())
SIZES = (8, 64, 1024, 4096, 16384, 32768)      # the smallest size of each kernel family, and the sizes with kernels of their own
BY_ID = {e[0]: e for e in REGISTRY + Q60C_REGISTRY}
Q60C_IDS = {e[0] for e in Q60C_REGISTRY}


def seed_of(n, name, salt=0):
    return n * 1000 + sum(map(ord, name)) + salt


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def cap(q):
    """the multiples of q inputs are spread over: [0, 4q), [0, 3q) under a prime above 2^61"""
    return 3 if q > 1 << 61 else 4


def lazy(rng, x, moduli, axis=0):
    """the same residues spread over [0, cap(q) q), the shape kept; `axis` is the prime axis of x"""
    shape = [1] * x.ndim
    shape[axis] = len(moduli)
    k = np.minimum(rng.integers(0, 4, size=x.shape, dtype=np.uint64), np.array([cap(q) - 1 for q in moduli], dtype=np.uint64).reshape(shape))
    return x + np.array(moduli, dtype=np.uint64).reshape(shape) * k


def draw(rng, moduli, batch, n):
    """(x, lx) [P][batch][n]: residues below q_p and the same spread; every prime's first frame opens with 0, q - 1 and, in lx, the top of the range"""
    q = np.array(moduli, dtype=np.uint64)
    x = np.stack([rng.integers(0, int(m), size=(batch, n), dtype=np.uint64) for m in moduli])
    x[:, 0, 0] = 0
    x[:, 0, 1:3] = (q - np.uint64(1))[:, None]
    lx = lazy(rng, x, moduli)
    lx[:, 0, :2] = x[:, 0, :2]
    lx[:, 0, 2] = q * np.array([cap(m) for m in moduli], dtype=np.uint64) - np.uint64(1)
    return x, lx


def first_bad(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
    return bad[:4].tolist(), np.asarray(got).reshape(-1)[bad[:4]].tolist(), np.asarray(want).reshape(-1)[bad[:4]].tolist()


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.size == want.size and np.array_equal(got, want), (what, "first differing words", first_bad(got, want))


# ---- (a) routing --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_default_plans_choose_the_expected_class(agx, orc, dev, n):
    """every single edge modulus and every mix: the registry entry a default plan reports is a product entry of this size whose class is the smallest
    that admits every modulus, for a small batch and for one past every forward companion's threshold; the companion for moduli 2^60 - c, 0 < c < 2^28,
    exactly where every modulus is one (c_max is, c_out is not)"""
    plans = [(name, (q,)) for name, q in edge_moduli(orc, n).items()] + list(MIXES(orc, n).items())
    for name, moduli in plans:
        plan = agx.Plan(n, list(moduli))
        for batch in (3, 5000):
            config = plan.forward_kernel(batch)
            assert config in PRODUCT_IDS | Q60C_IDS and BY_ID[config][1] == n, (n, name, batch, config)
            if (n, batch) == (4096, 5000):
                assert (config in Q60C_IDS) == all(0 < (1 << 60) - q < 1 << 28 for q in moduli), (n, name, batch, config)
            else:
                assert config not in Q60C_IDS, (n, name, batch, config)
            assert BY_ID[config][2] == expected_class(n, moduli), (n, name, batch, config)
            if name == "above31":
                assert BY_ID[config][2] not in (30, 31), (n, name, config)
            if name == "above60":
                assert BY_ID[config][2] != 60, (n, name, config)
        plan.close()


# ---- (b), (c) the transforms and products of one plan -------------------------------------------------------------------------------------------
def check_transforms(agx, orc, dev, plan, tabs, n, batch, seed, what):
    """forward (out of place, in place), forward_lazy, inverse (in place, out of place), pointwise, polymul and polymul_ntt with bhat_batch = batch and
    1, all on spread operands, against the oracle"""
    P = len(tabs)
    moduli = [t[0] for t in tabs]
    rng = np.random.default_rng(seed)
    x, lx = draw(rng, moduli, batch, n)
    r, lr = draw(rng, moduli, batch, n)
    qcol = np.array(moduli, dtype=np.uint64)[:, None]
    size = P * batch * n
    want = oracle_forward_rns(orc, x, tabs, n)
    d_x, d_y = dev.to_device(lx.reshape(-1)), dev.to_device(canary(0, size))
    plan.forward(d_x.data_ptr(), d_y.data_ptr(), batch, dev.stream)
    same(dev.to_host(d_y), want, (what, "forward"))
    same(dev.to_host(d_x), lx, (what, "forward changed its input"))
    plan.forward_lazy(d_x.data_ptr(), d_y.data_ptr(), batch, dev.stream)
    got = dev.to_host(d_y).reshape(P, -1)
    assert (got < qcol * np.uint64(4)).all(), (what, "forward_lazy left the range [0, 4q)")      # 4q < 2^64 for every admitted q
    same(got % qcol, want, (what, "forward_lazy"))
    plan.forward(d_x.data_ptr(), d_x.data_ptr(), batch, dev.stream)
    same(dev.to_host(d_x), want, (what, "forward in place"))
    # the inverse of arbitrary (not forward-image) words
    want_inv = oracle_inverse_set(orc, n, tuple(moduli), r)
    d_r, d_o = dev.to_device(lr.reshape(-1)), dev.to_device(canary(0, size))
    plan.inverse(d_r.data_ptr(), d_o.data_ptr(), batch, dev.stream)
    same(dev.to_host(d_o), want_inv, (what, "inverse"))
    plan.inverse(d_r.data_ptr(), d_r.data_ptr(), batch, dev.stream)
    same(dev.to_host(d_r), want_inv, (what, "inverse in place"))
    # products
    d_a, d_b, d_c, d_s = dev.to_device(lx.reshape(-1)), dev.to_device(lr.reshape(-1)), dev.to_device(canary(0, size)), dev.empty(size)
    plan.pointwise(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, dev.stream)
    same(dev.to_host(d_c), np.stack([orc.pointwise(x[p].reshape(-1), r[p].reshape(-1), q) for p, q in enumerate(moduli)]), (what, "pointwise"))
    want_mul = np.stack([oracle_polymul(orc, x[p].reshape(-1), r[p].reshape(-1), t[0], t[1], n) for p, t in enumerate(tabs)])
    plan.polymul(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    same(dev.to_host(d_c), want_mul, (what, "polymul"))
    d_bhat = dev.empty(size)
    plan.forward_lazy(d_b.data_ptr(), d_bhat.data_ptr(), batch, dev.stream)
    d_c.fill_(-1)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, batch, dev.stream)
    same(dev.to_host(d_c), want_mul, (what, "polymul_ntt, one bhat frame per frame"))
    r0 = np.ascontiguousarray(r[:, :1])
    d_b0, d_bhat0 = dev.to_device(r0.reshape(-1)), dev.empty(P * n)
    plan.forward(d_b0.data_ptr(), d_bhat0.data_ptr(), 1, dev.stream)
    d_c.fill_(-1)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat0.data_ptr(), d_c.data_ptr(), batch, 1, dev.stream)
    want_one = np.stack([oracle_polymul(orc, x[p].reshape(-1), np.tile(r0[p].reshape(-1), batch), t[0], t[1], n) for p, t in enumerate(tabs)])
    same(dev.to_host(d_c), want_one, (what, "polymul_ntt, one bhat frame per prime"))
    same(dev.to_host(d_a), lx, (what, "a product changed its operand"))
    return lx, want


@pytest.mark.parametrize("name", EDGE_NAMES)
@pytest.mark.parametrize("n", SIZES)
def test_single_modulus_plans(agx, orc, dev, n, name):
    """each edge modulus decides its class alone"""
    q = edge_moduli(orc, n)[name]
    plan, tabs = plan_for_moduli(agx, orc, n, (q,))
    check_transforms(agx, orc, dev, plan, tabs, n, 3, seed_of(n, name), (n, name, q))
    plan.close()


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", SIZES[:5])
def test_transforms_on_every_mix(agx, orc, dev, n, name):
    """the dense layout through every call; a plan made from the library's own tables writes the same words; a strided [poly][prime][n] layout at an odd
    offset (frames 8-byte aligned only), the gaps untouched"""
    batch, P = 3, 6
    moduli = MIXES(orc, n)[name]
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    lx, want = check_transforms(agx, orc, dev, plan, tabs, n, batch, seed_of(n, name), (n, name))
    own = agx.Plan(n, list(moduli))
    assert [own.psi(p) for p in range(P)] == [t[1] for t in tabs]
    d = dev.to_device(lx.reshape(-1))
    own.forward(d.data_ptr(), d.data_ptr(), batch, dev.stream)
    same(dev.to_host(d), want, (n, name, "forward, the library's tables"))
    own.inverse(d.data_ptr(), d.data_ptr(), batch, dev.stream)
    same(dev.to_host(d), lx % np.array(moduli, dtype=np.uint64)[:, None, None], (n, name, "round trip, the library's tables"))
    own.close()
    poly_stride, prime_stride, off = P * n + 12, n + 2, 1
    idx = (off + np.arange(P)[:, None, None] * prime_stride + np.arange(batch)[None, :, None] * poly_stride + np.arange(n)[None, None, :]).reshape(-1)
    buf = canary(3, off + batch * poly_stride)
    expect = buf.copy()
    buf[idx], expect[idx] = lx.reshape(-1), want
    d = dev.to_device(buf)
    ptr = d.data_ptr() + 8 * off
    plan.forward_strided(ptr, ptr, batch, prime_stride, poly_stride, dev.stream)
    same(dev.to_host(d), expect, (n, name, "forward_strided"))
    plan.inverse_strided(ptr, ptr, batch, prime_stride, poly_stride, dev.stream)
    expect[idx] = (lx % np.array(moduli, dtype=np.uint64)[:, None, None]).reshape(-1)
    same(dev.to_host(d), expect, (n, name, "inverse_strided"))
    plan.close()


# ---- (d) the RNS calls: cases computed once, shared with (e) ------------------------------------------------------------------------------------
RNS_SIZES = (64, 1024, 4096)
FUSED_SIZES = RNS_SIZES + (16384,)      # rescale, extend and ModDown have two-launch routes of their own up to the largest sizes


def batch_of(n):
    return 3 if n <= 4096 else 2


def orders_of(moduli):
    """the mix as given, rotated so that its smallest prime is the dropped last modulus, and rotated so that its widest is"""
    lo, hi = moduli.index(min(moduli)), moduli.index(max(moduli))
    out = [moduli, moduli[lo + 1:] + moduli[:lo + 1], moduli[hi + 1:] + moduli[:hi + 1]]
    return [m for k, m in enumerate(out) if m not in out[:k]]


@functools.lru_cache(maxsize=None)
def rescale_case(orc, n, moduli, batch, seed):
    """(xhat, xhat spread, {mode: expected words [P-1][batch][n]}), flat: any residues are NTT-form frames; the reference divides their CRT lift"""
    xhat, lhat = draw(np.random.default_rng(seed), moduli, batch, n)
    res = oracle_inverse_set(orc, n, moduli, xhat)
    want = {mode: oracle_forward_set(orc, n, moduli[:-1], rescale_reference(res, moduli, mode)).reshape(-1) for mode in (FLOOR, ROUND)}
    out = (xhat.reshape(-1), lhat.reshape(-1), want)
    for w in (out[0], out[1], *want.values()):
        w.setflags(write=False)
    return out


def run_rescale(dev, plan, words, batch, n, mode, in_place):
    P = plan.num_primes
    d_x = dev.to_device(words)
    if in_place:
        plan.rescale(d_x.data_ptr(), d_x.data_ptr(), d_x.data_ptr() + 8 * (P - 1) * batch * n, batch, mode, dev.stream)
        return dev.to_host(d_x)[:(P - 1) * batch * n]
    d_out, d_s = dev.to_device(canary(0, (P - 1) * batch * n)), dev.empty(batch * n)
    plan.rescale(d_x.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, mode, dev.stream)
    assert np.array_equal(dev.to_host(d_x), words), "x changed"
    return dev.to_host(d_out)


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", FUSED_SIZES)
def test_rescale_on_every_mix(agx, orc, dev, n, name):
    """floor and round, in place and not, reduced and spread inputs; the three orders give ratios q_L / q_i from 2^-46 (the smallest prime dropped from
    under 62-bit ones) to 2^46"""
    batch = batch_of(n)
    for k, moduli in enumerate(orders_of(MIXES(orc, n)[name])):
        plan, _ = plan_for_moduli(agx, orc, n, moduli)
        xhat, lhat, want = rescale_case(orc, n, moduli, batch, seed_of(n, name, k))
        for mode in (FLOOR, ROUND):
            for words, in_place in ((xhat, False), (lhat, False), (lhat, True), (xhat, True)):
                same(run_rescale(dev, plan, words, batch, n, mode, in_place), want[mode], (n, name, "order", k, "mode", mode, "in place", in_place))
        plan.close()


def extend_shapes(moduli):
    """(source first, source count, target first, target count): S = 1, 2 and 4 sources at either end into the remaining primes, and the smallest and
    the widest prime alone into the longer side of the rest -- a tiny source under 62-bit targets and the reverse"""
    out = [(0, 1, 1, 5), (5, 1, 0, 5), (0, 2, 2, 4), (4, 2, 0, 4), (0, 4, 4, 2), (2, 4, 0, 2)]
    for i in (moduli.index(min(moduli)), moduli.index(max(moduli))):
        out.append((i, 1, 0, i) if i >= 3 else (i, 1, i + 1, 5 - i))
    return [s for k, s in enumerate(out) if s not in out[:k]]


@functools.lru_cache(maxsize=None)
def extend_case(orc, n, moduli, shape, batch, seed):
    """(x, x spread, {form: expected words [T][batch][n]}), flat; x in coefficient form"""
    sf, S, df, T = shape
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    x, lx = draw(np.random.default_rng(seed), src, batch, n)
    coeff = convert(x, src, dst)
    want = {COEFF: coeff.reshape(-1), NTT: oracle_forward_set(orc, n, dst, coeff).reshape(-1)}
    out = (x.reshape(-1), lx.reshape(-1), want)
    for w in (out[0], out[1], *want.values()):
        w.setflags(write=False)
    return out


def run_extend(dev, plan, shape, words, batch, n, form):
    basis = plan.basis(*shape)
    d_x, d_out = dev.to_device(words), dev.to_device(canary(0, shape[3] * batch * n))
    basis.extend(d_x.data_ptr(), d_out.data_ptr(), batch, form, dev.stream)
    got = dev.to_host(d_out)
    assert np.array_equal(dev.to_host(d_x), words), "x changed"
    basis.close()
    return got


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", FUSED_SIZES)
def test_basis_extend_on_every_mix(agx, orc, dev, n, name):
    batch = batch_of(n)
    moduli = MIXES(orc, n)[name]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for shape in extend_shapes(moduli):
        x, lx, want = extend_case(orc, n, moduli, shape, batch, seed_of(n, name, shape[0] + 7 * shape[1]))
        for form in (COEFF, NTT):
            for words in (lx, x):
                same(run_extend(dev, plan, shape, words, batch, n, form), want[form], (n, name, shape, "form", form))
    plan.close()


MODDOWN_SHAPES = ((5, 1, 0, 5), (4, 2, 0, 4))


@functools.lru_cache(maxsize=None)
def moddown_case(orc, n, moduli, shape, batch, seed):
    """(xq, xp, both spread, the expected words [T][batch][n]), flat: any residues are NTT-form frames"""
    sf, S, df, T = shape
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    rng = np.random.default_rng(seed)
    xq, lq = draw(rng, dst, batch, n)
    xp, lp = draw(rng, src, batch, n)
    out = (xq.reshape(-1), xp.reshape(-1), lq.reshape(-1), lp.reshape(-1), mod_down_ntt(orc, n, xq, xp, src, dst).reshape(-1))
    for w in out:
        w.setflags(write=False)
    return out


def run_moddown(dev, plan, shape, xq, xp, batch, in_place):
    basis = plan.basis(*shape)
    d_xq, d_xp = dev.to_device(xq), dev.to_device(xp)
    if in_place:
        basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_xq.data_ptr(), d_xp.data_ptr(), batch, dev.stream)
        got = dev.to_host(d_xq)
    else:
        d_out, d_s = dev.to_device(canary(0, xq.size)), dev.empty(xp.size)
        basis.mod_down(d_xq.data_ptr(), d_xp.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream)
        got = dev.to_host(d_out)
        assert np.array_equal(dev.to_host(d_xq), xq) and np.array_equal(dev.to_host(d_xp), xp), "an input changed"
    basis.close()
    return got


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", FUSED_SIZES)
def test_basis_mod_down_on_every_mix(agx, orc, dev, n, name):
    """S = 1 and 2 special primes, in place (the sources given up as the scratch) and not, reduced and spread inputs"""
    batch = batch_of(n)
    moduli = MIXES(orc, n)[name]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for shape in MODDOWN_SHAPES:
        xq, xp, lq, lp, want = moddown_case(orc, n, moduli, shape, batch, seed_of(n, name, shape[1]))
        for q_words, p_words, in_place in ((lq, lp, False), (xq, xp, False), (lq, lp, True)):
            same(run_moddown(dev, plan, shape, q_words, p_words, batch, in_place), want, (n, name, shape, "in place", in_place))
    plan.close()


@functools.lru_cache(maxsize=None)
def inner_case(n, moduli, batch, seed):
    """(a [3][P][batch][n], b [3][2][P][batch][n]) spread over the lazy range, and {(g, broadcast): the expected words [2][P][batch][n]}"""
    rng = np.random.default_rng(seed)
    top = np.array(moduli, dtype=np.uint64) - np.uint64(1)
    a = np.stack([rng.integers(0, q, size=(3, batch, n), dtype=np.uint64) for q in moduli], axis=1)
    b = np.stack([rng.integers(0, q, size=(3, 2, batch, n), dtype=np.uint64) for q in moduli], axis=2)
    a[0, :, 0, 0] = 0
    a[:, :, 0, 1:3] = b[:, :, :, 0, 1:3] = top[:, None]      # three terms of (q - 1)^2
    want = {}
    for g in (1, 5):
        ag = np.ascontiguousarray(a[..., ntt_pi(n, g)])
        want[g, False], want[g, True] = inner_ref(ag, b, moduli), inner_ref(ag, np.ascontiguousarray(b[:, :, :, :1]), moduli)
    la, lb = lazy(rng, a, moduli, 1), lazy(rng, b, moduli, 2)
    la[:, :, 0, 2] = lb[:, :, :, 0, 2] = (top + np.uint64(1)) * np.array([cap(q) for q in moduli], dtype=np.uint64) - np.uint64(1)
    for w in (la, lb, *want.values()):
        w.setflags(write=False)
    return la, lb, want


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", RNS_SIZES)
def test_inner_products_on_every_mix(agx, orc, dev, n, name):
    """inner_product and inner_product_galois (g = 5): 3 terms, 2 outputs, the key per frame and broadcast"""
    batch, terms, outputs = 3, 3, 2
    moduli = MIXES(orc, n)[name]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    la, lb, want = inner_case(n, moduli, batch, seed_of(n, name))
    d_a = dev.to_device(la.reshape(-1))
    for broadcast in (False, True):
        d_b = dev.to_device(np.ascontiguousarray(lb[:, :, :, :1] if broadcast else lb).reshape(-1))
        bb = 1 if broadcast else batch
        d_c = dev.to_device(canary(0, outputs * 6 * batch * n))
        plan.inner_product(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, outputs, bb, dev.stream)
        same(dev.to_host(d_c), want[1, broadcast], (n, name, "inner_product", "broadcast", broadcast))
        d_c = dev.to_device(canary(0, outputs * 6 * batch * n))
        plan.inner_product_galois(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, terms, 5, outputs, bb, dev.stream)
        same(dev.to_host(d_c), want[5, broadcast], (n, name, "inner_product_galois", "broadcast", broadcast))
    same(dev.to_host(d_a), la, (n, name, "a changed"))
    plan.close()


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", RNS_SIZES)
def test_key_switch_on_every_mix(agx, orc, dev, n, name):
    """keyswitch_apply on the shapes TOP and LOWER, then decompose and apply_decomposed with g = 5, against keyswitch_ref and the two halves of
    hoisted_ref.  Parity only: the noise conditions need wide moduli and are not asserted here"""
    batch, g = 2, 5
    moduli = MIXES(orc, n)[name]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    for shape in (TOP, LOWER):
        chat, key, lchat, lkey, want = keyswitch_case(orc, n, moduli, shape, batch, seed_of(n, name, shape[0]))
        ks = plan.keyswitch(*shape)
        same(run_keyswitch(dev, ks, lchat, lkey, batch), want, (n, name, shape, "apply, spread"))
        same(run_keyswitch(dev, ks, chat, key, batch), want, (n, name, shape, "apply, reduced"))
        ext = decompose_ref(orc, n, moduli, shape, chat)
        ext_words, scratch_words, apply_words = ks.hoisted_words(batch)
        d_chat, d_ext, d_s = dev.to_device(lchat), dev.to_device(canary(0, ext_words)), dev.empty(scratch_words)
        ks.decompose(d_chat.data_ptr(), d_ext.data_ptr(), d_s.data_ptr(), batch, dev.stream)
        same(dev.to_host(d_ext), ext, (n, name, shape, "decompose"))
        d_key, d_out, d_s2 = dev.to_device(lkey), dev.to_device(canary(0, want.size)), dev.empty(apply_words)
        ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_s2.data_ptr(), batch, g, dev.stream)
        same(dev.to_host(d_out), apply_decomposed_ref(orc, n, moduli, shape, ext, key, batch, g), (n, name, shape, "apply_decomposed"))
        same(dev.to_host(d_ext), ext, (n, name, shape, "ext changed"))
        ks.close()
    plan.close()


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", RNS_SIZES)
def test_ring_calls_on_every_mix(agx, orc, dev, n, name):
    """add, sub, negate, add_galois (g = 5) and tensor over the prime range [1, 5), reduced and spread operands"""
    batch, first, count, g = 3, 1, 4, 5
    moduli = MIXES(orc, n)[name]
    sub = moduli[first:first + count]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    a, b, la, lb = ring_operands(n, moduli, batch, seed_of(n, name))
    pick = lambda x: np.ascontiguousarray(x[:, first:first + count])      # noqa: E731
    ra, rb = pick(a), pick(b)
    wants = {"add": add_ref(ra[0], rb[0], sub), "sub": sub_ref(ra[0], rb[0], sub), "negate": neg_ref(ra[0], sub),
             "add_galois": add_galois_ref(ra[0], rb[0], sub, g), "tensor": tensor_ref(ra, rb, sub)}
    slab = count * batch * n
    for label, aw, bw in (("spread", pick(la), pick(lb)), ("reduced", ra, rb)):
        d_a, d_b = dev.to_device(aw.reshape(-1)), dev.to_device(bw.reshape(-1))      # [2][count][batch][n]: component 0 leads
        pa, pb, st = d_a.data_ptr(), d_b.data_ptr(), dev.stream
        for kind in wants:
            d_c = dev.to_device(canary(0, 3 * slab if kind == "tensor" else slab))
            pc = d_c.data_ptr()
            {"add": lambda: plan.add(pa, pb, pc, batch, first, count, st), "sub": lambda: plan.sub(pa, pb, pc, batch, first, count, st),
             "negate": lambda: plan.negate(pa, pc, batch, first, count, st), "add_galois": lambda: plan.add_galois(pa, pb, pc, batch, g, first, count, st),
             "tensor": lambda: plan.tensor(pa, pb, pc, batch, first, count, st)}[kind]()
            same(dev.to_host(d_c), wants[kind], (n, name, kind, label))
        same(dev.to_host(d_a), aw, (n, name, "a changed"))
    plan.close()


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", RNS_SIZES)
def test_automorphism_on_every_mix(agx, orc, dev, n, name):
    """both forms, g = 5 and 2n - 1: the coefficient form on spread inputs against the definition, the NTT form on the oracle's transform of the same
    frames against the oracle's transform of their image"""
    batch = 3
    moduli = MIXES(orc, n)[name]
    plan, tabs = plan_for_moduli(agx, orc, n, moduli)
    a, la = draw(np.random.default_rng(seed_of(n, name)), moduli, batch, n)
    d_a, d_ahat = dev.to_device(la.reshape(-1)), dev.to_device(oracle_forward_rns(orc, a, tabs, n))
    for g in (5, 2 * n - 1):
        image = np.stack([sigma(a[p], g, n, q) for p, q in enumerate(moduli)])
        d_out = dev.to_device(canary(0, a.size))
        plan.automorphism(d_a.data_ptr(), d_out.data_ptr(), batch, g, COEFF, dev.stream)
        same(dev.to_host(d_out), image, (n, name, g, "coefficient form"))
        d_out = dev.to_device(canary(0, a.size))
        plan.automorphism(d_ahat.data_ptr(), d_out.data_ptr(), batch, g, NTT, dev.stream)
        same(dev.to_host(d_out), oracle_forward_rns(orc, image, tabs, n), (n, name, g, "NTT form"))
    same(dev.to_host(d_a), la, (n, name, "the input changed"))
    plan.close()


# ---- (e) the generic multi-launch route writes the same words -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ckks40", "edge60", "edge61", "edge62"])
@pytest.mark.parametrize("n", [1024, 4096])
def test_the_generic_route_agrees(agx, orc, dev, n, name):
    """rescale, extend to NTT form, ModDown and the key switch on gpu_util.radix2_twin(plan) against the default route and the reference"""
    batch = batch_of(n)
    moduli = MIXES(orc, n)[name]
    plan = agx.Plan(n, list(moduli), psi=[oracle_tables(orc, n, q)[1] for q in moduli])      # radix2_twin copies the roots: a plan made from roots
    twin = radix2_twin(agx, plan)
    assert twin.forward_kernel(batch) == -1 and plan.forward_kernel(batch) != -1
    xhat, lhat, want = rescale_case(orc, n, moduli, batch, seed_of(n, name, 0))
    for mode in (FLOOR, ROUND):
        routes = [run_rescale(dev, p, lhat, batch, n, mode, False) for p in (plan, twin)]
        same(routes[1], routes[0], (n, name, "rescale, the routes differ", mode))
        same(routes[1], want[mode], (n, name, "rescale, generic route", mode))
    for shape in ((5, 1, 0, 5), (4, 2, 0, 4)):
        x, lx, want = extend_case(orc, n, moduli, shape, batch, seed_of(n, name, shape[0] + 7 * shape[1]))
        routes = [run_extend(dev, p, shape, lx, batch, n, NTT) for p in (plan, twin)]
        same(routes[1], routes[0], (n, name, "extend, the routes differ", shape))
        same(routes[1], want[NTT], (n, name, "extend, generic route", shape))
    shape = MODDOWN_SHAPES[1]
    xq, xp, lq, lp, want = moddown_case(orc, n, moduli, shape, batch, seed_of(n, name, shape[1]))
    routes = [run_moddown(dev, p, shape, lq, lp, batch, False) for p in (plan, twin)]
    same(routes[1], routes[0], (n, name, "ModDown, the routes differ"))
    same(routes[1], want, (n, name, "ModDown, generic route"))
    chat, key, lchat, lkey, want = keyswitch_case(orc, n, moduli, TOP, 2, seed_of(n, name, TOP[0]))
    routes = []
    for p in (plan, twin):
        ks = p.keyswitch(*TOP)
        routes.append(run_keyswitch(dev, ks, lchat, lkey, 2))
        ks.close()
    same(routes[1], routes[0], (n, name, "key switch, the routes differ"))
    same(routes[1], want, (n, name, "key switch, generic route"))
    twin.close()
    plan.close()
