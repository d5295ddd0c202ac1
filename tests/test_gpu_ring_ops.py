"""agx_ntt_add, _sub, _negate, _add_galois and _tensor on the device: one streaming launch each over a range of the plan's primes.

The expected words come from Python integers (tests/ring_cases.py); every comparison is word for word, outputs go into canary-filled buffers.  The calls are
also held against the device calls they stand for (agx_ntt_pointwise, agx_ntt_automorphism), and the two compositions they complete -- a homomorphic
multiplication and a hoisted rotation -- run end to end on library calls alone."""
import functools

import numpy as np
import pytest

from gpu_util import Layout, arena_for, canary, capture, moduli_for, ntt_pi, plan_for_moduli, status_of
from ring_cases import (add_galois_ref, add_ref, hmult_case, hmult_deviation, hmult_ref, hrotate_case, hrotate_deviation, hrotate_ref, neg_ref, ring_operands,
                        sub_ref, tensor_ref)
from rns_cases import LOWER, TOP, TRIP
from rns_ref import device_residues, rotation_bound, spread

pytestmark = pytest.mark.gpu

KINDS = ("add", "sub", "negate", "add_galois", "tensor")
RANGES = ((0, 4), (1, 2), (3, 1))


def elements(n):
    """1 (the plain kernel), two small ones, -1 (conjugation) and the inverse of the rotation generator"""
    return (1, 3, 5, 2 * n - 1, pow(5, -1, 2 * n))


def call(plan, kind, pa, pb, pc, batch, first, count, g, stream):
    """the call `kind` with the arguments of all five in one order (pb and g are ignored where the call has none)"""
    if kind == "add":
        plan.add(pa, pb, pc, batch, first, count, stream)
    elif kind == "sub":
        plan.sub(pa, pb, pc, batch, first, count, stream)
    elif kind == "negate":
        plan.negate(pa, pc, batch, first, count, stream)
    elif kind == "add_galois":
        plan.add_galois(pa, pb, pc, batch, g, first, count, stream)
    else:
        plan.tensor(pa, pb, pc, batch, first, count, stream)


def reference(kind, a, b, moduli, g=1):
    """the words of `kind` on a, b [2][P][B][n] (the linear calls take component 0): [P][B][n], the tensor product [3][P][B][n]"""
    if kind == "tensor":
        return tensor_ref(a, b, moduli)
    return {"add": lambda: add_ref(a[0], b[0], moduli), "sub": lambda: sub_ref(a[0], b[0], moduli), "negate": lambda: neg_ref(a[0], moduli),
            "add_galois": lambda: add_galois_ref(a[0], b[0], moduli, g)}[kind]()


@functools.lru_cache(maxsize=None)
def _want(kind, n, moduli, batch, seed, g):
    """once per case over all of the plan's primes (read-only); a range takes its slabs"""
    a, b, _, _ = ring_operands(n, moduli, batch, seed)
    want = reference(kind, a, b, moduli, g)
    want.setflags(write=False)
    return want


def operands_of(kind, a, b, first, count):
    """the call's operands out of a, b [2][P][B][n] for the range: [count][B][n], the tensor product [2][count][B][n]"""
    pick = (lambda x: x[:, first:first + count]) if kind == "tensor" else (lambda x: x[0, first:first + count])
    return np.ascontiguousarray(pick(a)), np.ascontiguousarray(pick(b))


def want_of(kind, want, first, count):
    return np.ascontiguousarray(want[:, first:first + count] if kind == "tensor" else want[first:first + count])


def run(dev, plan, kind, a, b, batch, first, count, g=1):
    """out of place into a canary-filled c; returns the output words and checks a and b unchanged"""
    d_a, d_b = dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1))
    d_c = dev.to_device(canary(0, a.size * 3 // 2 if kind == "tensor" else a.size))
    call(plan, kind, d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, first, count, g, dev.stream)
    got = dev.to_host(d_c)
    assert np.array_equal(dev.to_host(d_a), a.reshape(-1)) and np.array_equal(dev.to_host(d_b), b.reshape(-1)), "an input changed"
    return got


def check(dev, plan, moduli, n, batch, seed, ranges, kinds=KINDS, gs=None):
    a, b, la, lb = ring_operands(n, tuple(moduli), batch, seed)
    for kind in kinds:
        for g in ((gs or elements(n)) if kind == "add_galois" else (1,)):
            want = _want(kind, n, tuple(moduli), batch, seed, g)
            for first, count in ranges:
                for name, aw, bw in (("reduced", a, b), ("spread", la, lb)):
                    x, y = operands_of(kind, aw, bw, first, count)
                    got = run(dev, plan, kind, x, y, batch, first, count, g)
                    bad = np.flatnonzero(got != want_of(kind, want, first, count).reshape(-1))
                    assert bad.size == 0, (kind, n, batch, g, (first, count), name, "first differing words", bad[:4].tolist())


# ---- parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])
def test_parity_60_bit(agx, orc, dev, n, batch):
    """all five calls on the ranges (0, 4), (1, 2) and (3, 1) of four primes: a range that does not start at 0 catches a slot served by prime `slot`"""
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    check(dev, plan, moduli, n, batch, n + batch, RANGES)
    plan.close()


def test_the_largest_frame(agx, orc, dev):
    """log_n = 15, the edge of the bit-reversal shift"""
    n, batch = 32768, 2
    moduli = moduli_for(orc.find_prime, n, [60] * 2)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    check(dev, plan, moduli, n, batch, 15, ((0, 2), (1, 1)), kinds=("add_galois", "tensor"), gs=(5,))
    plan.close()


def test_mixed_moduli(agx, orc, dev):
    n, batch = 1024, 3
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 30])
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    check(dev, plan, moduli, n, batch, 77, ((0, 4), (1, 3)), gs=(5, 2 * n - 1))
    plan.close()


def test_a_62_bit_prime(agx, orc, dev):
    """the tensor operands are all q - 1 in the first half of every frame: c_1 = 2 (q - 1)^2 mod q with q just below 2^62, reduced and spread"""
    n, batch = 1024, 3
    moduli = tuple(agx.find_primes(62, n, 1))
    q = moduli[0]
    assert q > (1 << 62) - (1 << 40)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    rng = np.random.default_rng(62)
    a, b = (rng.integers(0, q, size=(2, 1, batch, n), dtype=np.uint64) for _ in range(2))
    a[..., :n // 2] = b[..., :n // 2] = q - 1
    for kind in KINDS:
        want = reference(kind, a, b, moduli, 5)
        if kind == "tensor":
            assert int(want[1, 0, 0, 0]) == int(want[1, 0, batch - 1, n // 2 - 1]) == 2 * (q - 1) ** 2 % q
        for aw, bw in ((a, b), (spread(rng, a, moduli, 1), spread(rng, b, moduli, 1))):
            x, y = operands_of(kind, aw, bw, 0, 1)
            assert np.array_equal(run(dev, plan, kind, x, y, batch, 0, 1, 5), want.reshape(-1)), kind
    plan.close()


# ---- against the device calls they stand for, and against themselves ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 4096])
def test_identities_with_existing_calls(agx, orc, dev, n):
    batch = 5
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 60])
    P, words = len(moduli), len(moduli) * batch * n
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    a, b, la, lb = ring_operands(n, tuple(moduli), batch, n + 3)
    st = dev.stream
    # c_0 and c_2 of the tensor product are agx_ntt_pointwise on the same primes
    tensor = run(dev, plan, "tensor", la, lb, batch, 0, P).reshape(3, -1)
    d_a, d_b, d_c = dev.to_device(la.reshape(-1)), dev.to_device(lb.reshape(-1)), dev.empty(words)
    for part, half in ((0, 0), (2, 1)):
        plan.pointwise(d_a.data_ptr() + 8 * half * words, d_b.data_ptr() + 8 * half * words, d_c.data_ptr(), batch, st)
        assert np.array_equal(dev.to_host(d_c), tensor[part]), part
    # add_galois(0, b, g) is agx_ntt_automorphism(AGX_FORM_NTT, g) on reduced b
    d_zero = dev.to_device(np.zeros(words, dtype=np.uint64))
    d_x = dev.to_device(b[0].reshape(-1))
    for g in elements(n):
        plan.automorphism(d_x.data_ptr(), d_c.data_ptr(), batch, g, agx.FORM_NTT, st)
        moved = dev.to_host(d_c)
        assert np.array_equal(run(dev, plan, "add_galois", np.zeros_like(b[0]), b[0], batch, 0, P, g), moved), g
        d_out = dev.to_device(canary(0, words))
        plan.add_galois(d_zero.data_ptr(), d_x.data_ptr(), d_out.data_ptr(), batch, g, 0, P, st)
        assert np.array_equal(dev.to_host(d_out), moved), g
    # a - a = 0; -(-a) is a reduced
    assert not run(dev, plan, "sub", la[0], la[0], batch, 0, P).any()
    once = run(dev, plan, "negate", la[0], la[0], batch, 0, P).reshape(la[0].shape)
    assert np.array_equal(run(dev, plan, "negate", once, once, batch, 0, P), a[0].reshape(-1))
    plan.close()


@pytest.mark.parametrize("n", [8, 4096])
def test_allowed_aliasing(agx, orc, dev, n):
    """add with c = a, c = b and a = b = c; negate in place; add_galois with c = a; the tensor product with a = b: the out-of-place words"""
    batch, first, count, g = 5, 1, 3, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    sub = moduli[first:first + count]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, la, lb = ring_operands(n, tuple(moduli), batch, n + 9)
    x, y = operands_of("add", la, lb, first, count)
    st = dev.stream
    for kind in ("add", "sub"):
        ref = add_ref if kind == "add" else sub_ref
        for c_is in ("a", "b", "ab"):
            d_x, d_y = dev.to_device(x.reshape(-1)), dev.to_device(y.reshape(-1))
            pa, pb = d_x.data_ptr(), (d_x if c_is == "ab" else d_y).data_ptr()
            pc = pb if c_is == "b" else pa
            call(plan, kind, pa, pb, pc, batch, first, count, 1, st)
            want = ref(x, x if c_is == "ab" else y, sub).reshape(-1)
            assert np.array_equal(dev.to_host(d_y if c_is == "b" else d_x), want), (kind, c_is)
            if c_is == "a":
                assert np.array_equal(dev.to_host(d_y), y.reshape(-1))
    d_x = dev.to_device(x.reshape(-1))
    plan.negate(d_x.data_ptr(), d_x.data_ptr(), batch, first, count, st)
    assert np.array_equal(dev.to_host(d_x), neg_ref(x, sub).reshape(-1))
    for elt in (1, g, 2 * n - 1):
        d_x, d_y = dev.to_device(x.reshape(-1)), dev.to_device(y.reshape(-1))
        plan.add_galois(d_x.data_ptr(), d_y.data_ptr(), d_x.data_ptr(), batch, elt, first, count, st)
        assert np.array_equal(dev.to_host(d_x), add_galois_ref(x, y, sub, elt).reshape(-1)), elt
        assert np.array_equal(dev.to_host(d_y), y.reshape(-1))
    d_y = dev.to_device(y.reshape(-1))      # g = 1 is add: c may be b
    d_x = dev.to_device(x.reshape(-1))
    plan.add_galois(d_x.data_ptr(), d_y.data_ptr(), d_y.data_ptr(), batch, 1, first, count, st)
    assert np.array_equal(dev.to_host(d_y), add_ref(x, y, sub).reshape(-1))
    t, _ = operands_of("tensor", la, lb, first, count)
    d_t, d_c = dev.to_device(t.reshape(-1)), dev.to_device(canary(0, 3 * x.size))
    plan.tensor(d_t.data_ptr(), d_t.data_ptr(), d_c.data_ptr(), batch, first, count, st)
    assert np.array_equal(dev.to_host(d_c), tensor_ref(t, t, sub).reshape(-1))
    assert np.array_equal(dev.to_host(d_t), t.reshape(-1))
    plan.close()


# ---- placement ------------------------------------------------------------------------------------------------------------------
def layouts(n, batch, slabs, offsets):
    """frame sets of slabs[k] `primes` each, one behind the other with a gap, set k at a word of parity offsets[k]"""
    out, at = [], 0
    for count, parity in zip(slabs, offsets):
        at += (at % 2 != parity % 2)
        out.append(Layout(n, count, batch, offset=at))
        at = out[-1].span() + 6
    return out


@pytest.mark.parametrize("offsets", [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0)], ids=["16-byte", "odd", "c odd", "b odd", "a odd"])
@pytest.mark.parametrize("n,batch", [(8, 5), (4096, 3)])
def test_alignment_and_guard_bands(agx, orc, dev, n, batch, offsets):
    """every base 16-byte aligned (the pair form), every base at an odd word, exactly one base odd (the pair form must not be taken): the same words,
    the operands unchanged, and every word outside c still canary"""
    first, count, g = 1, 3, 5
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 60])
    sub = moduli[first:first + count]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    _, _, la, lb = ring_operands(n, tuple(moduli), batch, n + 11)
    for kind in KINDS:
        x, y = operands_of(kind, la, lb, first, count)
        want = reference(kind, x, y, sub, g) if kind == "tensor" else reference(kind, x[None], y[None], sub, g)
        k = 2 if kind == "tensor" else 1
        lx, ly, lc = layouts(n, batch, (k * count, k * count, (3 if kind == "tensor" else 1) * count), offsets)
        arena = arena_for(dev, n, (lx, x), (ly, y), (lc, None))
        assert arena.address(0) % 16 == 0
        call(plan, kind, arena.address(lx.offset), arena.address(ly.offset), arena.address(lc.offset), batch, first, count, g, dev.stream)
        img = arena.image()
        assert not arena.faults([(lx, x), (ly, y), (lc, None)], img), ("a word outside c changed", kind, offsets)
        assert np.array_equal(arena.frames(lc, img), want.reshape(-1)), (kind, offsets)
    plan.close()


# ---- argument rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_rejected_calls_write_nothing(agx, orc, dev, n):
    batch, g = 2, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 3)
    P = len(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    a, b, _, _ = ring_operands(n, tuple(moduli), batch, 5 * n)
    lx, ly, lc = layouts(n, batch, (2 * P, 2 * P, 3 * P), (0, 0, 0))      # room for the tensor product; the linear calls use the head of each
    arena = arena_for(dev, n, (lx, a), (ly, b), (lc, None))
    before = arena.image()
    pa, pb, pc = (arena.address(l.offset) for l in (lx, ly, lc))
    st, w, slab = dev.stream, 8, batch * n
    C = lambda kind, *args: status_of(agx, call, plan, kind, *args)      # noqa: E731
    for kind in KINDS:
        words = (2 if kind == "tensor" else 1) * P * slab
        assert C(kind, pa, pb, pc, batch, 0, 0, g, st) == 5, kind                                   # prime_count = 0
        for first, count in ((0, P + 1), (1, P), (P, 1), (P + 1, 0), (0xffffffff, 2), (2, 0xffffffff)):      # a range past P
            assert C(kind, pa, pb, pc, batch, first, count, g, st) == 5, (kind, first, count)
        for k in range(3):                                                                          # NULL and misaligned pointers
            if kind == "negate" and k == 1:
                continue
            null, odd = [pa, pb, pc], [pa, pb, pc]
            null[k], odd[k] = 0, odd[k] + 4
            assert C(kind, *null, batch, 0, P, g, st) == 1, (kind, k)
            assert C(kind, *null, batch, 0, 0, 4, st) == 1, (kind, k)                               # the NULL rule comes first
            assert C(kind, *odd, batch, 0, P, g, st) == 5, (kind, k)
        assert C(kind, pa, pb, pc, 1 << 40, 0, P, g, st) == 5, kind                                 # a batch past the grid limit
        assert C(kind, pa, pb, pc, (1 << 64) - 1, 0, P, g, st) == 5, kind
        # partial overlap of c with a: c's first word is a's last, c's last word is a's first, c one word into a
        out_words = (3 if kind == "tensor" else 1) * P * slab
        for at in (pa + w * (words - 1), pa - w * (out_words - 1), pa + w, pa - w):
            assert C(kind, pa, pb, at, batch, 0, P, g, st) == 5, (kind, hex(at - pa))
        if kind != "negate":
            for at in (pb + w * (words - 1), pb - w * (out_words - 1), pb + w):
                assert C(kind, pa, pb, at, batch, 0, P, g, st) == 5, (kind, hex(at - pb))
    assert C("add_galois", pa, pb, pb, batch, 0, P, g, st) == 5                                     # c touching b with g != 1, equal pointers included
    assert C("add_galois", pa, pb, pb, batch, 0, P, 2 * n - 1, st) == 5
    assert C("tensor", pa, pb, pa, batch, 0, P, g, st) == 5                                         # the tensor product in place
    assert C("tensor", pa, pb, pb, batch, 0, P, g, st) == 5
    assert C("tensor", pa, pa, pa, batch, 0, P, g, st) == 5
    for elt in (0, 2, 4, 2 * n - 2, 2 * n, 2 * n + 1, 4 * n + 5, 0xfffffffe, 0xffffffff):           # even, 0, 2n, 2n + 1 and beyond
        assert C("add_galois", pa, pb, pc, batch, 0, P, elt, st) == 5, elt
        assert C("add_galois", pa, pb, pc, 0, 0, P, elt, st) == 5, elt                              # also with an empty batch
    for kind in KINDS:                                                                              # batch = 0: AGX_OK, nothing launched
        assert C(kind, pa, pb, pc, 0, 0, P, g, st) == 0, kind
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # ranges that meet end to end do not touch: a | b | c back to back
    for kind in ("add_galois", "tensor"):
        x, y = operands_of(kind, a, b, 0, P)
        k, out = (2, 3) if kind == "tensor" else (1, 1)
        lo = Layout(n, out * P, batch, offset=2 * k * P * slab)
        packed = arena_for(dev, n, (Layout(n, k * P, batch, offset=0), x), (Layout(n, k * P, batch, offset=k * P * slab), y), (lo, None))
        base = packed.address(0)
        call(plan, kind, base, base + w * k * P * slab, base + w * 2 * k * P * slab, batch, 0, P, g, st)
        assert np.array_equal(packed.frames(lo), _want(kind, n, tuple(moduli), batch, 5 * n, g).reshape(-1)), kind
    plan.close()


def test_every_plan_serves(agx, orc, dev):
    """a forward-only plan and every variant give the same words: the calls read the plan's constants and nothing else"""
    n, batch = 4096, 3
    moduli = moduli_for(orc.find_prime, n, [60] * 4)
    for inverse in (False, True):
        plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=inverse)
        for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2, agx.VARIANT_REGBLOCK):
            plan.set_variant(variant)
            check(dev, plan, moduli, n, batch, 4099, ((1, 3),), gs=(5,))
        plan.close()


# ---- a second grid-stride step of each width -----------------------------------------------------------------------------------------------
def _second_step(agx, orc, dev, batch, odd):
    """n = 4096, two 60-bit primes, every word judged on the device in int64: sums of residues stay below 2^61; the tensor product's b is drawn from
    {0, 1, 2, 3}, so every product and the cross sum stay below 6q < 2^63 and a mis-indexed word of b still shows with probability 3/4.
    odd: a's base 8 bytes past a 16-byte boundary, so that the word form runs; otherwise every base 16-byte aligned (the pair form)"""
    torch = dev.torch
    n, g = 4096, 5
    moduli = moduli_for(orc.find_prime, n, [60] * 2)
    P = len(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    shift = 1 if odd else 0
    two = tuple(moduli) + tuple(moduli)      # [2][P] slabs
    d_a = torch.cat([dev.empty(shift), device_residues(torch, dev, two, batch, n, 1)])
    d_b, d_small = device_residues(torch, dev, two, batch, n, 2), device_residues(torch, dev, two, batch, n, 3, bound=4)
    d_c = dev.empty(3 * P * batch * n)
    assert all(t.data_ptr() % 16 == 0 for t in (d_a, d_b, d_small, d_c))
    pa = d_a.data_ptr() + 8 * shift
    av, bv, sv = d_a[shift:].view(2, P, batch, n), d_b.view(2, P, batch, n), d_small.view(2, P, batch, n)
    pi = torch.from_numpy(ntt_pi(n, g)).to(dev.device)

    def judge(what, part, want_of_prime):
        cv = d_c.view(3, P, batch, n)[part]
        for p, q in enumerate(moduli):
            want = want_of_prime(p) % int(q)
            if not torch.equal(cv[p], want):
                pytest.fail(f"{what}: prime {p}, first differing (frame, word) {(cv[p] != want).nonzero()[:4].tolist()}")

    d_c.fill_(-1)
    plan.add(pa, d_b.data_ptr(), d_c.data_ptr(), batch, 0, P, dev.stream)
    dev.sync()
    judge("add", 0, lambda p: av[0, p] + bv[0, p])
    assert int(d_c[P * batch * n]) == -1, "the word behind c changed"
    d_c.fill_(-1)
    plan.add_galois(pa, d_b.data_ptr(), d_c.data_ptr(), batch, g, 0, P, dev.stream)
    dev.sync()
    judge("add_galois", 0, lambda p: av[0, p] + bv[0, p][:, pi])
    assert int(d_c[P * batch * n]) == -1, "the word behind c changed"
    d_c.fill_(-1)
    plan.tensor(pa, d_small.data_ptr(), d_c.data_ptr(), batch, 0, P, dev.stream)
    dev.sync()
    judge("tensor c_0", 0, lambda p: av[0, p] * sv[0, p])
    judge("tensor c_1", 1, lambda p: av[0, p] * sv[1, p] + av[1, p] * sv[0, p])
    judge("tensor c_2", 2, lambda p: av[1, p] * sv[1, p])
    plan.close()


def test_second_step_pair_form_every_word(agx, orc, dev):
    """2,051 frames of 2,048 pairs pass the 16,384 x 256 work items of one sweep"""
    assert 2051 * (4096 // 2) > TRIP
    _second_step(agx, orc, dev, 2051, False)


def test_second_step_word_form_every_word(agx, orc, dev):
    """one base odd: one word per work item, so 1,025 frames pass one sweep"""
    assert 1025 * 4096 > TRIP
    _second_step(agx, orc, dev, 1025, True)


# ---- end to end: a homomorphic multiplication and a hoisted rotation on library calls alone ---------------------------------------------------------
N_E2E, BATCH_E2E = 1024, 2


def _hmult_buffers(dev, ks, a, b, key, q_count):
    slab = q_count * BATCH_E2E * N_E2E
    return (dev.to_device(a.reshape(-1)), dev.to_device(b.reshape(-1)), dev.to_device(key.reshape(-1)), dev.to_device(canary(0, 3 * slab)),
            dev.to_device(canary(0, 2 * slab)), dev.empty(ks.scratch_words(BATCH_E2E)))


def _hmult(plan, ks, bufs, q_count, stream):
    """tensor -> agx_ntt_keyswitch_apply on the c_2 slabs -> out_0 += d_0, out_1 += d_1, everything on `stream`"""
    d_a, d_b, d_key, d_d, d_out, d_s = (t.data_ptr() for t in bufs)
    slab = 8 * q_count * BATCH_E2E * N_E2E
    plan.tensor(d_a, d_b, d_d, BATCH_E2E, 0, q_count, stream)
    ks.apply(d_d + 2 * slab, d_key, d_out, d_s, BATCH_E2E, stream)
    plan.add(d_out, d_d, d_out, BATCH_E2E, 0, q_count, stream)
    plan.add(d_out + slab, d_d + slab, d_out + slab, BATCH_E2E, 0, q_count, stream)


@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
def test_hmult_end_to_end(agx, orc, dev, shape):
    """word-equal to the reference composition, within the noise condition, and the same words from a captured graph replayed twice"""
    n, batch, q_count = N_E2E, BATCH_E2E, shape[0]
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    a, b, key, s, shat, mhat, mhat2 = hmult_case(orc, n, tuple(moduli), shape, batch, 4000 + sum(shape))
    want = hmult_ref(orc, n, moduli, shape, a, b, key, batch)
    bufs = _hmult_buffers(dev, ks, a, b, key, q_count)
    _hmult(plan, ks, bufs, q_count, dev.stream)
    got = dev.to_host(bufs[4])
    assert np.array_equal(got, want.reshape(-1)), ("first differing words", np.flatnonzero(got != want.reshape(-1))[:4].tolist())
    assert np.array_equal(dev.to_host(bufs[0]), a.reshape(-1)) and np.array_equal(dev.to_host(bufs[1]), b.reshape(-1)), "a ciphertext changed"
    worst, bound = hmult_deviation(orc, n, moduli, shape, batch, got, shat, mhat, mhat2), rotation_bound(shape, s)
    print(f"hmult {shape}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, worst, bound)
    # captured on one stream (no parallel branches), replayed twice
    graph = capture(dev, lambda st: _hmult(plan, ks, bufs, q_count, st), lambda st: _hmult(plan, ks, bufs, q_count, st))
    for _ in range(2):
        bufs[3].fill_(-1)
        bufs[4].fill_(-1)
        graph.replay()
        assert np.array_equal(dev.to_host(bufs[4]), want.reshape(-1)), "replay"
    ks.close()
    plan.close()


@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
def test_hrotate_end_to_end(agx, orc, dev, shape):
    """decompose -> apply_decomposed(g = 5) -> add_galois in place on out_0: the reference's words, within rotation_bound of sigma_g(m)"""
    n, batch, q_count, g = N_E2E, BATCH_E2E, shape[0], 5
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    c, key, s, shat, mhat = hrotate_case(orc, n, tuple(moduli), shape, g, batch, 5000 + sum(shape))
    want = hrotate_ref(orc, n, moduli, shape, c, key, batch, g)
    slab = q_count * batch * n
    ext_words, decompose_words, apply_words = ks.hoisted_words(batch)
    d_c, d_key, d_out = dev.to_device(c.reshape(-1)), dev.to_device(key.reshape(-1)), dev.to_device(canary(0, 2 * slab))
    d_ext, d_s = dev.empty(ext_words), dev.empty(max(decompose_words, apply_words))
    st = dev.stream
    ks.decompose(d_c.data_ptr() + 8 * slab, d_ext.data_ptr(), d_s.data_ptr(), batch, st)
    ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, g, st)
    plan.add_galois(d_out.data_ptr(), d_c.data_ptr(), d_out.data_ptr(), batch, g, 0, q_count, st)
    got = dev.to_host(d_out)
    assert np.array_equal(got, want.reshape(-1)), ("first differing words", np.flatnonzero(got != want.reshape(-1))[:4].tolist())
    assert np.array_equal(dev.to_host(d_c), c.reshape(-1)), "the ciphertext changed"
    worst, bound = hrotate_deviation(orc, n, moduli, shape, g, batch, got, shat, mhat), rotation_bound(shape, s)
    print(f"hrotate {shape}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, worst, bound)
    ks.close()
    plan.close()
