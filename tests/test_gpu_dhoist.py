"""The double-hoisted linear transform on the device: agx_ntt_keyswitch_accumulate_decomposed (the inner-product half of apply_decomposed, weighted and
accumulating), agx_ntt_keyswitch_mod_down (its ModDown half) and agx_ntt_mul_add_galois (the multiply-accumulate on a range of primes with a broadcast
operand).  The reference is tests/dhoist_ref.py, Python integers on top of rns_ref.py; every comparison is word for word.  Every operand set of the two
streaming calls is placed in a guarded arena once at 16-byte bases (the pair kernels) and once with one base at 8 mod 16 (the word kernels); the words
around the output must stay as they were."""
import functools

import numpy as np
import pytest

from dhoist_ref import accumulate_ref, linear_transform_ref, mul_add_ref, rotation_keys, transform_deviation
from gpu_util import Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, status_of
from rns_cases import LOWER, SHAPE_IDS, SHAPES, TOP, keyswitch_case
from rns_ref import active_of, apply_decomposed_ref, decompose_ref, digits_of, rotation_bound, spread

pytestmark = pytest.mark.gpu

WEIGHTS = ("none", "one-frame", "per-frame")


def elements(n):
    return (1, 5, 2 * n - 1)


def sizes_of(shape, n, batch):
    """(ext, key, acc, out, weight per frame) in words, from the header's formulas"""
    q_count, A, D = shape[0], shape[0] + shape[2], len(digits_of(shape))
    slab = batch * n
    return D * A * slab, D * 2 * A * n, 2 * A * slab, 2 * q_count * slab, A * n


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


@functools.lru_cache(maxsize=None)
def _operands(orc, n, moduli, shape, batch, seed):
    """the operands of every accumulate case of one shape, drawn once (read-only): ext [D][A][batch n] as decompose writes it; per element a key
    [D][2][A][n] spread over [0, 4q); weights [A][1][n] and [A][batch][n] spread likewise; an old acc [2][A][batch n] of lazy words"""
    active = active_of(moduli, shape)
    A, D = len(active), len(digits_of(shape))
    rng = np.random.default_rng(seed)
    ext = decompose_ref(orc, n, moduli, shape, keyswitch_case(orc, n, moduli, shape, batch, seed)[0])
    keys = {g: spread(rng, np.stack([rng.integers(0, int(q), size=(D, 2, n), dtype=np.uint64) for q in active], axis=2), active, axis=2) for g in elements(n)}
    weights = {"none": None}
    for name, frames in (("one-frame", 1), ("per-frame", batch)):
        w = np.stack([rng.integers(0, int(q), size=(frames, n), dtype=np.uint64) for q in active])
        w[:, 0, 0], w[:, 0, 1] = 0, np.array(active, dtype=np.uint64) - np.uint64(1)      # a zero weight and the largest one
        weights[name] = spread(rng, w, active, axis=0)
    old = spread(rng, np.stack([rng.integers(0, int(q), size=(2, batch * n), dtype=np.uint64) for q in active], axis=1), active, axis=1)
    old[:, :, 0] = 4 * np.array(active, dtype=np.uint64)[None, :] - np.uint64(1)      # the top of the lazy range
    for a in (ext, old, *keys.values(), *[w for w in weights.values() if w is not None]):
        a.setflags(write=False)
    return ext, keys, weights, old


def run_accumulate(dev, ks, n, shape, batch, ext, key, weight, old, g, odd=None):
    """one accumulate_decomposed call in a guarded arena, ext | key | weight | acc each behind a gap, all at 16-byte bases or operand number `odd` at 8 mod
    16; checks every word outside acc unchanged (the inputs and the guards) and returns acc's words"""
    A, D = shape[0] + shape[2], len(digits_of(shape))
    layouts, at = [], 0
    for k, (primes, frames) in enumerate(((D * A, batch), (D * 2 * A, 1), (A, 1 if weight is None else weight.size // (A * n)), (2 * A, batch))):
        at += 6
        at += (at % 2) != (1 if odd == k else 0)
        layouts.append(Layout(n, primes, frames, offset=at))
        at = layouts[-1].span()
    le, lk, lw, la = layouts
    placed = [(le, ext), (lk, key), (la, old)] + ([(lw, weight)] if weight is not None else [])
    arena = arena_for(dev, n, *placed)
    ks.accumulate_decomposed(arena.address(le.offset), arena.address(lk.offset), arena.address(la.offset), batch, g,
                             None if weight is None else arena.address(lw.offset), None if weight is None else lw.batch, old is not None, dev.stream)
    img = arena.image()
    unchanged = [(le, ext), (lk, key), (la, None)] + ([(lw, weight)] if weight is not None else [])
    faults = arena.faults(unchanged, img)
    assert not faults, ("a word outside acc changed", odd, faults)
    return arena.frames(la, img)


def _check_accumulate(agx, orc, dev, n, moduli, shape, batch, seed):
    """every element x weight kind x accumulate against accumulate_ref, each at 16-byte bases and with one base (taken in turn) at 8 mod 16"""
    moduli = tuple(moduli)
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)      # no inverse tables are needed
    ks = plan.keyswitch(*shape)
    ext, keys, weights, old = _operands(orc, n, moduli, shape, batch, seed)
    turn = 0
    for g in elements(n):
        for kind in WEIGHTS:
            for acc_old in (None, old):
                want = accumulate_ref(n, moduli, shape, ext, keys[g], weights[kind], acc_old, batch, g).reshape(-1)
                operands = 4 if kind != "none" else 3
                for odd in (None, [0, 1, 3, 2][turn % operands]):
                    got = run_accumulate(dev, ks, n, shape, batch, ext, keys[g], weights[kind], None if acc_old is None else acc_old.copy(), g, odd)
                    assert np.array_equal(got, want), (n, shape, batch, g, kind, acc_old is not None, odd, "first differing words", _first_bad(got, want))
                turn += 1
    ks.close()
    plan.close()


# ---- accumulate_decomposed word for word -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n,batch", [(8, 5), (64, 5), (1024, 3), (4096, 2)])
def test_accumulate_decomposed_against_the_reference(agx, orc, dev, n, batch, shape):
    _check_accumulate(agx, orc, dev, n, moduli_for(orc.find_prime, n, [60] * 6), shape, batch, n * 7 + batch + shape[0])


@pytest.mark.parametrize("n,widths", [(64, [30] * 6), (1024, [60, 30, 61, 30, 60, 60])], ids=["30-bit-64", "mixed-1024"])
def test_accumulate_decomposed_other_moduli(agx, orc, dev, n, widths):
    _check_accumulate(agx, orc, dev, n, moduli_for(orc.find_prime, n, widths), TOP, 5, n + widths[1])


# ---- identities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_the_two_halves_are_apply_decomposed(agx, orc, dev, n, shape):
    """accumulate_decomposed(w = NULL, accumulate = 0, g) then keyswitch_mod_down equals apply_decomposed(g) word for word -- on the device and against
    rns_ref.apply_decomposed_ref -- under the plan's own routes and under AGX_VARIANT_LDS_RADIX2, where ModDown takes its four-launch route; mod_down
    leaves acc's Q slabs as they were"""
    batch = 3
    moduli = tuple(moduli_for(orc.find_prime, n, [60] * 6))
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    q_count, A = shape[0], shape[0] + shape[2]
    ext, keys, _, _ = _operands(orc, n, moduli, shape, batch, n + 41)
    ext_w, key_w, acc_w, out_w, _ = sizes_of(shape, n, batch)
    d_ext = dev.to_device(ext)
    for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2):
        plan.set_variant(variant)
        for g in elements(n):
            d_key = dev.to_device(keys[g])
            d_acc, d_out, d_whole, d_scratch = dev.to_device(canary(0, acc_w)), dev.to_device(canary(0, out_w)), dev.to_device(canary(7, out_w)), dev.empty(acc_w)
            ks.accumulate_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_acc.data_ptr(), batch, g, stream=dev.stream)
            acc = dev.to_host(d_acc).reshape(2, A, batch * n)
            assert np.array_equal(acc, accumulate_ref(n, moduli, shape, ext, keys[g], None, None, batch, g))
            ks.mod_down(d_acc.data_ptr(), d_out.data_ptr(), batch, dev.stream)
            ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_whole.data_ptr(), d_scratch.data_ptr(), batch, g, dev.stream)
            got, whole = dev.to_host(d_out), dev.to_host(d_whole)
            assert np.array_equal(got, whole), (n, shape, variant, g, "first differing words", _first_bad(got, whole))
            assert np.array_equal(got, apply_decomposed_ref(orc, n, moduli, shape, ext, keys[g], batch, g).reshape(-1)), (n, shape, variant, g)
            assert np.array_equal(dev.to_host(d_acc).reshape(2, A, -1)[:, :q_count], acc[:, :q_count]), "mod_down changed a Q slab of acc"
        assert ks.hoisted_info()[1] == 1 + 2 * plan.basis(shape[1], shape[2], 0, q_count).mod_down_launches()
    assert np.array_equal(dev.to_host(d_ext).reshape(-1), ext.reshape(-1)), "ext changed"
    ks.close()
    plan.close()


def _ring_words(n, moduli, batch, seed):
    """(w one frame, w per frame, b, c old) over `moduli`, spread over [0, 4q), with the edge words in front"""
    rng = np.random.default_rng(seed)
    q = np.array(moduli, dtype=np.uint64)
    out = []
    for frames in (1, batch, batch, batch):
        x = np.stack([rng.integers(0, int(m), size=(frames, n), dtype=np.uint64) for m in moduli])
        x[:, 0, 0], x[:, 0, 1] = 0, q - np.uint64(1)
        x = spread(rng, x, moduli, axis=0)
        x[:, -1, -1] = 4 * q - np.uint64(1)
        out.append(x)
    return out


@pytest.mark.parametrize("n", [8, 64, 4096])
def test_mul_add_galois_is_the_calls_it_generalises(agx, orc, dev, n):
    batch = 3
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 30, 60, 60] if n >= 1024 else [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    P = len(moduli)
    _, w, b, old = _ring_words(n, moduli, batch, n + 5)
    q = np.array(moduli, dtype=np.uint64)[:, None, None]
    d_w, d_b, d_ones = dev.to_device(w), dev.to_device(b), dev.to_device(np.ones(P * n, dtype=np.uint64))
    d_c, d_ref = dev.to_device(canary(0, b.size)), dev.to_device(canary(3, b.size))
    # g = 1, accumulate = 0, a weight per frame, the whole plan: agx_ntt_pointwise
    plan.mul_add_galois(d_w.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, stream=dev.stream)
    plan.pointwise(d_w.data_ptr(), d_b.data_ptr(), d_ref.data_ptr(), batch, dev.stream)
    assert np.array_equal(dev.to_host(d_c), dev.to_host(d_ref)), "pointwise"
    for g in elements(n):
        # w = 1, accumulate = 0: agx_ntt_automorphism(AGX_FORM_NTT, g), reduced
        plan.mul_add_galois(d_ones.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, g, w_batch=1, stream=dev.stream)
        plan.automorphism(d_b.data_ptr(), d_ref.data_ptr(), batch, g, agx.FORM_NTT, dev.stream)
        assert np.array_equal(dev.to_host(d_c).reshape(P, batch, n), dev.to_host(d_ref).reshape(P, batch, n) % q), ("automorphism", g)
        # w = 1, accumulate = 1: agx_ntt_add_galois
        d_c.copy_(dev.to_device(old.reshape(-1)))
        d_old = dev.to_device(old)
        plan.mul_add_galois(d_ones.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), batch, g, w_batch=1, accumulate=True, stream=dev.stream)
        plan.add_galois(d_old.data_ptr(), d_b.data_ptr(), d_ref.data_ptr(), batch, g, stream=dev.stream)
        assert np.array_equal(dev.to_host(d_c), dev.to_host(d_ref)), ("add_galois", g)
    plan.close()


# ---- mul_add_galois against Python integers ----------------------------------------------------------------------------------------------
def run_mul_add(dev, plan, n, count, first, batch, w, b, old, g, odd=None, in_place=False):
    """one call in a guarded arena, w | b | c each behind a gap, all at 16-byte bases or operand number `odd` at 8 mod 16 (in place: c is b); checks
    every word outside c unchanged and returns c's words"""
    layouts, at = [], 0
    for k, frames in enumerate((w.size // (count * n), batch, batch)):
        at += 6
        at += (at % 2) != (1 if odd == k else 0)
        layouts.append(Layout(n, count, frames, offset=at))
        at = layouts[-1].span()
    lw, lb, lc = layouts
    if in_place:
        lc = lb
    placed = [(lw, w), (lb, b)] + ([(lc, old)] if old is not None and not in_place else [])
    arena = arena_for(dev, n, *placed, (lc, None))
    plan.mul_add_galois(arena.address(lw.offset), arena.address(lb.offset), arena.address(lc.offset), batch, g, lw.batch, old is not None, first, count, dev.stream)
    img = arena.image()
    faults = arena.faults([(lw, w), (lc, None)] + ([] if in_place else [(lb, b)]), img)
    assert not faults, ("a word outside c changed", odd, faults)
    return arena.frames(lc, img)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 8, 64, 4096])
def test_mul_add_galois_against_integers(agx, orc, dev, n, batch):
    """the ranges (0, P), (1, 2), (P - 1, 1) x g x {one weight frame, one per frame} x accumulate, each at 16-byte bases and with one base (taken in turn)
    at 8 mod 16; and c == b in place at g = 1"""
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61, 30, 60, 60] if n >= 1024 else [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    P = len(moduli)
    w1, wb, b, old = _ring_words(n, moduli, batch, 31 * n + batch)
    turn = 0
    for first, count in ((0, P), (1, 2), (P - 1, 1)):
        sub = moduli[first:first + count]
        cut = lambda x: np.ascontiguousarray(x[first:first + count])      # noqa: E731
        for g in sorted({1, 3, 2 * n - 1} | ({5} if n > 2 else set())):      # every one odd and below 2n
            for w in (cut(w1), cut(wb)):
                for c_old in (None, cut(old)):
                    want = mul_add_ref(n, sub, w, cut(b), c_old, batch, g).reshape(-1)
                    for odd in (None, turn % 3):
                        got = run_mul_add(dev, plan, n, count, first, batch, w, cut(b), c_old, g, odd)
                        assert np.array_equal(got, want), (n, batch, first, count, g, w.shape, c_old is not None, odd, _first_bad(got, want))
                    turn += 1
        want = mul_add_ref(n, sub, cut(w1), cut(b), None, batch, 1).reshape(-1)
        for odd in (None, 1):      # in place at g = 1: c IS b
            assert np.array_equal(run_mul_add(dev, plan, n, count, first, batch, cut(w1), cut(b), None, 1, odd, in_place=True), want), (n, batch, first, count, odd)
    plan.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [TOP, LOWER], ids=["top", "lower"])
@pytest.mark.parametrize("n", [64, 1024])
def test_a_linear_transform_end_to_end(agx, orc, dev, n, shape):
    """out = sum_r w_r o sigma_{g_r}(ct) + w_0 o ct for R = 3 rotation keys that share one s, as INTEGRATION.md lists it: decompose, three accumulates, ONE
    keyswitch_mod_down, three gathered multiply-adds of c0 and the unrotated diagonal on c0 and c1.  Word for word against linear_transform_ref, and the
    result decrypts to the transform of the plaintext within p_count (1 + ||s||_1): a condition, not a measurement"""
    batch = 2
    gs = (5, 2 * n - 1, 25)
    moduli = tuple(moduli_for(orc.find_prime, n, [60] * 6))
    active = active_of(moduli, shape)
    q_count, A = shape[0], len(active)
    Q = active[:q_count]
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    rng = np.random.default_rng(n + sum(shape))
    c0, c1 = (np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in Q]) for _ in range(2))
    s, shat, keys = rotation_keys(orc, n, moduli, shape, gs, 3000 + n + sum(shape))
    weight = lambda: np.stack([rng.integers(0, int(q), size=(1, n), dtype=np.uint64) for q in active])      # noqa: E731
    rotations = [(g, keys[g], weight()) for g in gs]
    diagonal = weight()
    want = linear_transform_ref(orc, n, moduli, shape, decompose_ref(orc, n, moduli, shape, c1), rotations, batch, c0, c1, diagonal)
    ext_w, scratch_w, acc_w = ks.hoisted_words(batch)
    d_c0, d_c1, d_ext, d_scr, d_acc = dev.to_device(c0), dev.to_device(c1), dev.empty(ext_w), dev.empty(scratch_w), dev.to_device(canary(0, acc_w))
    d_out = dev.to_device(canary(0, 2 * c0.size))
    out0, out1, st = d_out.data_ptr(), d_out.data_ptr() + 8 * c0.size, dev.stream
    d_keys, d_ws, d_diag = [dev.to_device(k) for _, k, _ in rotations], [dev.to_device(w) for _, _, w in rotations], dev.to_device(diagonal)
    ks.decompose(d_c1.data_ptr(), d_ext.data_ptr(), d_scr.data_ptr(), batch, st)
    for r, (g, _, _) in enumerate(rotations):
        ks.accumulate_decomposed(d_ext.data_ptr(), d_keys[r].data_ptr(), d_acc.data_ptr(), batch, g, d_ws[r].data_ptr(), 1, r > 0, st)
    ks.mod_down(d_acc.data_ptr(), out0, batch, st)      # one ModDown pair for the whole sum
    for r, (g, _, _) in enumerate(rotations):           # out_0 += w_r o sigma_g(c0): the weight's first q_count slabs are the weight under Q
        plan.mul_add_galois(d_ws[r].data_ptr(), d_c0.data_ptr(), out0, batch, g, 1, True, 0, q_count, st)
    plan.mul_add_galois(d_diag.data_ptr(), d_c0.data_ptr(), out0, batch, 1, 1, True, 0, q_count, st)
    plan.mul_add_galois(d_diag.data_ptr(), d_c1.data_ptr(), out1, batch, 1, 1, True, 0, q_count, st)
    got = dev.to_host(d_out)
    ks.close()
    plan.close()
    assert np.array_equal(got, want.reshape(-1)), (n, shape, "first differing words", _first_bad(got, want.reshape(-1)))
    worst = transform_deviation(orc, n, moduli, shape, batch, c1, shat, got, rotations, c0, diagonal)
    bound = rotation_bound(shape, s)
    print(f"n = {n}, shape {shape}: worst deviation {worst}, bound {bound}")
    assert worst <= bound, (n, shape, worst, bound)


# ---- argument rules ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(64, TOP), (4096, LOWER)])
def test_rejected_keyswitch_calls_write_nothing(agx, orc, dev, n, shape):
    """one case per rule of the two status orders, each rule in front of the one that follows it; acc and out pre-filled and compared afterwards"""
    batch, g = 2, 5
    moduli = tuple(moduli_for(orc.find_prime, n, [60] * 6))
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    fwd_only, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    ks, no_inverse = plan.keyswitch(*shape), fwd_only.keyswitch(*shape)
    ext, keys, weights, old = _operands(orc, n, moduli, shape, batch, 3 * n)
    ext_w, key_w, acc_w, out_w, w_w = sizes_of(shape, n, batch)
    A, slab = shape[0] + shape[2], batch * n
    le = Layout(n, ext_w // slab, batch, offset=0)
    lk = Layout(n, key_w // n, 1, offset=le.span() + 2 * n)
    lw = Layout(n, A, batch, offset=lk.span() + 2 * n)
    la = Layout(n, acc_w // slab, batch, offset=lw.span() + 2 * n)
    lo = Layout(n, out_w // slab, batch, offset=la.span() + 2 * n)
    arena = arena_for(dev, n, (le, ext), (lk, keys[g]), (lw, weights["per-frame"]), (la, old), (lo, None))
    before = arena.image()
    pe, pk, pw, pa, po = (arena.address(l.offset) for l in (le, lk, lw, la, lo))
    st, w8 = dev.stream, 8
    acc = lambda k=ks, e=pe, key=pk, a=pa, b=batch, elt=g, wt=pw, wb=batch, ac=1: status_of(agx, k.accumulate_decomposed, e, key, a, b, elt, wt, wb, ac, st)      # noqa: E731
    down = lambda k=ks, a=pa, o=po, b=batch: status_of(agx, k.mod_down, a, o, b, st)      # noqa: E731
    # accumulate_decomposed: 1. NULL (a NULL weight is w = 1 and no error: below)
    assert acc(e=0) == 1 and acc(key=0) == 1 and acc(a=0) == 1
    assert acc(e=0, b=1 << 62) == 1 and acc(a=0, wb=7, ac=2, elt=4) == 1                      # in front of rules 2, 3 and 5
    # 2. the 2^60 limits
    assert acc(b=1 << 55) == 5 and acc(b=(1 << 64) - 1) == 5
    assert acc(b=1 << 55, wb=1 << 55) == 5                                                    # weight_batch == batch there: rule 2 alone
    # 3. weight_batch and accumulate, in front of the alignment and the overlap rule
    for wb in (0, 3, batch + 1, (1 << 64) - 1):
        assert acc(wb=wb) == 5, wb
    assert acc(ac=2) == 5 and acc(ac=-1) == 5 and acc(wb=1, ac=2, e=pe + 1) == 5
    assert acc(wt=0, wb=7, b=0) == 0                                                          # a NULL weight: weight_batch is ignored
    # 4. alignment, the grid limits, any two touching
    ptrs, sizes, names = [pe, pk, pw, pa], [ext_w, key_w, A * slab, acc_w], ["e", "key", "wt", "a"]
    for name, p in zip(names, ptrs):
        for off in (1, 4):
            assert acc(**{name: p + off}) == 5, (name, off)
    assert acc(b=1 << 40, wb=1 << 40) == 5 and acc(b=(1 << 31) - 1, wb=(1 << 31) - 1) == 5
    for i in range(4):
        for j in range(4):
            if i != j:
                for at in (ptrs[i], ptrs[i] + w8 * (sizes[i] - 1), ptrs[i] - w8 * (sizes[j] - 1)):
                    assert acc(**{names[j]: at}) == 5, (i, j, at - ptrs[i])
    assert acc(wt=pa + w8 * (acc_w - 1), wb=1) == 5 and acc(wt=pa - w8 * (A * n - 1), wb=1) == 5      # the one-frame weight's own extent
    assert acc(key=pe, elt=4) == 5                                                             # in front of rule 5
    # 5. the Galois element, in front of the empty batch
    for elt in (0, 2, 2 * n - 2, 2 * n, 2 * n + 1, 0xffffffff):
        assert acc(elt=elt) == 5 and acc(elt=elt, b=0, wb=0) == 5, elt
    # 7. an empty batch; a forward-only plan serves
    assert acc(b=0, wb=0) == 0 and acc(b=0, wb=1) == 0
    # mod_down: NULL; the limits; alignment, the grids, acc and out touching; no inverse tables; an empty batch
    assert down(a=0) == 1 and down(o=0) == 1 and down(a=0, b=1 << 62) == 1
    assert down(b=1 << 55) == 5 and down(b=(1 << 64) - 1) == 5 and down(b=1 << 40) == 5 and down(b=(1 << 31) - 1) == 5
    for off in (1, 4):
        assert down(a=pa + off) == 5 and down(o=po + off) == 5
    for at in (pa, pa + w8 * (acc_w - 1), pa - w8 * (out_w - 1)):
        assert down(o=at) == 5, at - pa
    assert down(k=no_inverse) == 9 and down(k=no_inverse, o=pa) == 5                           # the overlap rule comes first
    assert down(k=no_inverse, b=0) == 9 and down(b=0) == 0                                     # the missing inverse in front of the empty batch
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # accepted: the forward-only plan accumulates; ext | key | weight | acc and acc | out back to back
    want = accumulate_ref(n, moduli, shape, ext, keys[g], weights["per-frame"], old, batch, g).reshape(-1)
    assert acc(k=no_inverse) == 0
    assert np.array_equal(arena.frames(la), want)
    offs = [0, ext_w, ext_w + key_w, ext_w + key_w + A * slab, ext_w + key_w + A * slab + acc_w]
    packed = arena_for(dev, n, (le.at(offs[0]), ext), (lk.at(offs[1]), keys[g]), (lw.at(offs[2]), weights["per-frame"]), (la.at(offs[3]), old), (lo.at(offs[4]), None))
    ks.accumulate_decomposed(packed.address(offs[0]), packed.address(offs[1]), packed.address(offs[3]), batch, g, packed.address(offs[2]), batch, True, st)
    assert np.array_equal(packed.frames(la.at(offs[3])), want)
    ks.mod_down(packed.address(offs[3]), packed.address(offs[4]), batch, st)
    assert not packed.faults([(le.at(offs[0]), ext), (lk.at(offs[1]), keys[g]), (lw.at(offs[2]), weights["per-frame"]), (la.at(offs[3]), None), (lo.at(offs[4]), None)])
    for h in (ks, no_inverse, plan, fwd_only):
        h.close()


@pytest.mark.parametrize("n", [64, 4096])
def test_rejected_mul_add_calls_write_nothing(agx, orc, dev, n):
    """agx_ntt_add_galois's status order with the w_batch and accumulate rules beside the range rule"""
    batch, g, first, count = 2, 5, 1, 3
    moduli = moduli_for(orc.find_prime, n, [60] * 6)
    plan, _ = plan_for_moduli(agx, orc, n, moduli, inverse=False)
    P, words = len(moduli), 3 * batch * n
    cut = lambda x: np.ascontiguousarray(x[first:first + count])      # noqa: E731
    w1, wb, b, old = (cut(x) for x in _ring_words(n, moduli, batch, n + 77))
    lw, lb, lc = Layout(n, count, batch, offset=0), Layout(n, count, batch, offset=words + 2 * n), Layout(n, count, batch, offset=2 * words + 4 * n)
    arena = arena_for(dev, n, (lw, wb), (lb, b), (lc, old))
    pw, pb, pc = (arena.address(l.offset) for l in (lw, lb, lc))
    st, w8 = dev.stream, 8
    call = lambda w=pw, v=pb, c=pc, bt=batch, elt=g, k=batch, ac=1, f=first, cnt=count: status_of(agx, plan.mul_add_galois, w, v, c, bt, elt, k, ac, f, cnt, st)      # noqa: E731
    assert call(w=0) == 1 and call(v=0) == 1 and call(c=0) == 1 and call(c=0, cnt=0, k=7, ac=2, elt=4) == 1      # NULL in front of everything
    for f, cnt in ((0, 0), (0, P + 1), (P, 1), (P - 1, 2), (1, 0xffffffff), (0xffffffff, 2)):                    # the range
        assert call(f=f, cnt=cnt) == 5, (f, cnt)
    for k in (0, 3, batch + 1, (1 << 64) - 1):                                                               # w_batch
        assert call(k=k) == 5, k
    assert call(ac=2) == 5 and call(ac=-1) == 5                                                              # accumulate
    assert call(cnt=0, w=pw + 1) == 5 and call(k=3, c=pc + 4) == 5 and call(ac=2, c=pb) == 5                 # beside the range rule, in front of the next rules
    for name, p in (("w", pw), ("v", pb), ("c", pc)):                                                        # alignment
        for off in (1, 4):
            assert call(**{name: p + off}) == 5, (name, off)
    assert call(bt=1 << 40, k=1 << 40) == 5 and call(bt=(1 << 64) - 1, k=1) == 5                              # the grid limit, an extent past 2^60
    for at in (pc, pc + w8 * (words - 1), pc - w8 * (words - 1)):                                            # c touches w or b
        assert call(w=at) == 5 and call(v=at) == 5, at - pc
    assert call(w=pc + w8 * (words - 1), k=1) == 5 and call(w=pc - w8 * (count * n - 1), k=1) == 5           # the one-frame weight's own extent
    assert call(v=pc, elt=1, bt=0, k=0) == 0                                                                 # g = 1: c may be exactly b
    assert call(v=pc + w8, elt=1) == 5 and call(v=pc, elt=3) == 5                                            # but no partial overlap, and no other element
    assert call(v=pc, elt=4) == 5 and call(w=pb) == 0                                                        # overlap in front of the element; w and b may overlap
    want = mul_add_ref(n, moduli[first:first + count], b, b, old, batch, g).reshape(-1)
    assert np.array_equal(arena.frames(lc), want)                                                            # that last call ran: w was b
    for elt in (0, 2, 2 * n - 2, 2 * n, 2 * n + 1, 0xffffffff):                                              # the Galois element, in front of the empty batch
        assert call(elt=elt) == 5 and call(elt=elt, bt=0, k=0) == 5, elt
    assert call(bt=0, k=0) == 0 and call(bt=0, k=1) == 0
    dev.sync()
    after = arena.image()
    assert not arena.faults([(lw, wb), (lb, b), (lc, want)], after), "a rejected call wrote memory"
    plan.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(64, TOP), (4096, LOWER)])
def test_the_chain_is_graph_capturable(agx, orc, dev, n, shape):
    """accumulate x 2 -> mod_down -> mul_add_galois as ONE linear chain on one stream: captured, replayed twice on fresh inputs, equal to the eager words"""
    torch = dev.torch
    batch = 3
    gs = (5, 2 * n - 1)
    moduli = tuple(moduli_for(orc.find_prime, n, [60] * 6))
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    ks = plan.keyswitch(*shape)
    q_count = shape[0]
    ext_w, key_w, acc_w, out_w, w_w = sizes_of(shape, n, batch)
    d_ext, d_acc, d_out, d_c0 = dev.empty(ext_w), dev.empty(acc_w), dev.empty(out_w), dev.empty(q_count * batch * n)
    d_keys, d_ws = [dev.empty(key_w) for _ in gs], [dev.empty(w_w) for _ in gs]

    def load(seed):
        ext, keys, weights, old = _operands(orc, n, moduli, shape, batch, seed)
        as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int64).copy())      # noqa: E731
        d_ext.copy_(as_t(ext))
        d_c0.copy_(as_t(old.reshape(-1)[:q_count * batch * n]))      # any lazy words under Q
        for d_key, d_w, g in zip(d_keys, d_ws, gs):
            d_key.copy_(as_t(keys[g]))
            d_w.copy_(as_t(weights["one-frame"]))
        d_acc.zero_()
        d_out.zero_()

    def call(s):
        for r, (d_key, d_w, g) in enumerate(zip(d_keys, d_ws, gs)):
            ks.accumulate_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_acc.data_ptr(), batch, g, d_w.data_ptr(), 1, r > 0, s)
        ks.mod_down(d_acc.data_ptr(), d_out.data_ptr(), batch, s)
        plan.mul_add_galois(d_ws[0].data_ptr(), d_c0.data_ptr(), d_out.data_ptr(), batch, gs[0], 1, True, 0, q_count, s)

    seeds = (n + 1, n + 2)
    eager = {}
    for seed in seeds:
        load(seed)
        call(dev.stream)
        eager[seed] = dev.to_host(d_out)
    assert not np.array_equal(eager[seeds[0]], eager[seeds[1]])
    load(seeds[0])
    graph = capture(dev, call, call)
    for seed in seeds[::-1]:
        load(seed)
        graph.replay()
        dev.sync()
        assert np.array_equal(dev.to_host(d_out), eager[seed]), ("replay", seed)
    # the eager words are the reference's
    ext, keys, weights, old = _operands(orc, n, moduli, shape, batch, seeds[0])
    rotations = [(g, keys[g], weights["one-frame"]) for g in gs]
    want = linear_transform_ref(orc, n, moduli, shape, ext, rotations, batch)
    active = active_of(moduli, shape)
    want[0] = mul_add_ref(n, active[:q_count], weights["one-frame"][:q_count], old.reshape(-1)[:q_count * batch * n], want[0], batch, gs[0])
    assert np.array_equal(eager[seeds[0]], want.reshape(-1))
    ks.close()
    plan.close()
