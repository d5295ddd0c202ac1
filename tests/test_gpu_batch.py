"""agx_ntt_batch_encode / _decode and agx_ntt_plain_reduce on the device, word for word against the Python-integer model (tests/batch_ref.py): whole frames
at n = 2, 4, 8, 64; sampled frames and slots by the definition z_j = m(psi^{e_j}) and encode o decode = identity over all words at n = 512 ... 32768; the
smallest admitted prime, 65537, a prime on each side of 2^31 and one of 61 bits; batches 1, 3 and one past a grid-stride trip; the scratch apart and the
scratch the operand, with guard bands; the default route and the radix-2 twin through agx_ntt_batch_plan; 8-byte-only placement (the 8-byte stores); graph
capture; the statuses in their order, rejected calls writing nothing; plain_reduce at L = 1, 2, 4, 16, every kind of t, lazy and reduced words, 0 and
+-(D - 1) / 2, every factor; and BFV and BGV from slots to slots on the listings of INTEGRATION.md."""
import functools
import random

import numpy as np
import pytest

import batch_ref as ref
from gpu_util import Layout, arena_for, canary, capture, moduli_for, plan_for_moduli, status_of
from modulus_cases import prime_above, prime_below
from rns_ref import oracle_forward_set

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _moduli_t(orc, n):
    """per n: the smallest admitted prime, 65537 (2n divides 65536 for every size), one prime on each side of 2^31, one of 61 bits"""
    ts = [prime_above(orc, 1, n), 65537, prime_below(orc, 1 << 31, n), prime_above(orc, 1 << 31, n), prime_below(orc, 1 << 61, n)]
    assert all((t - 1) % (2 * n) == 0 and ref.is_prime(t) for t in ts) and ts[4] > 1 << 60
    return list(dict.fromkeys(ts))


def _slots(rng, t, count):
    """slot words: any 64-bit words, the words around t and the ends of the range among them"""
    fixed = [0, 1, t - 1, t, t + 1, 2 * t, 2**64 - 1, 2**63, 2**64 - t]
    z = rng.integers(0, 2**64, size=count, dtype=np.uint64)
    k = min(count, len(fixed))
    z[-k:] = _u64(fixed[:k])
    return z


def _set_variant(agx, batch, variant):
    assert agx.lib().agx_ntt_plan_set_variant(batch.plan(), variant) == 0


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


# ---- batching: whole frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8, 64])
def test_whole_frames_against_the_model(agx, orc, dev, n):
    st = dev.stream
    for t in _moduli_t(orc, n):
        b = agx.Batch(n, t)
        assert b.info()[:3] == (n, t, ref.min_root(t, n)) == (n, t, agx.min_root(t, n))
        for batch in (1, 3):
            rng = np.random.default_rng(n * 1000 + batch)
            count = batch * n
            z = _slots(rng, t, count)
            want_m = _u64([ref.encode(row.tolist(), n, t) for row in z.reshape(batch, n)]).reshape(-1)
            msg = rng.integers(0, t, size=count, dtype=np.uint64)
            msg[:min(count, 3)] = _u64([t - 1, 0, 1][:min(count, 3)])
            model = ref.decode if n <= 8 else ref.decode_fast      # the definition slot by slot; at n = 64 the transform the CPU test judges against it
            want_z = _u64([model(row.tolist(), n, t) for row in msg.reshape(batch, n)]).reshape(-1)
            for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2):
                _set_variant(agx, b, variant)
                lz, lm = Layout(n, 1, batch, offset=0), Layout(n, 1, batch, offset=count)      # they meet end to end
                arena = arena_for(dev, n, (lz, z), (lm, None))
                b.encode(arena.address(0), arena.address(count), batch, st)
                img = arena.image()
                got = arena.frames(lm, img)
                assert np.array_equal(got, want_m), (n, t, batch, variant, "encode", _first_bad(got, want_m))
                assert not arena.faults([(lz, z), (lm, None)], img)
                for in_place in (False, True):
                    lm, lz = Layout(n, 1, batch, offset=0), Layout(n, 1, batch, offset=count)
                    ls = lm if in_place else Layout(n, 1, batch, offset=2 * count)
                    placed = [(lm, msg), (lz, None)] + ([] if in_place else [(ls, None)])
                    arena = arena_for(dev, n, *placed)
                    b.decode(arena.address(0), arena.address(count), arena.address(ls.offset), batch, st)
                    img = arena.image()
                    got = arena.frames(lz, img)
                    assert np.array_equal(got, want_z), (n, t, batch, variant, in_place, "decode", _first_bad(got, want_z))
                    judged = [(lm, None if in_place else msg), (lz, None)] + ([] if in_place else [(ls, None)])
                    assert not arena.faults(judged, img), (n, t, batch, in_place)      # d_m unchanged with a scratch apart; nothing outside the frames
        b.close()


# ---- batching: sampled frames and slots, the identity over all words -------------------------------------------------------------------------
def _judge_sampled(dev, agx, b, n, t, batch, seed, misalign=False, apart=True):
    """encode random slot words inside a guarded arena, judge sampled frames and slots of the polynomial by the definition, decode with the scratch apart
    (apart) and with the scratch the operand, and compare ALL words with the slots modulo t; after every call every word outside the call's outputs -- the
    guard bands, the gaps, the operands -- must be what it was.  misalign: every buffer 8 bytes off a 16-byte boundary.  Without `apart` the arena holds two
    buffers only (the sizes past a grid-stride trip): decode then writes the slots over d_z."""
    st = dev.stream
    count, off = batch * n, 1 if misalign else 0
    rng = np.random.default_rng(seed)
    z = _slots(rng, t, count)
    gap = 2      # canary words between the buffers: an even count keeps every buffer's alignment class
    lz, lm = Layout(n, 1, batch, offset=off), Layout(n, 1, batch, offset=off + count + gap)
    lb, ls = Layout(n, 1, batch, offset=off + 2 * (count + gap)), Layout(n, 1, batch, offset=off + 3 * (count + gap))
    arena = arena_for(dev, n, (lz, z), (lm, None), *(((lb, None), (ls, None)) if apart else ()))
    pz, pm, pb, ps = (arena.address(l.offset) for l in (lz, lm, lb, ls)) if apart else (arena.address(lz.offset), arena.address(lm.offset), None, None)
    assert all((p % 16 == 8) == misalign for p in (pz, pm, pb, ps) if p is not None)
    b.encode(pz, pm, batch, st)
    img = arena.image()
    m = arena.frames(lm, img)
    assert not arena.faults([(lz, z), (lm, None)] + ([(lb, None), (ls, None)] if apart else []), img), (n, t, batch, "encode wrote outside d_m")
    if apart:
        assert np.array_equal(arena.frames(lb, img), canary(arena.band + lb.offset, count)) and np.array_equal(arena.frames(ls, img), canary(arena.band + ls.offset, count))
    assert int(m.max()) < t
    pyr = random.Random(seed)
    for f in sorted({0, batch - 1, pyr.randrange(batch)}):
        row = m[f * n:(f + 1) * n].tolist()
        for j in sorted({0, n // 2 - 1, n // 2, n - 1, pyr.randrange(n), pyr.randrange(n)}):
            assert ref.decode_slot(row, n, t, j) == int(z[f * n + j]) % t, (n, t, batch, f, j)
    want = z % np.uint64(t)
    if apart:
        b.decode(pm, pb, ps, batch, st)
        img = arena.image()
        got = arena.frames(lb, img)
        assert np.array_equal(got, want), (n, t, batch, "scratch apart", _first_bad(got, want))
        assert not arena.faults([(lz, z), (lm, m), (lb, None), (ls, None)], img), (n, t, batch, "decode wrote outside d_z and the scratch, or changed d_m")
        b.decode(pm, pz, pm, batch, st)      # the scratch the operand; the slots go over d_z
        img = arena.image()
        judged = [(lz, None), (lm, None), (lb, want), (ls, None)]
    else:
        b.decode(pm, pz, pm, batch, st)
        img = arena.image()
        judged = [(lz, None), (lm, None)]
    got = arena.frames(lz, img)
    assert np.array_equal(got, want), (n, t, batch, "scratch the operand", _first_bad(got, want))
    assert not arena.faults(judged, img), (n, t, batch, "decode in place wrote outside d_z and d_m")


@pytest.mark.parametrize("n", [512, 1024, 4096, 32768])
def test_sampled_frames_and_the_identity_over_all_words(agx, orc, dev, n):
    for t in _moduli_t(orc, n):
        b = agx.Batch(n, t)
        for variant in (agx.VARIANT_AUTO, agx.VARIANT_LDS_RADIX2):
            _set_variant(agx, b, variant)
            inv = fwd = 1 if variant == agx.VARIANT_AUTO or n <= 16384 else 2
            if variant == agx.VARIANT_LDS_RADIX2:
                assert b.info()[3:] == (1 + inv, fwd + 1), (n, t, b.info())
            else:
                assert b.info()[3] in (2, 3) and b.info()[4] in (2, 3)
            for batch in (1, 3):
                _judge_sampled(dev, agx, b, n, t, batch, n + batch)
        b.close()


@pytest.mark.parametrize("batch,misalign", [(2049, False), (1025, True)], ids=["pairs", "words"])
def test_one_batch_past_a_grid_stride_trip(agx, orc, dev, batch, misalign):
    """a launch covers 16384 x 256 work items a trip: 2048 frames of n = 4096 where a lane stores a pair of words, 1024 where the output is only 8-byte
    aligned and a lane stores one; the last frame is among the judged ones.  Two buffers in one guarded arena: decode runs with the scratch the operand (both
    scratch modes run at every other size)"""
    n, t = 4096, 65537
    b = agx.Batch(n, t)
    _judge_sampled(dev, agx, b, n, t, batch, batch, misalign, apart=False)
    b.close()


def test_an_encode_decode_pair_replays_from_a_graph(agx, orc, dev):
    torch = dev.torch
    n, t, batch = 1024, prime_below(orc, 1 << 61, 1024), 3
    b = agx.Batch(n, t)
    count = batch * n
    rng = np.random.default_rng(5)
    zs = [_slots(rng, t, count) for _ in range(2)]
    d_z, d_m, d_back, d_scr = dev.to_device(zs[0]), dev.empty(count), dev.empty(count), dev.empty(count)

    def pair(s):
        b.encode(d_z.data_ptr(), d_m.data_ptr(), batch, s)
        b.decode(d_m.data_ptr(), d_back.data_ptr(), d_scr.data_ptr(), batch, s)

    graph = capture(dev, pair, pair)
    for z in zs[::-1]:
        d_z.copy_(torch.from_numpy(z.view(np.int64).copy()))
        d_m.zero_(), d_back.zero_()
        graph.replay()
        dev.sync()
        assert np.array_equal(dev.to_host(d_back), z % np.uint64(t))
        m = dev.to_host(d_m)
        for j in (0, 1, n // 2, n - 1):
            assert ref.decode_slot(m[:n].tolist(), n, t, j) == int(z[j]) % t
    b.close()


def test_status_rules_in_order_and_rejected_calls_write_nothing(agx, orc, dev):
    n, batch, t = 64, 2, 257
    b = agx.Batch(n, t)
    count, w, st = batch * n, 8, dev.stream
    rng = np.random.default_rng(3)
    z, msg = _slots(rng, t, count), rng.integers(0, t, size=count, dtype=np.uint64)
    lz, lm, ls = Layout(n, 1, batch, offset=0), Layout(n, 1, batch, offset=count), Layout(n, 1, batch, offset=2 * count)
    arena = arena_for(dev, n, (lz, z), (lm, msg), (ls, None))
    before = arena.image()
    pz, pm, ps = (arena.address(l.offset) for l in (lz, lm, ls))
    E, D = b.encode, b.decode
    assert [status_of(agx, E, *a, batch, st) for a in ((0, pm), (pz, 0), (0, 0))] == [1, 1, 1]                                   # NULL
    assert status_of(agx, E, 0, pm + 4, 1 << 63, st) == 1                                                                       # ... before every other rule
    assert [status_of(agx, E, *a, batch, st) for a in ((pz + 4, pm), (pz, pm + 4))] == [5, 5]                                   # uint64_t data
    assert status_of(agx, E, pz, pm, (1 << 64) - 1, st) == 5 and status_of(agx, E, pz, pm, 1 << 40, st) == 5                    # the grid limit
    for out in (pz, pz + w, pz + w * (count - 1), pz - w * (count - 1)):                                                        # d_m touches d_z
        assert status_of(agx, E, pz, out, batch, st) == 5, out - pz
    E(pz, pm, 0, st)                                                                                                            # an empty batch
    assert [status_of(agx, D, *a, batch, st) for a in ((0, pz, ps), (pm, 0, ps), (pm, pz, 0))] == [1, 1, 1]                      # NULL
    assert [status_of(agx, D, *a, batch, st) for a in ((pm + 4, pz, ps), (pm, pz + 4, ps), (pm, pz, ps + 4))] == [5, 5, 5]       # uint64_t data
    assert status_of(agx, D, pm, pz, ps, (1 << 64) - 1, st) == 5 and status_of(agx, D, pm, pz, ps, 1 << 40, st) == 5            # the grid limit
    for scratch in (pm + w, pm + w * (n // 2), pm + w * (count - 1), pm - w * (count - 1)):                                     # a scratch that straddles d_m
        assert status_of(agx, D, pm, pz, scratch, batch, st) == 5
    for out in (pm, pm + w * (n // 2), pm + w * (count - 1), ps, ps + w * (count - 1), pm - w * (count - 1)):                   # d_z touches d_m or the scratch
        assert status_of(agx, D, pm, out, ps, batch, st) == 5
    assert status_of(agx, D, pm, pm + w, pm, batch, st) == 5                                                                    # ... also where the scratch is d_m
    D(pm, pz, ps, 0, st), D(pm, pz, pm, 0, st)                                                                                  # an empty batch
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # allowed: ranges that meet end to end
    D(pm, pz, ps, batch, st)
    img = arena.image()
    assert np.array_equal(arena.frames(lz, img), _u64([ref.decode(r.tolist(), n, t) for r in msg.reshape(batch, n)]).reshape(-1))
    assert not arena.faults([(lz, None), (lm, msg), (ls, None)], img)
    # creation: the rules behind the NULL rule that need a device-side view of nothing are tests/test_abi_batch.py's; here, what a real handle reports
    assert b.info()[:3] == (n, t, agx.min_root(t, n)) and b.plan()
    b.close()
    b.close()


# ---- agx_ntt_plain_reduce ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reduce_case(orc, n, Q, batch):
    """coefficients X (Python integers) with 0, +-1 and +-(D - 1) / 2 among them, their NTT-form residues reduced and spread over the lazy range"""
    rng, nprng = random.Random(n * 31 + len(Q)), np.random.default_rng(len(Q))
    D = ref.product(Q)
    H = (D - 1) // 2
    count = batch * n
    X = [rng.randrange(-H, H + 1) for _ in range(count)]
    edges = [0, 1, -1, H, -H, H - 1, 1 - H]
    for f in range(batch):      # every frame carries the edges, at places of their own
        for k, v in enumerate(edges):
            X[f * n + (7 * k + f) % n] = v
    rows = _u64([[v % q for v in X] for q in Q])
    x = oracle_forward_set(orc, n, Q, rows)
    lazy = x + _u64([[int(k) * q for k in nprng.integers(0, 4, size=count)] for q in Q])
    for a in (x, lazy):
        a.setflags(write=False)
    return tuple(X), x.reshape(-1), lazy.reshape(-1)


@pytest.mark.parametrize("L", [1, 2, 4, 16])
@pytest.mark.parametrize("n", [64, 4096])
def test_plain_reduce_against_the_model(agx, orc, dev, n, L):
    batch = 3 if n == 64 else 1
    moduli = moduli_for(orc.find_prime, n, [60, 50, 55, 60] + [58] * 4 + [45] * 8 + [52])[:L] + (orc.find_prime(59, n, 0),)      # Q, then gamma
    Q = tuple(moduli[:L])
    plan = plan_for_moduli(agx, orc, n, moduli)[0]
    X, x, lazy = _reduce_case(orc, n, Q, batch)
    count, st = batch * n, dev.stream
    for t in (2, 1 << 16, 257, 65537, prime_below(orc, 1 << 61, n)):
        plain = plan.plain(0, L, L, t)
        for factor in (1, 0, t - 1, (1 << 64) - 1):
            want = _u64([factor % t * v % t for v in X])
            for name, words in (("reduced", x), ("lazy", lazy)):
                for in_place in (False, True):
                    d_x, d_got = dev.to_device(words), dev.to_device(canary(0, count))
                    d_scratch = d_x if in_place else dev.to_device(canary(7, L * count))
                    plain.reduce(d_x.data_ptr(), d_got.data_ptr(), d_scratch.data_ptr(), batch, factor, st)
                    got = dev.to_host(d_got)
                    assert np.array_equal(got, want), (n, L, t, factor, name, in_place, _first_bad(got, want))
                    assert in_place or np.array_equal(dev.to_host(d_x), words), "d_x changed"
        plain.close()
    if n == 64 and L == 4:      # the model itself, from the residues alone, gives the same words
        rows = [[v % q for v in X] for q in Q]
        assert ref.reduce(rows, Q, 65537, 3) == [3 * v % 65537 for v in X] == ref.reduce_device_form(rows, Q, 65537, 3)
    plan.close()


def test_plain_reduce_status_rules_and_guard_bands(agx, orc, dev):
    n, batch, L, t = 64, 2, 3, 65537
    moduli = moduli_for(orc.find_prime, n, [45, 52, 60, 57])
    plan, forward_only = plan_for_moduli(agx, orc, n, moduli)[0], plan_for_moduli(agx, orc, n, moduli, inverse=False)[0]
    plain, lame = plan.plain(0, L, L, t), forward_only.plain(0, L, L, t)
    X, x, _ = _reduce_case(orc, n, tuple(moduli[:L]), batch)
    slab, w, st = batch * n, 8, dev.stream
    lx, ls, lm = Layout(n, L, batch, offset=0), Layout(n, L, batch, offset=L * slab), Layout(n, 1, batch, offset=2 * L * slab)
    arena = arena_for(dev, n, (lx, x), (ls, None), (lm, None))
    before = arena.image()
    px, ps, pm = (arena.address(l.offset) for l in (lx, ls, lm))
    R = lambda *a: status_of(agx, plain.reduce, *a)      # noqa: E731   (d_x, d_m, d_scratch, batch, factor, stream)
    assert [R(*a, batch, 1, st) for a in ((0, pm, ps), (px, 0, ps), (px, pm, 0))] == [1, 1, 1]                       # NULL
    assert [R(*a, batch, 1, st) for a in ((px + 4, pm, ps), (px, pm + 4, ps), (px, pm, ps + 4))] == [5, 5, 5]         # uint64_t data
    assert R(px, pm, ps, (1 << 64) - 1, 1, st) == 5 and R(px, pm, ps, 1 << 40, 1, st) == 5                           # the grid limit
    for scratch in (px + w, px + w * (L * slab - 1), px - w * (L * slab - 1)):                                       # a scratch that straddles d_x
        assert R(px, pm, scratch, batch, 1, st) == 5
    for out in (px, px + w * (L * slab - 1), ps, ps + w * (L * slab - 1), px - w * (slab - 1)):                      # d_m touches d_x or the scratch
        assert R(px, out, ps, batch, 1, st) == 5
    assert R(px, px + w * slab, px, batch, 1, st) == 5                                                               # ... also where the scratch is d_x
    assert status_of(agx, lame.reduce, px + 4, pm, ps, batch, 1, st) == 5                                            # no inverse tables: behind the argument rules,
    assert status_of(agx, lame.reduce, px, pm, ps, batch, 1, st) == 9 and status_of(agx, lame.reduce, px, pm, ps, 0, 1, st) == 9      # in front of the empty batch
    plain.reduce(px, pm, ps, 0, 1, st)
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    plain.reduce(px, pm, ps, batch, t - 1, st)      # ranges that meet end to end
    img = arena.image()
    assert np.array_equal(arena.frames(lm, img), _u64([(t - 1) * v % t for v in X])) and np.array_equal(arena.frames(lx, img), x)
    assert not arena.faults([(lx, x), (ls, None), (lm, None)], img)
    for h in (plain, lame, plan, forward_only):
        h.close()


# ---- end to end: BFV and BGV from slots to slots ("BFV with batching" and "BGV") --------------------------------------------
class _Scheme:
    """the plan of both listings at n = 64: Q = three ~50-bit primes, the special prime P behind them, one more prime as the gamma of the level-4 handle;
    every ciphertext component is a buffer of ALL five slabs (agx_ntt_automorphism works on the whole plan), of which the ranged calls use a prefix"""

    def __init__(self, agx, orc, dev, t):
        self.agx, self.dev, self.t, self.n, self.batch = agx, dev, t, 64, 2
        n = self.n
        self.moduli = moduli_for(orc.find_prime, n, [50, 50, 50, 52, 55])
        self.plan = agx.Plan(n, list(self.moduli))
        self.W = 5
        self.slab = self.batch * n
        self.bt = agx.Batch(n, t)
        self.seed = bytes(range(32))
        self.st = dev.stream
        self.s_hat = dev.empty(self.W * n)      # [5][1][n]
        self.plan.sample_ternary(self.seed, 0, self.s_hat.data_ptr(), 1, 0, 0, None, NTT, self.st)
        self.draw = 1

    def component(self):
        d = self.dev.empty(self.W * self.slab)
        d.zero_()
        return d

    def encode(self, z):
        d_z, d_m = self.dev.to_device(_u64(z).reshape(-1)), self.dev.empty(self.slab)
        self.bt.encode(d_z.data_ptr(), d_m.data_ptr(), self.batch, self.st)
        return d_m

    def decode(self, d_m):
        d_z = self.dev.empty(self.slab)
        self.bt.decode(d_m.data_ptr(), d_z.data_ptr(), d_m.data_ptr(), self.batch, self.st)
        return self.dev.to_host(d_z).reshape(self.batch, self.n).tolist()

    def mask(self, c0, L, noise):
        """(c0, c1) <- (c0 - a s + noise, a) on the primes [0, L): a uniform, a s through one key frame per prime"""
        p, st, b = self.plan, self.st, self.batch
        c1, tmp = self.component(), self.component()
        p.sample_uniform(self.seed, self.draw, c1.data_ptr(), b, 0, 0, L, st)
        p.mul_add_galois(self.s_hat.data_ptr(), c1.data_ptr(), tmp.data_ptr(), b, 1, 1, False, 0, L, st)
        p.sub(c0.data_ptr(), tmp.data_ptr(), c0.data_ptr(), b, 0, L, st)
        p.add(c0.data_ptr(), noise.data_ptr(), c0.data_ptr(), b, 0, L, st)
        self.draw += 1
        return [c0, c1]

    def phase(self, ct, L, key=None):
        """c0 + c1 s (+ c2 s^2) on the primes [0, L), NTT form, [L][batch][n]: one accumulating product per component behind the first"""
        p, st, b = self.plan, self.st, self.batch
        key = self.s_hat if key is None else key
        out, power = self.component(), key
        p.add(ct[0].data_ptr(), out.data_ptr(), out.data_ptr(), b, 0, L, st)      # out = c0 (out is zero)
        for k, c in enumerate(ct[1:]):
            if k:
                nxt = self.dev.empty(self.W * self.n)
                p.mul_add_galois(key.data_ptr(), power.data_ptr(), nxt.data_ptr(), 1, 1, None, False, 0, L, st)      # s^(k+1)
                power = nxt
            p.mul_add_galois(power.data_ptr(), c.data_ptr(), out.data_ptr(), b, 1, 1, True, 0, L, st)
        return out

    def close(self):
        self.bt.close()
        self.plan.close()


@pytest.mark.parametrize("t", [257, 65537])
def test_bfv_from_slots_to_slots(agx, orc, dev, t):
    S = _Scheme(agx, orc, dev, t)
    p, st, b, n, L = S.plan, S.st, S.batch, S.n, 3
    plain = p.plain(0, L, L, t)      # Q = [0, 3), gamma = the special prime
    rng = random.Random(t)
    z = [[[rng.randrange(t) for _ in range(n)] for _ in range(b)] for _ in range(3)]

    def encrypt(slots):
        c0, e = S.component(), S.component()
        plain.scale_up(S.encode(slots).data_ptr(), c0.data_ptr(), b, NTT, st)                 # Delta m
        p.sample_cbd(S.seed, S.draw, 21, e.data_ptr(), b, 0, 0, L, NTT, st)
        return S.mask(c0, L, e)

    def decrypt(ct):
        ph, d_m = S.phase(ct, L), dev.empty(S.slab)
        plain.scale_down(ph.data_ptr(), d_m.data_ptr(), ph.data_ptr(), b, st)
        return S.decode(d_m)

    ct1, ct2 = encrypt(z[0]), encrypt(z[1])
    assert decrypt(ct1) == z[0] and decrypt(ct2) == z[1], "fresh ciphertexts"
    total = [S.component(), S.component()]
    for c in range(2):
        p.add(ct1[c].data_ptr(), ct2[c].data_ptr(), total[c].data_ptr(), b, 0, L, st)
    assert decrypt(total) == [[(u + v) % t for u, v in zip(z[0][f], z[1][f])] for f in range(b)], "the slot-wise sum"
    lifted, prod = S.component(), [S.component(), S.component()]
    plain.lift(S.encode(z[2]).data_ptr(), lifted.data_ptr(), b, NTT, st)                      # multiply-plain: the centred, unscaled plaintext
    for c in range(2):
        p.mul_add_galois(lifted.data_ptr(), ct1[c].data_ptr(), prod[c].data_ptr(), b, 1, None, False, 0, L, st)
    assert decrypt(prod) == [[u * v % t for u, v in zip(z[0][f], z[2][f])] for f in range(b)], "the slot-wise product with a plaintext"
    plain.close()
    S.close()


@pytest.mark.parametrize("t", [257, 65537])
def test_bgv_from_slots_to_slots(agx, orc, dev, t):
    S = _Scheme(agx, orc, dev, t)
    p, st, b, n, W = S.plan, S.st, S.batch, S.n, S.W
    top, low = p.plain(0, 4, 4, t), p.plain(0, 3, 3, t)      # level 4 = Q and the special prime (gamma: the fifth prime); level 3 = Q (gamma: the special prime)
    rng = random.Random(t + 1)
    z = [[[rng.randrange(t) for _ in range(n)] for _ in range(b)] for _ in range(2)]
    t_frame = dev.to_device(_u64([[t % q] * n for q in S.moduli]).reshape(-1))      # the constant t, one frame per prime: NTT form of a constant is itself

    def encrypt(slots):
        c0, e, te = S.component(), S.component(), S.component()
        top.lift(S.encode(slots).data_ptr(), c0.data_ptr(), b, NTT, st)                       # the centred message, unscaled
        p.sample_cbd(S.seed, S.draw, 21, e.data_ptr(), b, 0, 0, 4, NTT, st)
        p.mul_add_galois(t_frame.data_ptr(), e.data_ptr(), te.data_ptr(), b, 1, 1, False, 0, 4, st)      # t e
        return S.mask(c0, 4, te)

    def decrypt(ct, handle, L, factor=1, key=None):
        ph, d_m = S.phase(ct, L, key), dev.empty(S.slab)
        handle.reduce(ph.data_ptr(), d_m.data_ptr(), ph.data_ptr(), b, factor, st)
        return S.decode(d_m)

    ct1, ct2 = encrypt(z[0]), encrypt(z[1])
    assert decrypt(ct1, top, 4) == z[0] and decrypt(ct2, top, 4) == z[1], "fresh ciphertexts"
    # the tensor product, decrypted under (1, s, s^2): agx_ntt_tensor takes [2][count][batch][n] operands, so the level's slabs are gathered first
    slab4 = 4 * S.slab
    ops = [dev.empty(2 * slab4) for _ in range(2)]
    for o, ct in zip(ops, (ct1, ct2)):
        for c in range(2):
            o[c * slab4:(c + 1) * slab4].copy_(ct[c][:slab4])
    d_t3 = dev.empty(3 * slab4)
    p.tensor(ops[0].data_ptr(), ops[1].data_ptr(), d_t3.data_ptr(), b, 0, 4, st)
    ct3 = [S.component() for _ in range(3)]
    for k in range(3):
        ct3[k][:slab4].copy_(d_t3[k * slab4:(k + 1) * slab4])
    product = [[u * v % t for u, v in zip(z[0][f], z[1][f])] for f in range(b)]
    assert decrypt(ct3, top, 4) == product, "the tensor product under (1, s, s^2)"
    # ModDown by the special prime with the plaintext modulus t: the plaintext now carries P^-1 mod t, which factor = P mod t undoes
    down = p.basis(3, 1, 0, 3, t)
    ct3_low = [S.component() for _ in range(3)]
    for k in range(3):
        down.mod_down(ct3[k].data_ptr(), ct3[k].data_ptr() + 8 * 3 * S.slab, ct3_low[k].data_ptr(), ct3[k].data_ptr() + 8 * 3 * S.slab, b, st)
    assert decrypt(ct3_low, low, 3, S.moduli[3] % t) == product, "after ModDown, undone by factor"
    if t > 257:      # without the factor the slots are the product times P^-1 mod t: something else (P mod 257 may be 1; at 65537 it is not)
        assert S.moduli[3] % t != 1 and decrypt(ct3_low, low, 3) != product
    # a row rotation and the row swap through agx_ntt_automorphism on the ModDown'ed ciphertext, decrypted at the level of Q under (1, sigma_g(s), sigma_g(s)^2)
    for g, turn in ((agx.galois_element(n, 3), lambda row: ref.rotate_rows(row, 3)), (2 * n - 1, ref.swap_rows)):
        moved = [S.component() for _ in range(3)]
        for c in range(3):
            p.automorphism(ct3_low[c].data_ptr(), moved[c].data_ptr(), b, g, NTT, st)
        key = dev.empty(W * n)
        p.automorphism(S.s_hat.data_ptr(), key.data_ptr(), 1, g, NTT, st)
        assert decrypt(moved, low, 3, S.moduli[3] % t, key) == [turn(row) for row in product], ("sigma_g", g)
    for h in (down, top, low):
        h.close()
    S.close()
