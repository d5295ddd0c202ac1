"""Where the words live: every kernel family under odd alignment, odd strides and guard bands (run with -m gpu on an MI355X).

The arithmetic of the kernels is covered by test_gpu_parity.py on fresh, 256-byte aligned, densely packed buffers.  Here the same
kernels, under default selection (plus the radix-2 LDS variant), run on frames that sit at odd element offsets and odd strides inside
guarded arenas (gpu_util.GuardedArena): every result is compared bit for bit with the CPU oracle, and every word of every arena that
belongs to no output frame -- the bands in front of and behind the frames, the gaps between them, the whole input of an out-of-place
call -- must come back as it went in.  tests/test_layout_helpers.py shows on the CPU that these checks can fail."""
import numpy as np
import pytest

from gpu_util import GuardedArena, Layout, arena_for, capture, oracle_polymul, plan_from_oracle_tables, rand_coeffs

pytestmark = pytest.mark.gpu

RB_SIZES = [1024, 2048, 4096, 8192, 16384, 32768]


def _batches(n):
    return (67, 259) if n <= 512 else ((5,) if n <= 4096 else (3,))


# (family, n, modulus bits, batch): two primes for n <= 8192, one above
CASES = ([("wp64", n, bits, b) for n in (2, 16, 32, 256, 512) for bits in (60, 62) for b in _batches(n)]
         + [("wp32", n, bits, b) for n in (32, 512) for bits in (30, 31) for b in _batches(n)]
         + [("rb64", n, bits, b) for n in RB_SIZES for bits in (60, 61, 62) for b in _batches(n)]
         + [("rb32", n, bits, b) for n in RB_SIZES for bits in (30, 31) for b in _batches(n)]
         + [("radix2", n, 60, b) for n in (8, 1024, 32768) for b in _batches(n)])
IDS = [f"{f}-n{n}-q{bits}-b{b}" for f, n, bits, b in CASES]


class _Case:
    """plan from the oracle's tables, and the oracle's answers for [prime][batch][n] operands of this plan"""

    def __init__(self, agx, orc, family, n, bits, batch, primes=None):
        self.orc, self.n, self.bits, self.batch = orc, n, bits, batch
        self.primes = (2 if n <= 8192 else 1) if primes is None else primes
        self.plan, self.tabs = plan_from_oracle_tables(agx, orc, n, bits, self.primes)
        if family == "radix2":
            self.plan.set_variant(agx.VARIANT_LDS_RADIX2)
        self.radix2 = family == "radix2"
        self.hi = 4 if bits < 62 else 3          # inputs anywhere in [0,4q); [0,3q) at 62 bits
        self.itw = [orc.make_inv_tables(t[0], t[1], n)[0] for t in self.tabs]
        self.rng = np.random.default_rng(n * 1009 + bits * 17 + batch)

    def rand(self, batch=None, hi=None):
        count = (self.batch if batch is None else batch) * self.n
        return np.concatenate([rand_coeffs(self.rng, count, t[0], hi_mult=self.hi if hi is None else hi) for t in self.tabs])

    def per_prime(self, x):
        return x.reshape(self.primes, -1)

    def reduce(self, x):
        return np.concatenate([xp % np.uint64(t[0]) for xp, t in zip(self.per_prime(x), self.tabs)])

    def forward(self, x, threads=1):
        if threads > 1:
            return np.concatenate([self.orc.forward_mt(xp.copy(), t[0], t[2], t[3], self.n, threads) for xp, t in zip(self.per_prime(x), self.tabs)])
        return np.concatenate([self.orc.forward(xp, t[0], t[2], t[3], self.n) for xp, t in zip(self.per_prime(x), self.tabs)])

    def inverse(self, y):
        return np.concatenate([self.orc.inverse(yp % np.uint64(t[0]), t[0], itw, self.n) for yp, t, itw in zip(self.per_prime(y), self.tabs, self.itw)])

    def pointwise(self, a, b):
        return np.concatenate([self.orc.pointwise(ap % np.uint64(t[0]), bp % np.uint64(t[0]), t[0])
                               for ap, bp, t in zip(self.per_prime(a), self.per_prime(b), self.tabs)])

    def product(self, a, b, b_batch=None):
        """a * b in Z_q[X]/(X^n + 1) frame by frame through the oracle's transforms (b_batch = 1: every frame of a prime meets b's one
        frame of that prime); the first and the last frame are cross-checked against the schoolbook product for n <= 1024"""
        n, B = self.n, self.batch
        bb = B if b_batch is None else b_batch
        out = np.empty_like(a)
        for p, t in enumerate(self.tabs):
            for f in range(B):
                sa = slice((p * B + f) * n, (p * B + f + 1) * n)
                fb = f if bb == B else 0
                sb = slice((p * bb + fb) * n, (p * bb + fb + 1) * n)
                out[sa] = oracle_polymul(self.orc, a[sa], b[sb], t[0], t[1], n)
                if n <= 1024 and f in (0, B - 1):
                    q = np.uint64(t[0])
                    assert np.array_equal(out[sa], self.orc.schoolbook(a[sa] % q, b[sb] % q, t[0], n))
        return out

    def close(self):
        self.plan.close()


def _describe(faults):
    return "; ".join(f"word {f['index']} (prime {f['prime']} frame {f['frame']} + {f['rel']}): got {f['got']:#x}, want {f['want']:#x}" for f in faults)


class _Report:
    """collects what went wrong over the many launches of one test, so that one failing layout does not hide the next"""

    def __init__(self):
        self.lines = []

    def check(self, what, arena, placed):
        faults = arena.faults(placed)
        if faults:
            self.lines.append(f"{what}: {_describe(faults)}")
        return not faults

    def require(self, what, ok):
        if not ok:
            self.lines.append(what)

    def done(self):
        assert not self.lines, "\n".join(self.lines)


def _layouts(n, primes, batch):
    """(name, input layout, output layout, one arena for both) of the out-of-place call; the in-place calls use the input layout"""
    dense = Layout(n, primes, batch)
    prime_major = Layout(n, primes, batch, prime_stride=batch * (n + 1) + 3, poly_stride=n + 1)      # every other frame misaligned under an aligned base
    poly_major = Layout(n, primes, batch, prime_stride=n + 1, poly_stride=primes * (n + 1) + 4)
    interleaved = Layout(n, primes, batch, prime_stride=2 * batch * n, poly_stride=2 * n)             # out = in + n: documented as legal
    return [("dense, input at element 1", dense.at(1), dense, False),
            ("dense, output at element 1", dense, dense.at(1), False),
            ("dense, both at element 1", dense.at(1), dense.at(1), False),
            ("prime-major padded", prime_major, prime_major, False),
            ("poly-major padded", poly_major, poly_major, False),
            ("interleaved in one arena", interleaved, interleaved.at(n), True)]


def _strided_calls(case, dev, rep, name, lin, lout, shared, x, want_f, want_i):
    """forward_strided out of place and in place, inverse_strided in place on one layout, every arena judged word for word"""
    n, B, plan, stream = case.n, case.batch, case.plan, dev.stream
    ps, ls = lin.prime_stride, lin.poly_stride
    if shared:
        src = dst = arena_for(dev, n, (lin, x), (lout, None))
    else:
        src, dst = arena_for(dev, n, (lin, x)), arena_for(dev, n, (lout, None))
    plan.forward_strided(src.address(lin.offset), dst.address(lout.offset), B, ps, ls, stream)
    if shared:
        rep.check(f"{name}: forward out of place", src, [(lin, x), (lout, want_f)])
    else:
        rep.check(f"{name}: forward out of place, output arena", dst, [(lout, want_f)])
        rep.check(f"{name}: forward out of place, input arena", src, [(lin, x)])
    arena = arena_for(dev, n, (lin, x))
    plan.forward_strided(arena.address(lin.offset), arena.address(lin.offset), B, ps, ls, stream)
    rep.check(f"{name}: forward in place", arena, [(lin, want_f)])
    arena = arena_for(dev, n, (lin, x))
    plan.inverse_strided(arena.address(lin.offset), arena.address(lin.offset), B, ps, ls, stream)
    rep.check(f"{name}: inverse in place", arena, [(lin, want_i)])


@pytest.mark.parametrize("family,n,bits,batch", CASES, ids=IDS)
def test_strided_layouts_in_guarded_arenas(agx, orc, dev, family, n, bits, batch):
    """odd bases, padded prime-major and poly-major layouts with odd strides, and the interleaved out-of-place layout, through
    forward_strided (out of place, in place) and inverse_strided (in place)"""
    case = _Case(agx, orc, family, n, bits, batch)
    x = case.rand()
    want_f, want_i = case.forward(x), case.inverse(x)
    rep = _Report()
    for name, lin, lout, shared in _layouts(n, case.primes, batch):
        _strided_calls(case, dev, rep, name, lin, lout, shared, x, want_f, want_i)
    case.close()
    rep.done()


@pytest.mark.parametrize("family,n,bits,batch", CASES, ids=IDS)
def test_dense_transforms_at_odd_bases(agx, orc, dev, family, n, bits, batch):
    """forward, forward_lazy, inverse and fill_synthetic with every base pointer at element offset 1 of its arena"""
    case = _Case(agx, orc, family, n, bits, batch)
    plan, odd = case.plan, Layout(n, case.primes, batch).at(1)
    x = case.rand()
    want_f = case.forward(x)
    rep = _Report()
    for call in ("forward", "inverse"):
        want = want_f if call == "forward" else case.inverse(x)
        src, dst = arena_for(dev, n, (odd, x)), arena_for(dev, n, (odd, None))
        getattr(plan, call)(src.address(1), dst.address(1), batch, dev.stream)
        rep.check(f"{call} out of place, output arena", dst, [(odd, want)])
        rep.check(f"{call} out of place, input arena", src, [(odd, x)])
        getattr(plan, call)(src.address(1), src.address(1), batch, dev.stream)
        rep.check(f"{call} in place", src, [(odd, want)])
    # lazy outputs: below 4q and congruent to the transform
    src, dst = arena_for(dev, n, (odd, x)), arena_for(dev, n, (odd, None))
    plan.forward_lazy(src.address(1), dst.address(1), batch, dev.stream)
    image = dst.image()
    rep.check("forward_lazy, words outside the output frames", dst, [(odd, None)])
    rep.check("forward_lazy, input arena", src, [(odd, x)])
    y = dst.frames(odd, image)
    for yp, t in zip(case.per_prime(y), case.tabs):
        rep.require(f"forward_lazy: a value of modulus {t[0]} is not below 4q", bool((yp.astype(object) < 4 * t[0]).all()))
    rep.require("forward_lazy: not congruent to the transform", np.array_equal(case.reduce(y), want_f))
    # synthetic coefficients: the same words as on an aligned buffer
    even = odd.at(0)
    aligned, shifted = arena_for(dev, n, (even, None)), arena_for(dev, n, (odd, None))
    plan.fill_synthetic(aligned.address(0), batch, 5, 99, dev.stream)
    plan.fill_synthetic(shifted.address(1), batch, 5, 99, dev.stream)
    filled = aligned.frames(even)
    for fp, t in zip(case.per_prime(filled), case.tabs):
        rep.require("fill_synthetic: a value is not reduced", bool((fp < np.uint64(t[0])).all()))
    rep.check("fill_synthetic on an aligned base", aligned, [(even, filled)])
    rep.check("fill_synthetic at element 1", shifted, [(odd, filled)])
    case.close()
    rep.done()


@pytest.mark.parametrize("family,n,bits,batch", CASES, ids=IDS)
def test_pointwise_and_polymul_at_odd_bases(agx, orc, dev, family, n, bits, batch):
    """agx_ntt_pointwise (c distinct, c = a, c = b) and agx_ntt_polymul (c distinct, c = a, c = b, a = b = c) with every operand at
    element offset 1; pointwise operands in [0,4q), reduced under 62-bit moduli"""
    case = _Case(agx, orc, family, n, bits, batch)
    plan, odd = case.plan, Layout(n, case.primes, batch).at(1)
    rep = _Report()

    def run(call, a, b, alias, want):
        """alias: which operands c is ('', 'a', 'b', 'ab'); operands that are not c must come back unchanged"""
        A = arena_for(dev, n, (odd, a))
        Bm = A if alias == "ab" else arena_for(dev, n, (odd, b))
        C = {"": None, "a": A, "b": Bm, "ab": A}[alias] or arena_for(dev, n, (odd, None))
        if call == "pointwise":
            plan.pointwise(A.address(1), Bm.address(1), C.address(1), batch, dev.stream)
        else:
            S = arena_for(dev, n, (odd, None)) if case.radix2 else None      # only the three-launch path of the radix-2 kernels needs scratch
            plan.polymul(A.address(1), Bm.address(1), C.address(1), S.address(1) if S else 0, batch, dev.stream)
            if S:
                rep.check(f"{call}, c = {alias or 'distinct'}: scratch arena", S, [(odd, None)])
        what = f"{call}, c = {alias or 'distinct'}"
        rep.check(f"{what}: result arena", C, [(odd, want)])
        if A is not C:
            rep.check(f"{what}: arena of a", A, [(odd, a)])
        if Bm is not C:
            rep.check(f"{what}: arena of b", Bm, [(odd, b)])

    a, b = case.rand(hi=1 if bits == 62 else 4), case.rand(hi=1 if bits == 62 else 4)
    want = case.pointwise(a, b)
    for alias in ("", "a", "b"):
        run("pointwise", a, b, alias, want)
    a, b = case.rand(), case.rand()
    want = case.product(a, b)
    for alias in ("", "a", "b"):
        run("polymul", a, b, alias, want)
    run("polymul", a, a, "ab", case.product(a, a))
    case.close()
    rep.done()


@pytest.mark.parametrize("family,n,bits,batch", CASES, ids=IDS)
def test_polymul_ntt_at_odd_bases(agx, orc, dev, family, n, bits, batch):
    """agx_ntt_polymul_ntt with a, c and bhat each at an even or an odd element offset, independently; bhat written by forward and by
    forward_lazy, one frame per frame and one frame per prime; c = a at odd offsets too"""
    case = _Case(agx, orc, family, n, bits, batch)
    plan, primes = case.plan, case.primes
    dense = Layout(n, primes, batch)
    rep = _Report()
    a = case.rand()
    for bb in (batch, 1):
        b = case.rand(batch=bb)
        want = case.product(a, b, b_batch=bb)
        lb = Layout(n, primes, bb)
        for fwd in ("forward", "forward_lazy"):
            src, dst = arena_for(dev, n, (lb, b)), arena_for(dev, n, (lb, None))
            getattr(plan, fwd)(src.address(0), dst.address(0), bb, dev.stream)
            bhat = dst.frames(lb)
            for oa, oc, ob in [(oa, oc, ob) for oa in (0, 1) for oc in (0, 1) for ob in (0, 1)] + [(1, "a", 0), (1, "a", 1), (0, "a", 1)]:
                what = f"bhat by {fwd}, bhat_batch {bb}, a at {oa}, c at {oc}, bhat at {ob}"
                A, H = arena_for(dev, n, (dense.at(oa), a)), arena_for(dev, n, (lb.at(ob), bhat))
                if oc == "a":
                    C, lc = A, dense.at(oa)
                else:
                    lc = dense.at(oc)
                    C = arena_for(dev, n, (lc, None))
                plan.polymul_ntt(A.address(oa), H.address(ob), C.address(lc.offset), batch, bb, dev.stream)
                rep.check(f"{what}: result arena", C, [(lc, want)])
                if C is not A:
                    rep.check(f"{what}: arena of a", A, [(dense.at(oa), a)])
                rep.check(f"{what}: arena of bhat", H, [(lb.at(ob), bhat)])
    case.close()
    rep.done()


def test_forward_companion_under_a_stride(agx, orc, dev):
    """n = 4096, 60-bit modulus, one prime, 4,099 frames: from 4,096 frames per launch the forward runs on its streamed companion
    kernel, which computes its own frame addresses; poly-major padded layout (odd prime stride, frames at every alignment)"""
    n, batch = 4096, 4099
    case = _Case(agx, orc, "rb64", n, 60, batch, primes=1)
    lay = Layout(n, 1, batch, prime_stride=n + 1, poly_stride=(n + 1) + 4)
    x = case.rand()
    want = case.forward(x, threads=8)
    rep = _Report()
    src, dst = arena_for(dev, n, (lay, x)), arena_for(dev, n, (lay, None))
    case.plan.forward_strided(src.address(0), dst.address(0), batch, lay.prime_stride, lay.poly_stride, dev.stream)
    rep.check("forward out of place, output arena", dst, [(lay, want)])
    rep.check("forward out of place, input arena", src, [(lay, x)])
    del dst
    case.plan.forward_strided(src.address(0), src.address(0), batch, lay.prime_stride, lay.poly_stride, dev.stream)
    rep.check("forward in place", src, [(lay, want)])
    case.close()
    rep.done()


def test_counter_driven_inverse_under_a_stride(agx, orc, dev):
    """n = 16384, 60-bit moduli, 301 frames under each of two primes: 602 frames, more than the two workgroups per CU that stay
    resident, so the inverse's workgroups draw further frames from the counter and compute the addresses of those themselves;
    poly-major padded layout, forward and inverse, and the inverse once more inside a captured graph, where it takes the
    stateless form and walks the frames with a fixed stride"""
    import torch

    n, batch, primes = 16384, 301, 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert primes * batch > 2 * cus, f"{primes * batch} frames do not exceed the resident grid of {cus} CUs: no workgroup would take a second frame"
    case = _Case(agx, orc, "rb64", n, 60, batch, primes=primes)
    lay = Layout(n, primes, batch, prime_stride=n + 1, poly_stride=primes * (n + 1) + 4)
    x = case.rand()
    want_f, want_i = case.forward(x, threads=8), case.inverse(x)
    rep = _Report()
    _strided_calls(case, dev, rep, "poly-major padded", lay, lay, False, x, want_f, want_i)
    # captured: out of place, so that a replay is repeatable
    src, dst = arena_for(dev, n, (lay, x)), arena_for(dev, n, (lay, None))
    warm = arena_for(dev, n, (lay, x))
    graph = capture(dev, lambda s: case.plan.inverse_strided(warm.address(0), warm.address(0), batch, lay.prime_stride, lay.poly_stride, s),   # warm-up on an arena of its own
                    lambda s: case.plan.inverse_strided(src.address(0), dst.address(0), batch, lay.prime_stride, lay.poly_stride, s))
    rep.check("capture must not run the launch", dst, [(lay, None)])
    rep.require("capture must not run the launch: an output frame holds results", not np.array_equal(dst.frames(lay), want_i))
    graph.replay()
    dev.sync()
    rep.check("captured inverse, output arena", dst, [(lay, want_i)])
    rep.check("captured inverse, input arena", src, [(lay, x)])
    case.close()
    rep.done()


@pytest.mark.parametrize("frames", [1, 128, 129, 1024, 1025, 2048, 3073])
def test_host_streaming_tails(agx, orc, frames):
    """Plan.forward_host_stream / inverse_host_stream of one plan at n = 4096: both sides of the 4 MiB small-input cutoff (128
    frames) and of the 32 MiB staging chunk (1,024 frames), an exact multiple of it, and four chunks (3,073 frames: the three
    staging slots are reused and a one-frame tail is drained).  `out` is a view at element offset 1 of a canary-filled host
    array whose bands must come back untouched; in2 differs from in for the forward"""
    n = 4096
    case = _Case(agx, orc, "rb64", n, 60, frames, primes=1)
    q, _, tw, pre = case.tabs[0]
    lay = Layout(n, 1, frames).at(1)
    a, b, y = case.rand(hi=1), case.rand(hi=1), case.rand(hi=1)
    mixed = a.reshape(frames, n).copy()
    mixed[:, n // 2:] = b.reshape(frames, n)[:, n // 2:]
    rep = _Report()
    out = GuardedArena(n, lay.span())
    got = case.plan.forward_host_stream(a, b, frames, out=out.view(1, frames * n))
    rep.require("forward_host_stream must return the caller's buffer", got.ctypes.data == out.address(1))
    rep.check("forward_host_stream", out, [(lay, orc.forward_mt(mixed.reshape(-1), q, tw, pre, n, 8))])
    out = GuardedArena(n, lay.span())
    case.plan.inverse_host_stream(y, frames, out=out.view(1, frames * n))
    rep.check("inverse_host_stream", out, [(lay, case.inverse(y))])
    case.close()
    rep.done()
