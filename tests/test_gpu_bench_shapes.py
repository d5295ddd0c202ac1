"""Parity at the launch shapes bench.py times (secondary_lines under --full), at launches past 2^31 and 2^32 elements, and the
refusal of frame layouts whose frames overlap one another.

Every output frame is covered: a full-batch differential against a twin plan forced onto the radix-2 LDS kernels (checked against
the oracle in test_gpu_parity.py::test_radix2_inverse_and_product_bit_exact), the shift property X^j * b on every product frame, and
the CPU oracle on frames copied back at the edges of the work decomposition.  All comparisons are exact: torch.equal on the device,
np.array_equal on the host."""
import numpy as np
import pytest

from gpu_util import EDGES, OracleRef as _Ref, big_memory, check_negacyclic_shifts, fill_monomials, frames_to_host as _frames      # noqa: F401  (big_memory: the fixture is used by name)
from gpu_util import radix2_twin, sample_frames as _sample, shift_exponents

pytestmark = pytest.mark.gpu


def _lazy(torch, x, moduli, seed):
    """x + q_p * k with k uniform in 0..3 per element: the same residues spread over the transforms' input range [0, 4q)"""
    g = torch.Generator(device=x.device)
    g.manual_seed(seed)
    k = torch.randint(0, 4, x.shape, generator=g, device=x.device, dtype=torch.int64)
    q = torch.tensor([int(v) for v in moduli], dtype=torch.int64, device=x.device)[:, None]
    return (x.view(len(moduli), -1) + q * k.view(len(moduli), -1)).view(-1)


def _check_oracle(kind, ref, frames, batch, got, *ins):
    for g in frames:
        want = getattr(ref, kind)(g // batch, *(x[g] for x in ins))
        assert np.array_equal(got[g], want), f"{kind}: frame {g % batch} of prime {g // batch} differs from the oracle"


def _check_transforms(torch, dev, plan, twin, ref, x, xl, batch, ops, in_place, frames):
    """forward / inverse of the lazy input xl (residues x) against the radix-2 twin on the whole batch and the oracle on `frames`,
    and the round trip back to x"""
    n = plan.n
    xl_h = _frames(xl, frames, n)
    for op in ("forward", "inverse"):
        if op not in ops:
            continue
        if in_place:
            y = xl.clone()
            getattr(plan, op)(y.data_ptr(), y.data_ptr(), batch, dev.stream)
        else:
            y = torch.empty_like(xl)
            getattr(plan, op)(xl.data_ptr(), y.data_ptr(), batch, dev.stream)
        y2 = torch.empty_like(xl)
        getattr(twin, op)(xl.data_ptr(), y2.data_ptr(), batch, dev.stream)
        dev.sync()
        assert torch.equal(y, y2), f"{op} differs from the radix-2 twin"
        _check_oracle(op, ref, frames, batch, _frames(y, frames, n), xl_h)
        back = "inverse" if op == "forward" else "forward"
        getattr(plan, back)(y.data_ptr(), y.data_ptr(), batch, dev.stream)
        dev.sync()
        assert torch.equal(y, x), f"{op} then {back} is not the identity on the residues"
        del y, y2


def _check_products(torch, dev, plan, twin, ref, xl, batch, aliasing, frames):
    """polymul with c distinct ("c"), c = a ("a"), c = b ("b"): against the radix-2 twin's three-launch product on the whole batch, the
    oracle on `frames`, and the shift property on every frame with the monomials X^j_f as the first and as the second operand"""
    n, primes = plan.n, plan.num_primes
    b = torch.empty_like(xl)
    plan.fill_synthetic(b.data_ptr(), batch, batch, 7, dev.stream)
    bl = _lazy(torch, b, plan.moduli, 2)
    want = torch.empty_like(xl)
    scratch = torch.empty_like(xl)
    twin.polymul(xl.data_ptr(), bl.data_ptr(), want.data_ptr(), scratch.data_ptr(), batch, dev.stream)
    del scratch
    u, v, c = torch.empty_like(xl), torch.empty_like(xl), torch.empty_like(xl)

    def run(first, second, alias):
        out = {"c": c, "a": first, "b": second}[alias]
        plan.polymul(first.data_ptr(), second.data_ptr(), out.data_ptr(), 0, batch, dev.stream)
        dev.sync()
        return out

    for alias in aliasing:
        u.copy_(xl)
        v.copy_(bl)
        assert torch.equal(run(u, v, alias), want), f"product (c = {alias}) differs from the radix-2 twin"
    _check_oracle("polymul", ref, frames, batch, _frames(want, frames, n), _frames(xl, frames, n), _frames(bl, frames, n))
    del want
    for alias in aliasing:
        for mono_first in (True, False):
            fill_monomials(torch, u, primes, batch, n)
            v.copy_(bl)
            got = run(u, v, alias) if mono_first else run(v, u, alias)
            bad = check_negacyclic_shifts(torch, got, b, plan.moduli, batch, n)
            assert not bad, f"X^j * b wrong (c = {alias}, monomials {'first' if mono_first else 'second'}): (prime, frames) {bad}"


# bench.py secondary_lines (slabs of 4 x 4096 x 4096 words, batch = words / (4 n)): plan, batch, in place, c = a as it times them
BENCH_SHAPES = [
    (32, 60, 4, 524288, ("forward", "inverse", "polymul")),
    (32, 30, 4, 524288, ("forward",)),
    (256, 60, 4, 65536, ("forward",)),
    (512, 60, 4, 32768, ("forward", "inverse", "polymul")),
    (512, 30, 4, 32768, ("forward",)),
    (1024, 30, 4, 4096, ("forward",)),
    (4096, 30, 4, 4096, ("forward", "inverse", "polymul")),
    (4096, 60, 4, 4096, ("inverse", "polymul")),
]


@pytest.mark.parametrize("n,bits,primes,batch,ops", BENCH_SHAPES)
def test_bench_secondary_shapes(agx, orc, dev, n, bits, primes, batch, ops):
    torch = dev.torch
    plan = agx.Plan(n, agx.find_primes(bits, n, primes))
    twin = radix2_twin(agx, plan)
    ref = _Ref(orc, plan)
    x = dev.empty(primes * batch * n)
    plan.fill_synthetic(x.data_ptr(), batch, 0, 42, dev.stream)
    xl = _lazy(torch, x, plan.moduli, 1)
    frames = _sample(primes, batch, n)
    _check_transforms(torch, dev, plan, twin, ref, x, xl, batch, ops, True, frames)
    if "polymul" in ops:
        _check_products(torch, dev, plan, twin, ref, xl, batch, ("a",), frames)
    plan.close()
    twin.close()


def test_bench_config5_slice_shape(agx, orc, dev):
    """n = 32768, one 60-bit prime, batch 1024: the product with c distinct, c = a and c = b; forward and inverse out of place"""
    torch = dev.torch
    n, batch = 32768, 1024
    plan = agx.Plan(n, agx.find_primes(60, n, 1))
    twin = radix2_twin(agx, plan)
    ref = _Ref(orc, plan)
    x = dev.empty(batch * n)
    plan.fill_synthetic(x.data_ptr(), batch, 0, 42, dev.stream)
    xl = _lazy(torch, x, plan.moduli, 3)
    frames = _sample(1, batch, n)
    _check_transforms(torch, dev, plan, twin, ref, x, xl, batch, ("forward", "inverse"), False, frames)
    _check_products(torch, dev, plan, twin, ref, xl, batch, ("c", "a", "b"), frames)
    plan.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# launches of more than 2^32 elements (34 GB and more per buffer: an MI355X holds 288 GB)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,primes,batch", [(4096, 4, 262400), (16384, 8, 33000), (32, 4, (1 << 25) + (1 << 20))])
def test_transforms_past_2_32_elements(agx, orc, dev, big_memory, n, primes, batch):
    """the default forward out of place against the radix-2 twin on the whole buffer and the oracle on both sides of element offsets
    2^28, 2^31 and 2^32 and at the last frame; then in place (must equal out of place) and the inverse in place back to the input
    (n = 16384: the inverse that hands frames out through a ticket counter; n = 32: the wave-packed kernels)"""
    torch = dev.torch
    total = primes * batch * n
    assert total > 1 << 32
    big_memory(3, total)
    plan = agx.Plan(n, agx.find_primes(60, n, primes))
    twin = radix2_twin(agx, plan)
    ref = _Ref(orc, plan)
    frames = _sample(primes, batch, n, EDGES + (total,))
    a, y, t = dev.empty(total), dev.empty(total), dev.empty(total)
    plan.fill_synthetic(a.data_ptr(), batch, 0, 11, dev.stream)
    a_h = _frames(a, frames, n)
    plan.forward(a.data_ptr(), y.data_ptr(), batch, dev.stream)
    twin.forward(a.data_ptr(), t.data_ptr(), batch, dev.stream)
    dev.sync()
    assert torch.equal(y, t), "forward differs from the radix-2 twin"
    _check_oracle("forward", ref, frames, batch, _frames(y, frames, n), a_h)
    plan.forward(a.data_ptr(), a.data_ptr(), batch, dev.stream)
    dev.sync()
    assert torch.equal(a, y), "forward in place differs from out of place"
    plan.inverse(a.data_ptr(), a.data_ptr(), batch, dev.stream)
    plan.fill_synthetic(t.data_ptr(), batch, 0, 11, dev.stream)        # the input again, regenerated instead of kept
    dev.sync()
    assert torch.equal(a, t), "inverse in place does not return the input"
    del a, y, t
    plan.close()
    twin.close()


def test_product_and_pointwise_past_2_32_elements(agx, orc, dev, big_memory):
    """n = 4096, one prime, batch 1,050,000: polymul(a, b, a) with a = X^j_f checked on every frame, pointwise with c aliasing the
    second operand checked on every element, and both against the oracle around element offsets 2^28, 2^31, 2^32 and at the end"""
    torch = dev.torch
    n, batch = 4096, 1050000
    total = batch * n
    assert total > 1 << 32
    big_memory(3, total)
    plan = agx.Plan(n, agx.find_primes(60, n, 1))
    q = plan.moduli[0]
    ref = _Ref(orc, plan)
    frames = _sample(1, batch, n, EDGES + (total,))
    m, b, w = dev.empty(total), dev.empty(total), dev.empty(total)
    fill_monomials(torch, m, 1, batch, n)
    plan.fill_synthetic(b.data_ptr(), batch, 0, 13, dev.stream)
    plan.polymul(m.data_ptr(), b.data_ptr(), m.data_ptr(), 0, batch, dev.stream)
    dev.sync()
    bad = check_negacyclic_shifts(torch, m, b, [q], batch, n)
    assert not bad, f"X^j * b wrong at (prime, frames) {bad}"
    b_h, c_h = _frames(b, frames, n), _frames(m, frames, n)
    j = shift_exponents(torch, 0, batch, n, "cpu").numpy()
    for g in frames:
        mono = np.zeros(n, dtype=np.uint64)
        mono[j[g]] = 1
        assert np.array_equal(c_h[g], ref.polymul(0, mono, b_h[g])), f"product frame {g} differs from the oracle"
    # pointwise on every element: w = k in 0..3 (from the element index), c = b o w written over w, expected k b mod q (< 2^62: exact)
    step = 1 << 27

    def small(lo, hi):
        i = torch.arange(lo, hi, dtype=torch.int64, device=w.device)
        return (i ^ (i >> 12)) % 4

    for lo in range(0, total, step):
        w[lo:min(total, lo + step)] = small(lo, min(total, lo + step))
    plan.pointwise(b.data_ptr(), w.data_ptr(), w.data_ptr(), batch, dev.stream)
    dev.sync()
    for lo in range(0, total, step):
        hi = min(total, lo + step)
        assert torch.equal(w[lo:hi], small(lo, hi) * b[lo:hi] % q), f"pointwise wrong in elements [{lo}, {hi})"
    # full-width operands: the product's output against b
    plan.pointwise(m.data_ptr(), b.data_ptr(), w.data_ptr(), batch, dev.stream)
    w_h = _frames(w, frames, n)
    for g in frames:
        assert np.array_equal(w_h[g], orc.pointwise(c_h[g], b_h[g], q)), f"pointwise frame {g} differs from the oracle"
    del m, b, w
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# frame layouts that overlap themselves or the other operand are refused
# ---------------------------------------------------------------------------------------------------------------------------------
def _touch_expected(n, primes, batch, prime_stride, poly_stride, off):
    """brute force over frame starts: two distinct frames of one set within n elements of each other, or (off != 0) any frame of the
    input within n elements of any frame of the output (which starts off elements later)"""
    starts = [p * prime_stride + b * poly_stride for p in range(primes) for b in range(batch)]
    for i, s in enumerate(starts):
        if any(abs(s - t) < n for t in starts[i + 1:]):
            return True
    return off != 0 and any(abs(s - t - off) < n for s in starts for t in starts)


@pytest.mark.parametrize("n", [32, 4096])
def test_overlapping_layouts_are_rejected(agx, orc, dev, n):
    """forward_strided / inverse_strided over a grid of layouts (2 or 3 primes, 1 to 3 polynomials, strides from 0 to B n + 8) and output
    offsets (0, +-1, +-n/2, +-n, +B n): status 5 exactly when the brute-force predicate finds touching frames, with memory untouched;
    every accepted call matches the oracle frame for frame and leaves every word outside its output frames as it was.  The buffer
    holds every layout of the grid (accepted or not) with n words to spare on both sides."""
    torch = dev.torch
    pad, span = 2 * n, 2 * (3 * n + 8) + 2 * (3 * n + 8) + n + 3 * n      # (P-1) ps + (B-1) qs + n, + the largest offset
    size = pad + span + pad
    wrong = {}      # layout -> [what went wrong, per call]
    for primes in (2, 3):
        plan = agx.Plan(n, [orc.find_prime(60, n, k) for k in range(primes)])
        ref = _Ref(orc, plan)
        rng = np.random.default_rng(n + primes)
        x = rng.integers(0, min(plan.moduli), size=size, dtype=np.uint64)
        keep = dev.to_device(x)
        d = dev.to_device(x)
        base = d.data_ptr() + 8 * pad
        for batch in (1, 2, 3):
            strides = sorted({0, 1, n // 2, n - 1, n, n + 1, 2 * n, 3 * n, batch * n, batch * n + 8})
            offs = sorted({0, 1, -1, n // 2, -(n // 2), n, -n, batch * n})
            for ps in strides:
                for qs in strides:
                    bad = wrong.setdefault(f"P={primes} B={batch} prime_stride={ps} poly_stride={qs}", [])
                    for off in offs:
                        reject = _touch_expected(n, primes, batch, ps, qs, off)
                        for op in ("forward", "inverse"):
                            try:
                                getattr(plan, op + "_strided")(base, base + 8 * off, batch, ps, qs, dev.stream)
                                status = 0
                            except agx.AgxError as e:
                                status = e.status
                            if reject:
                                if status != 5:
                                    bad.append(f"{op} out {off:+d}: status {status}, want 5")
                                    d.copy_(keep)
                                continue
                            if status != 0:
                                bad.append(f"{op} out {off:+d}: status {status}, want 0")
                                continue
                            got = dev.to_host(d)
                            d.copy_(keep)
                            want = x.copy()
                            for p in range(primes):
                                for b in range(batch):
                                    lo = pad + p * ps + b * qs
                                    want[lo + off:lo + off + n] = getattr(ref, op)(p, x[lo:lo + n])
                            if not np.array_equal(got, want):
                                bad.append(f"{op} out {off:+d}: output or words outside the output frames differ")
                    dev.sync()
                    if not torch.equal(d, keep):
                        bad.append("a rejected call changed memory")
                        d.copy_(keep)
        plan.close()
    wrong = {k: v for k, v in wrong.items() if v}
    assert not wrong, f"{len(wrong)} layouts handled wrongly:\n" + "\n".join(f"{k}: {'; '.join(v[:4])}" for k, v in list(wrong.items())[:60])


@pytest.mark.parametrize("n", [32, 4096])
def test_layouts_that_do_not_fit_are_refused(agx, orc, dev, n):
    """forward_strided / inverse_strided with a stride of 2^61 or 2^61 + n words between two polynomials (one prime, batch 2) or between two
    primes (two primes, batch 1): the extent is past 2^60 words, byte offsets no longer fit 64 bits, so the call is refused with status 5
    before anything is launched and every word stays as it was.  2^61 words are 2^64 bytes: the second frame of a build that wrongly
    accepted such a call would wrap onto word 0 or n of the 2n-word payload, inside the buffer (n guard words on both sides)."""
    torch = dev.torch
    wrong = []
    for primes in (1, 2):
        plan = agx.Plan(n, [orc.find_prime(60, n, k) for k in range(primes)])
        x = np.random.default_rng(n + primes).integers(0, min(plan.moduli), size=4 * n, dtype=np.uint64)
        keep, d = dev.to_device(x), dev.to_device(x)
        base = d.data_ptr() + 8 * n
        for stride in ((1 << 61), (1 << 61) + n):
            batch, ps, qs = (2, 2 * n, stride) if primes == 1 else (1, stride, n)
            for op in ("forward", "inverse"):
                try:
                    getattr(plan, op + "_strided")(base, base, batch, ps, qs, dev.stream)
                    status = 0
                except agx.AgxError as e:
                    status = e.status
                dev.sync()
                if status != 5:
                    wrong.append(f"{op} P={primes} B={batch} prime_stride={ps} poly_stride={qs}: status {status}, want 5")
                if not torch.equal(d, keep):
                    wrong.append(f"{op} P={primes} B={batch} prime_stride={ps} poly_stride={qs}: memory changed")
                    d.copy_(keep)
        plan.close()
    assert not wrong, "\n".join(wrong)
