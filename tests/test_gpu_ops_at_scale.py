"""agx_ntt_automorphism, agx_ntt_rescale and the generic path of agx_ntt_polymul_ntt at the smallest launches whose grid-stride loops
take a second trip (a launch holds at most 16,384 blocks of 256 threads per grid row: TRIP work items), whose loop inverse walks over
more frames than its resident grid holds, and past element offsets 2^31 and 2^32.

Every output word is judged on the device by a reference that shares nothing with the kernel under test (gpu_util.py; the checkers
are tested themselves in test_scale_checkers.py), and frames copied back at the edges of the work decomposition are judged by the CPU
oracle and by Python integers.  All comparisons are exact: torch.equal on the device, np.array_equal on the host."""
import numpy as np
import pytest

from gpu_util import (EDGES, OracleRef, big_memory, boundary_frames, capture, check_automorphism_coeff, check_automorphism_ntt,      # noqa: F401  (big_memory: the fixture is used by name)
                      check_fixed_shifts, check_rescale_identity, fill_rescale_constants, frames_to_host, library_find_prime, loop_batch, moduli_for,
                      radix2_twin, rescale_identity_sum_, rescale_reference, resident_grid, sample_frames, sigma, spread_lazy_, thin_frames)

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
FLOOR, ROUND = 0, 1
TRIP = 2048 * 8 * 256      # work items of one trip round a grid-stride loop (grid_1d, csrc/ntt_kernels.hip)


def _where(bad):
    return "; ".join(f"prime {p} frame {f} element {e}" for p, f, e in bad)


def _first_difference(torch, got, want, batch, n):
    """'prime p frame f element e' of the first differing word of two dense [prime][batch][n] buffers"""
    step = 1 << 27
    for lo in range(0, got.numel(), step):
        d = (got[lo:lo + step] != want[lo:lo + step]).nonzero()
        if d.numel():
            i = lo + int(d[0])
            return f"prime {i // (batch * n)} frame {(i // n) % batch} element {i % n} (word {i})"
    return "no difference"


def _assert_equal(torch, got, want, batch, n, what):
    assert torch.equal(got, want), f"{what}: first difference at {_first_difference(torch, got, want, batch, n)}"


# ---------------------------------------------------------------------------------------------------------------------------------
# agx_ntt_automorphism
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_automorphism(torch, dev, plan, ref, a, out, batch, frames, gs, what):
    """a: residues in [0, 4q) (coefficient form), consumed: both forms for every g of gs on the whole buffer (device checkers) and on
    `frames` (global frame numbers) against the definition as a scatter and the oracle's transform of it"""
    n, moduli = plan.n, plan.moduli
    a_h = frames_to_host(a, frames, n)
    for g in gs:
        out.fill_(-1)
        plan.automorphism(a.data_ptr(), out.data_ptr(), batch, g, COEFF, dev.stream)
        dev.sync()
        bad = check_automorphism_coeff(torch, out, a, moduli, batch, n, g)
        assert not bad, f"{what}, coefficient form, g = {g}: {_where(bad)}"
        got = frames_to_host(out, frames, n)
        for f in frames:
            assert np.array_equal(got[f], sigma(a_h[f], g, n, moduli[f // batch])), \
                f"{what}, coefficient form, g = {g}: frame {f % batch} of prime {f // batch} differs from the definition"
    plan.forward(a.data_ptr(), a.data_ptr(), batch, dev.stream)      # a <- its transform, in place
    for g in gs:
        out.fill_(-1)
        plan.automorphism(a.data_ptr(), out.data_ptr(), batch, g, NTT, dev.stream)
        dev.sync()
        bad = check_automorphism_ntt(torch, out, a, batch, n, g)
        assert not bad, f"{what}, NTT form, g = {g}: {_where(bad)}"
        got = frames_to_host(out, frames, n)
        for f in frames:
            p = f // batch
            assert np.array_equal(got[f], ref.forward(p, sigma(a_h[f], g, n, moduli[p]))), \
                f"{what}, NTT form, g = {g}: frame {f % batch} of prime {p} differs from the oracle's transform of sigma_g(a)"


# n, moduli, batch, base at an odd word, work items that must exceed TRIP: words of a prime (coefficient form), words or pairs of the call (NTT form)
AUTOMORPHISM = [
    (4096, (60, 30, 61), 1100, False, ("per_prime", "pairs")),      # the 16-byte kernel: 6.76 M pairs
    (4096, (60, 30, 61), 1100, True, ("per_prime", "words")),       # the 8-byte kernel: 13.5 M words
    (32, (60, 60), 140000, False, ("per_prime", "pairs")),
    (32768, (60,), 130, False, ("per_prime",)),                     # 2.13 M pairs: one trip of the 16-byte kernel
    (32768, (60,), 130, True, ("per_prime", "words")),
]


@pytest.mark.parametrize("n,spec,batch,odd,second_trip", AUTOMORPHISM)
def test_automorphism_past_one_grid_stride_trip(agx, orc, dev, n, spec, batch, odd, second_trip):
    """g in {5, 2n-1, n+1}, inputs in [0, 4q) for the coefficient form; both buffers at an even or at an odd word of a larger allocation"""
    torch = dev.torch
    moduli = list(moduli_for(library_find_prime(agx), n, spec))
    primes, total = len(moduli), len(moduli) * batch * n
    items = {"per_prime": batch * n, "words": total, "pairs": total // 2}
    for k in second_trip:
        assert items[k] > TRIP, (k, items[k])
    plan = agx.Plan(n, moduli)
    ref = OracleRef(orc, plan)
    off = 1 if odd else 0
    room_a, room_o = dev.empty(total + 2), dev.empty(total + 2)
    a, out = room_a[off:off + total], room_o[off:off + total]
    assert a.data_ptr() % 16 == 8 * off and out.data_ptr() % 16 == 8 * off
    plan.fill_synthetic(a.data_ptr(), batch, 0, 21, dev.stream)
    dev.sync()
    spread_lazy_(torch, a, moduli, 4)
    room_o.fill_(-1)
    _check_automorphism(torch, dev, plan, ref, a, out, batch, sample_frames(primes, batch, n), (5, 2 * n - 1, n + 1), (n, spec, batch, "odd" if odd else "even"))
    assert all(int(room_o[k]) == -1 for k in ((0, total + 1) if odd else (total, total + 1))), "a word next to the output changed"
    plan.close()


def test_automorphism_past_2_32_elements(agx, orc, dev, big_memory):
    """n = 4096, four 60-bit primes, batch 262,400 (two buffers of 34 GB): every word on the device, and the frames on both sides of element
    offsets 2^28, 2^31, 2^32 and at the end on the host"""
    torch = dev.torch
    n, primes, batch = 4096, 4, 262400
    total = primes * batch * n
    assert total > 1 << 32
    big_memory(2, total)
    plan = agx.Plan(n, agx.find_primes(60, n, primes))
    ref = OracleRef(orc, plan)
    frames = sample_frames(primes, batch, n, EDGES + (total,))
    a, out = dev.empty(total), dev.empty(total)
    plan.fill_synthetic(a.data_ptr(), batch, 0, 23, dev.stream)
    dev.sync()
    spread_lazy_(torch, a, plan.moduli, 6)
    _check_automorphism(torch, dev, plan, ref, a, out, batch, frames, (5, 2 * n - 1, n + 1), "past 2^32")
    del a, out
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# agx_ntt_polymul_ntt, generic path: forward, pointwise_bhat_kernel, inverse
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,spec,batch,radix2", [(512, (60, 60), 8300, False), (4096, (30, 30), 1100, False), (16384, (60, 60), 260, True)])
def test_polymul_ntt_generic_path_past_one_grid_stride_trip(agx, orc, dev, n, spec, batch, radix2):
    """n <= 512, all-narrow moduli and plans forced onto the radix-2 kernels take the three-launch path.  a in [0, 4q); the whole batch
    against agx_ntt_polymul of a default plan (one fused kernel, no pointwise pass) with c distinct: dense, then broadcast against the
    product with the one b frame tiled; the oracle on the boundary frames"""
    torch = dev.torch
    moduli = list(moduli_for(library_find_prime(agx), n, spec))
    primes, total = len(moduli), len(moduli) * batch * n
    assert batch * n > TRIP
    fused = agx.Plan(n, moduli)
    plan = agx.Plan(n, moduli, psi=[fused.psi(p) for p in range(primes)])
    if radix2:
        plan.set_variant(agx.VARIANT_LDS_RADIX2)
    ref = OracleRef(orc, fused)
    frames = sample_frames(primes, batch, n)
    a, b, bhat, want, c = (dev.empty(total) for _ in range(5))
    fused.fill_synthetic(a.data_ptr(), batch, 0, 31, dev.stream)
    fused.fill_synthetic(b.data_ptr(), batch, batch, 31, dev.stream)
    dev.sync()
    spread_lazy_(torch, a, moduli, 8)
    a_h = frames_to_host(a, frames, n)
    # dense
    fused.polymul(a.data_ptr(), b.data_ptr(), want.data_ptr(), 0, batch, dev.stream)
    plan.forward(b.data_ptr(), bhat.data_ptr(), batch, dev.stream)
    c.fill_(-1)
    plan.polymul_ntt(a.data_ptr(), bhat.data_ptr(), c.data_ptr(), batch, batch, dev.stream)
    dev.sync()
    _assert_equal(torch, c, want, batch, n, "dense")
    b_h, c_h = frames_to_host(b, frames, n), frames_to_host(c, frames, n)
    for f in frames:
        assert np.array_equal(c_h[f], ref.polymul(f // batch, a_h[f], b_h[f])), f"dense: frame {f % batch} of prime {f // batch} differs from the oracle"
    # broadcast: frame 0 of every prime's b, shared by the whole batch
    b1 = b.view(primes, batch, n)[:, 0].contiguous().view(-1)
    bhat1 = torch.empty_like(b1)
    plan.forward_lazy(b1.data_ptr(), bhat1.data_ptr(), 1, dev.stream)
    b.view(primes, batch, n)[:] = b1.view(primes, 1, n)
    fused.polymul(a.data_ptr(), b.data_ptr(), want.data_ptr(), 0, batch, dev.stream)
    c.fill_(-1)
    plan.polymul_ntt(a.data_ptr(), bhat1.data_ptr(), c.data_ptr(), batch, 1, dev.stream)
    dev.sync()
    _assert_equal(torch, c, want, batch, n, "broadcast")
    c_h = frames_to_host(c, frames, n)
    for f in frames:
        assert np.array_equal(c_h[f], ref.polymul(f // batch, a_h[f], b_h[(f // batch) * batch])), f"broadcast: frame {f % batch} of prime {f // batch} differs from the oracle"
    plan.close()
    fused.close()


def test_polymul_ntt_generic_path_past_2_32_elements(agx, orc, dev, big_memory):
    """n = 32, four 60-bit primes, batch 2^25 + 2^20, broadcast, c = a: bhat is the transform of X^j_p, one j per prime, so every frame of c
    must be a's frame shifted negacyclically by j_p -- built with torch on every frame; the oracle round the offsets 2^28, 2^31, 2^32
    and at the end"""
    torch = dev.torch
    n, primes, batch = 32, 4, (1 << 25) + (1 << 20)
    total = primes * batch * n
    assert total > 1 << 32 and batch * n > TRIP
    big_memory(2, total)
    plan = agx.Plan(n, agx.find_primes(60, n, primes))
    ref = OracleRef(orc, plan)
    shifts = [1, 13, n - 1, 6]
    frames = sample_frames(primes, batch, n, EDGES + (total,))
    mono = np.zeros((primes, n), dtype=np.uint64)
    mono[np.arange(primes), shifts] = 1
    d_mono, bhat = dev.to_device(mono.reshape(-1)), dev.empty(primes * n)
    plan.forward(d_mono.data_ptr(), bhat.data_ptr(), 1, dev.stream)
    a, keep = dev.empty(total), dev.empty(total)
    plan.fill_synthetic(a.data_ptr(), batch, 0, 33, dev.stream)
    plan.fill_synthetic(keep.data_ptr(), batch, 0, 33, dev.stream)
    plan.polymul_ntt(a.data_ptr(), bhat.data_ptr(), a.data_ptr(), batch, 1, dev.stream)
    dev.sync()
    bad = check_fixed_shifts(torch, a, keep, plan.moduli, batch, n, shifts)
    assert not bad, f"X^j * a wrong at {_where(bad)}"
    a_h, c_h = frames_to_host(keep, frames, n), frames_to_host(a, frames, n)
    for f in frames:
        assert np.array_equal(c_h[f], ref.polymul(f // batch, a_h[f], mono[f // batch])), f"frame {f % batch} of prime {f // batch} differs from the oracle"
    del a, keep
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# agx_ntt_rescale
# ---------------------------------------------------------------------------------------------------------------------------------
def _identity_operands(torch, dev, plan, batch, seed):
    """(y, x): y = one fill_synthetic call over [P][batch][n] (slabs 0 .. P-2: the residues of Y, the last slab: r), x = the residues of
    X = Y q_L + r in coefficient form: the product y o C by the plan's pointwise, the sum with torch (gpu_util.rescale_identity_sum_)"""
    total = plan.num_primes * batch * plan.n
    y, x = dev.empty(total), dev.empty(total)
    plan.fill_synthetic(y.data_ptr(), batch, 0, seed, dev.stream)
    fill_rescale_constants(torch, x, plan.moduli)
    plan.pointwise(y.data_ptr(), x.data_ptr(), x.data_ptr(), batch, dev.stream)
    dev.sync()
    rescale_identity_sum_(torch, x, y, plan.moduli)
    return y, x


def _to_ntt_form(dev, plan, x, xhat, batch, mode):
    """forward for one mode, forward_lazy for the other"""
    (plan.forward if mode == FLOOR else plan.forward_lazy)(x.data_ptr(), xhat.data_ptr(), batch, dev.stream)


def _rescale_frames(batch, n, resident, edges=()):
    """frame numbers (within a prime) for the Python-integer check: the boundary frames; from n = 16384 on at most 16, among them 0, 1,
    batch - 3, batch - 1 and both sides of the resident grid"""
    frames = boundary_frames(batch, extra=edges)
    if n >= 16384:
        frames = thin_frames(frames, [0, 1, batch - 3, batch - 1, resident - 1, resident] + list(edges))
    return frames


def _host_reference(torch, x, moduli, batch, n, frames):
    """{mode: [P-1][len(frames)][n] words of Y mod q_i}: the frames of x (all P residues) copied back, X rebuilt per coefficient by CRT"""
    P = len(moduli)
    idx = torch.tensor(frames, device=x.device)
    res = x.view(P, batch, n)[:, idx].cpu().numpy().view(np.uint64).reshape(P, -1)
    return {mode: rescale_reference(res, moduli, mode).reshape(P - 1, len(frames), n) for mode in (FLOOR, ROUND)}


def _check_sampled(torch, ref, out, want, batch, n, frames, what):
    """the NTT-form output frames against the oracle's transform of Y mod q_i"""
    idx = torch.tensor(frames, device=out.device)
    got = out.view(-1, batch, n)[:want.shape[0], idx].cpu().numpy().view(np.uint64)
    for p in range(want.shape[0]):
        for k, f in enumerate(frames):
            assert np.array_equal(got[p, k], ref.forward(p, want[p, k])), f"{what}: frame {f} of prime {p} differs from the oracle's transform of Y mod q"


RESCALE = [
    # n, moduli, batch (None: from the device's CU count), what the case is there for
    (4096, (60, 60, 60), 1100, "fused"),
    (16384, (60, 60), None, "loop"),
    (32768, (60, 60), None, "loop"),
    (512, (60, 60, 60), 8300, "generic"),
    (4096, (30, 30, 30), 1100, "generic"),
    (4096, (60, 30, 61), 1100, "mixed"),
]


@pytest.mark.parametrize("n,spec,batch,kind", RESCALE)
def test_rescale_past_one_grid_stride_trip_and_one_resident_grid(agx, orc, dev, n, spec, batch, kind):
    """both modes (floor from forward's output, round from forward_lazy's), out of place with a scratch of its own and in place with x's
    last slab as the scratch: the two must agree word for word; the inverse of the output must be the constructed quotient on every
    word; the output frames at the edges of the work decomposition must be the oracle's transform of Y mod q_i, Y from Python integers.
    Where the two-launch route serves the plan (n >= 1024 and some modulus of 2^31 or more) the radix-2 twin's four launches must give
    the same words."""
    torch = dev.torch
    moduli = list(moduli_for(library_find_prime(agx), n, spec))
    P = len(moduli)
    resident = resident_grid(torch, n)
    if kind == "loop":
        batch = loop_batch(torch, n)
        assert batch > resident and batch % resident != 0, (batch, resident)      # the last slab alone: more frames than workgroups, a ragged last round
    else:
        assert batch * n > TRIP
    slab, head = batch * n, (P - 1) * batch * n
    plan = agx.Plan(n, moduli)
    ref = OracleRef(orc, plan)
    twin = radix2_twin(agx, plan) if n >= 1024 and max(moduli) >= 1 << 31 else None
    y, x = _identity_operands(torch, dev, plan, batch, 51)
    frames = _rescale_frames(batch, n, resident)
    want = _host_reference(torch, x, moduli, batch, n, frames)
    xhat, out, scratch = dev.empty(P * slab), dev.empty(P * slab), dev.empty(slab)
    for mode in (FLOOR, ROUND):
        what = (n, spec, batch, "round" if mode else "floor")
        _to_ntt_form(dev, plan, x, xhat, batch, mode)
        out.fill_(-1)
        plan.rescale(xhat.data_ptr(), out.data_ptr(), scratch.data_ptr(), batch, mode, dev.stream)
        dev.sync()
        assert int(out[head]) == -1 and int(out[-1]) == -1, "out of place: a word behind the output changed"
        _check_sampled(torch, ref, out, want[mode], batch, n, frames, what)
        if twin is not None:
            t_out, t_s = dev.empty(head), dev.empty(slab)
            twin.rescale(xhat.data_ptr(), t_out.data_ptr(), t_s.data_ptr(), batch, mode, dev.stream)
            dev.sync()
            _assert_equal(torch, out[:head], t_out, batch, n, f"{what}: the radix-2 twin")
            del t_out, t_s
        plan.rescale(xhat.data_ptr(), xhat.data_ptr(), xhat.data_ptr() + 8 * head, batch, mode, dev.stream)      # in place: xhat is consumed
        dev.sync()
        _assert_equal(torch, xhat[:head], out[:head], batch, n, f"{what}: in place against out of place")
        out[head:].zero_()
        plan.inverse(out.data_ptr(), out.data_ptr(), batch, dev.stream)
        dev.sync()
        bad = check_rescale_identity(torch, out, y, moduli, batch, n, mode)
        assert not bad, f"{what}: not the constructed quotient at {_where(bad)}"
    plan.close()
    if twin is not None:
        twin.close()


def test_rescale_stateless_loop_inverse_in_a_graph(agx, orc, dev):
    """n = 16384 captured: the loop inverse takes its fixed-stride form, on more frames than its resident grid holds.  A floor and a
    round call captured one after the other on a side stream (one branch), replayed once; each output must be the constructed quotient
    on every word and equal the eager call's"""
    torch = dev.torch
    n, spec = 16384, (60, 60)
    moduli = list(moduli_for(library_find_prime(agx), n, spec))
    P = len(moduli)
    batch, resident = loop_batch(torch, n), resident_grid(torch, n)
    assert batch > resident and batch % resident != 0, (batch, resident)
    slab, head = batch * n, (P - 1) * batch * n
    plan = agx.Plan(n, moduli)
    y, x = _identity_operands(torch, dev, plan, batch, 53)
    xhat = dev.empty(P * slab)
    plan.forward(x.data_ptr(), xhat.data_ptr(), batch, dev.stream)
    outs = [dev.empty(P * slab) for _ in (FLOOR, ROUND)]
    eager, scratch = dev.empty(P * slab), dev.empty(slab)

    def both_modes(s):
        for mode in (FLOOR, ROUND):
            plan.rescale(xhat.data_ptr(), outs[mode].data_ptr(), scratch.data_ptr(), batch, mode, s)

    graph = capture(dev, lambda s: plan.rescale(xhat.data_ptr(), eager.data_ptr(), scratch.data_ptr(), batch, FLOOR, s), both_modes)      # warm-up into a buffer of its own
    for o in outs:
        o.fill_(-1)
    graph.replay()
    dev.sync()
    for mode in (FLOOR, ROUND):
        plan.rescale(xhat.data_ptr(), eager.data_ptr(), scratch.data_ptr(), batch, mode, dev.stream)
        dev.sync()
        _assert_equal(torch, outs[mode][:head], eager[:head], batch, n, f"replay against the eager call, mode {mode}")
        outs[mode][head:].zero_()
        plan.inverse(outs[mode].data_ptr(), outs[mode].data_ptr(), batch, dev.stream)
        dev.sync()
        bad = check_rescale_identity(torch, outs[mode], y, moduli, batch, n, mode)
        assert not bad, f"replayed mode {mode}: not the constructed quotient at {_where(bad)}"
    plan.close()


def test_rescale_past_2_32_elements(agx, orc, dev, big_memory):
    """n = 4096, five 60-bit primes, batch 262,400 (two buffers of 43 GB), in place, both modes: the constructed quotient on every word,
    and Python integers on the frames round element offsets 2^28, 2^31, 2^32 and at the end of the output"""
    torch = dev.torch
    n, P, batch = 4096, 5, 262400
    total, head = P * batch * n, (P - 1) * batch * n
    assert head > 1 << 32
    big_memory(2, total)
    plan = agx.Plan(n, agx.find_primes(60, n, P))
    moduli = plan.moduli
    ref = OracleRef(orc, plan)
    edges = sorted({g % batch for e in EDGES + (head,) for g in ((e - 1) // n, e // n)})
    frames = sorted(set(edges) | {0, 1, batch - 3, batch - 1})
    y, x = _identity_operands(torch, dev, plan, batch, 55)
    want = _host_reference(torch, x, moduli, batch, n, frames)
    for mode in (FLOOR, ROUND):
        if mode == ROUND:      # x again: the same construction, in place of a third buffer
            fill_rescale_constants(torch, x, moduli)
            plan.pointwise(y.data_ptr(), x.data_ptr(), x.data_ptr(), batch, dev.stream)
            dev.sync()
            rescale_identity_sum_(torch, x, y, moduli)
        _to_ntt_form(dev, plan, x, x, batch, mode)
        plan.rescale(x.data_ptr(), x.data_ptr(), x.data_ptr() + 8 * head, batch, mode, dev.stream)
        dev.sync()
        _check_sampled(torch, ref, x, want[mode], batch, n, frames, f"past 2^32, mode {mode}")
        plan.inverse(x.data_ptr(), x.data_ptr(), batch, dev.stream)      # the last slab holds the scratch's coefficients in [0, q_L): any input will do
        dev.sync()
        bad = check_rescale_identity(torch, x, y, moduli, batch, n, mode)
        assert not bad, f"past 2^32, mode {mode}: not the constructed quotient at {_where(bad)}"
    del x, y
    plan.close()
