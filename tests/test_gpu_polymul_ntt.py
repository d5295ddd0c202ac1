"""agx_ntt_polymul_ntt on the device: c = a * b in Z_q[X]/(X^n + 1) with b given by its transform bhat (what forward / forward_lazy
of the same plan wrote), one bhat frame per frame (dense) or one per prime shared by the whole batch (broadcast).

Every comparison is exact (== on uint64 words): the results are fully reduced.  The expected words come from the CPU oracle's own
NTT pipeline (gpu_util.oracle_polymul) and, on whole batches, from agx_ntt_polymul and from the shift property X^j * b."""
import numpy as np
import pytest

from gpu_util import (REGISTRY, boundary_frames, capture, check_negacyclic_shifts, fill_monomials, group_of_two, moduli_for, oracle_polymul,
                      oracle_tables, plan_from_oracle_tables, rand_coeffs, select_entry, status_of)

pytestmark = pytest.mark.gpu

SIZES = [2, 16, 32, 512, 1024, 2048, 4096, 8192, 16384, 32768]
# modulus classes: 60 bits (16q-lazy kernels), 61 (fast), 62 (exact), 31 and 30 (the 32-bit kernels' two tiers)
CLASSES = [60, 61, 62, 31, 30]


def _operands(rng, tabs, batch, n, bits, b_batch=None):
    """a in [0,4q) ([0,3q) at 62 bits: 4q would not fit 64 bits), b in [0,q); [prime][batch][n] each (b: [prime][b_batch][n])"""
    hi = 4 if bits < 62 else 3
    a = np.concatenate([rand_coeffs(rng, batch * n, t[0], hi_mult=hi) for t in tabs])
    b = np.concatenate([rand_coeffs(rng, (batch if b_batch is None else b_batch) * n, t[0]) for t in tabs])
    return a, b


def _oracle(orc, a, b, tabs, batch, n, frames=None, b_batch=None):
    """{(prime, frame): expected words} for the listed frames (default: all); b_batch = 1: every frame meets b's frame (p, 0)"""
    bb = batch if b_batch is None else b_batch
    want = {}
    for p, t in enumerate(tabs):
        for f in (range(batch) if frames is None else frames):
            fb = f if bb == batch else 0
            sa = slice((p * batch + f) * n, (p * batch + f + 1) * n)
            sb = slice((p * bb + fb) * n, (p * bb + fb + 1) * n)
            want[(p, f)] = oracle_polymul(orc, a[sa], b[sb], t[0], t[1], n)
    return want


def _assert_frames(got, want, batch, n, what):
    for (p, f), w in want.items():
        assert np.array_equal(got[(p * batch + f) * n:(p * batch + f + 1) * n], w), f"{what}: frame {f} of prime {p} differs from the oracle"


@pytest.mark.parametrize("bits", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_against_the_oracle(agx, orc, dev, n, bits):
    """two primes, a ragged batch; bhat from forward and, separately, from forward_lazy: both must give the oracle's words, which
    are also what agx_ntt_polymul writes for (a, b)"""
    primes = 2
    batch = 259 if n <= 512 else 5
    plan, tabs = plan_from_oracle_tables(agx, orc, n, bits, primes)
    rng = np.random.default_rng(n * 101 + bits)
    a, b = _operands(rng, tabs, batch, n, bits)
    want = _oracle(orc, a, b, tabs, batch, n, frames=boundary_frames(batch) if n <= 512 else None)
    d_a, d_b = dev.to_device(a), dev.to_device(b)
    d_ref, d_s = dev.empty(a.size), dev.empty(a.size)
    plan.polymul(d_a.data_ptr(), d_b.data_ptr(), d_ref.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    ref = dev.to_host(d_ref)
    _assert_frames(ref, want, batch, n, "polymul")
    for fwd in ("forward", "forward_lazy"):
        d_bhat, d_c = dev.empty(a.size), dev.empty(a.size)
        getattr(plan, fwd)(d_b.data_ptr(), d_bhat.data_ptr(), batch, dev.stream)
        bhat = dev.to_host(d_bhat)
        plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, stream=dev.stream)
        got = dev.to_host(d_c)
        _assert_frames(got, want, batch, n, f"polymul_ntt (bhat by {fwd})")
        assert np.array_equal(got, ref), f"polymul_ntt (bhat by {fwd}) differs from polymul"
        assert np.array_equal(dev.to_host(d_a), a) and np.array_equal(dev.to_host(d_bhat), bhat), "operands changed"
    plan.close()


@pytest.mark.parametrize("n,bits,batch", [(32, 60, 259), (512, 30, 259), (1024, 60, 37), (4096, 60, 261), (4096, 62, 9), (4096, 30, 9),
                                          (8192, 61, 5), (16384, 60, 300), (32768, 60, 7), (32768, 62, 5), (4096, 60, 1), (32768, 60, 1), (2, 61, 1)])
def test_broadcast(agx, orc, dev, n, bits, batch):
    """bhat_batch = 1: the whole batch equals the dense call on bhat tiled `batch` times, and the oracle on the boundary frames"""
    torch = dev.torch
    primes = 2
    plan, tabs = plan_from_oracle_tables(agx, orc, n, bits, primes)
    rng = np.random.default_rng(n * 7 + bits + batch)
    a, b = _operands(rng, tabs, batch, n, bits, b_batch=1)
    d_a, d_b = dev.to_device(a), dev.to_device(b)
    d_bhat = dev.empty(b.size)
    plan.forward(d_b.data_ptr(), d_bhat.data_ptr(), 1, dev.stream)
    d_tiled = d_bhat.view(primes, 1, n).expand(primes, batch, n).contiguous().view(-1)
    d_c, d_d = dev.empty(a.size), dev.empty(a.size)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, 1, dev.stream)
    plan.polymul_ntt(d_a.data_ptr(), d_tiled.data_ptr(), d_d.data_ptr(), batch, batch, dev.stream)
    dev.sync()
    assert torch.equal(d_c, d_d), "broadcast differs from the dense call on the tiled bhat"
    want = _oracle(orc, a, b, tabs, batch, n, frames=boundary_frames(batch), b_batch=1)
    _assert_frames(dev.to_host(d_c), want, batch, n, "broadcast")
    assert np.array_equal(dev.to_host(d_a), a)
    plan.close()


def _dense_and_broadcast(agx, orc, dev, plan, tabs, n, bits, seed, what):
    batch = 3
    rng = np.random.default_rng(seed)
    a, b = _operands(rng, tabs, batch, n, bits)
    d_a, d_b, d_bhat, d_c = dev.to_device(a), dev.to_device(b), dev.empty(a.size), dev.empty(a.size)
    plan.forward(d_b.data_ptr(), d_bhat.data_ptr(), batch, dev.stream)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, batch, dev.stream)       # no scratch anywhere
    _assert_frames(dev.to_host(d_c), _oracle(orc, a, b, tabs, batch, n), batch, n, f"{what} dense")
    # broadcast: frame 1 of every prime's b as the shared operand
    b1 = np.concatenate([b[(p * batch + 1) * n:(p * batch + 2) * n] for p in range(len(tabs))])
    d_b1, d_bhat1 = dev.to_device(b1), dev.empty(b1.size)
    plan.forward_lazy(d_b1.data_ptr(), d_bhat1.data_ptr(), 1, dev.stream)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat1.data_ptr(), d_c.data_ptr(), batch, 1, dev.stream)
    _assert_frames(dev.to_host(d_c), _oracle(orc, a, b1, tabs, batch, n, b_batch=1), batch, n, f"{what} broadcast")


@pytest.mark.parametrize("config,n,max_bits", REGISTRY)
def test_every_registry_entry_at_its_own_size(agx, orc, dev, config, n, max_bits):
    """each registry id selected explicitly at its size, under the largest modulus its arithmetic admits and a 30-bit one, two
    primes: dense and broadcast against the oracle.  Entries without a kernel of their own for this product (forward-only ids, the
    32-bit and wave-packed families) are served by the generic path, without scratch."""
    for bits in (max_bits, 30):
        plan, tabs = plan_from_oracle_tables(agx, orc, n, bits, 2)
        select_entry(agx, plan, config)
        _dense_and_broadcast(agx, orc, dev, plan, tabs, n, bits, config * 131 + bits, (config, bits))
        plan.close()


@pytest.mark.parametrize("n,bits", [(32, 60), (4096, 60), (4096, 62), (16384, 30), (32768, 60)])
def test_radix2_plans_take_the_generic_path(agx, orc, dev, n, bits):
    plan, tabs = plan_from_oracle_tables(agx, orc, n, bits, 2)
    plan.set_variant(agx.VARIANT_LDS_RADIX2)
    _dense_and_broadcast(agx, orc, dev, plan, tabs, n, bits, n + bits, ("radix-2", n, bits))
    plan.close()


@pytest.mark.parametrize("n,bits", [(64, 60), (4096, 60), (4096, 30), (16384, 61)])
def test_aliasing_and_rejection(agx, orc, dev, n, bits):
    torch = dev.torch
    primes, batch = 2, 5
    plan, tabs = plan_from_oracle_tables(agx, orc, n, bits, primes)
    rng = np.random.default_rng(n + bits)
    a, b = _operands(rng, tabs, batch, n, bits)
    d_a, d_b = dev.to_device(a), dev.to_device(b)
    # one allocation for bhat and its neighbourhood: [ n words | bhat | room for a whole c behind any word of bhat ]
    d_room = dev.empty(2 * a.size + 2 * n)
    d_room.zero_()
    d_bhat = d_room[n:n + a.size]
    plan.forward(d_b.data_ptr(), d_bhat.data_ptr(), batch, dev.stream)
    d_c = dev.empty(a.size)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, stream=dev.stream)
    d_in = d_a.clone()
    plan.polymul_ntt(d_in.data_ptr(), d_bhat.data_ptr(), d_in.data_ptr(), batch, stream=dev.stream)      # c == a
    dev.sync()
    assert torch.equal(d_in, d_c), "in place differs from out of place"
    _assert_frames(dev.to_host(d_c), _oracle(orc, a, b, tabs, batch, n, frames=[0, batch - 1]), batch, n, "out of place")
    keep_room, keep_c = d_room.clone(), d_c.clone()
    P = plan.polymul_ntt
    st = dev.stream
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), d_bhat.data_ptr(), batch, batch, st) == 5           # c == bhat
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), d_bhat.data_ptr() + 8 * (n // 2), batch, batch, st) == 5      # c over bhat, n/2 later
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), d_bhat.data_ptr() - 8 * (n // 2), batch, batch, st) == 5      # ... n/2 earlier
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), d_bhat.data_ptr() + 8 * (primes * n - n // 2), batch, 1, st) == 5   # broadcast: bhat is primes * n words
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, 2, st) == 5                  # bhat_batch not in {1, batch}
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), d_a.data_ptr() + 8 * (n // 2), batch, batch, st) == 5   # c straddles a
    assert status_of(agx, P, 0, d_bhat.data_ptr(), d_c.data_ptr(), batch, batch, st) == 1
    assert status_of(agx, P, d_a.data_ptr(), 0, d_c.data_ptr(), batch, batch, st) == 1
    assert status_of(agx, P, d_a.data_ptr(), d_bhat.data_ptr(), 0, batch, batch, st) == 1
    fwd_only, _ = plan_from_oracle_tables(agx, orc, n, bits, primes, inverse=False)
    assert status_of(agx, fwd_only.polymul_ntt, d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), batch, batch, st) == 9
    fwd_only.close()
    P(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), 0, 0, st)      # empty batch: nothing happens, as agx_ntt_polymul
    P(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), 0, 1, st)
    dev.sync()
    assert torch.equal(d_room, keep_room) and torch.equal(d_c, keep_c), "a rejected call wrote memory"
    assert np.array_equal(dev.to_host(d_a), a)
    plan.close()


@pytest.mark.parametrize("n,primes,batch", [(4096, 4, 4096), (32768, 1, 1024)])
def test_bench_shapes_shift_property(agx, orc, dev, n, primes, batch):
    """the launch shapes the speed figures are taken at: a = X^j_f, so every frame of c must be b_f rotated negacyclically by j_f --
    checked on the device on every frame; dense, then broadcast with one b per prime"""
    torch = dev.torch
    plan = agx.Plan(n, agx.find_primes(60, n, primes))
    a = dev.empty(primes * batch * n)
    b, bhat, c = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    fill_monomials(torch, a, primes, batch, n)
    plan.fill_synthetic(b.data_ptr(), batch, 0, 7, dev.stream)
    plan.forward(b.data_ptr(), bhat.data_ptr(), batch, dev.stream)
    plan.polymul_ntt(a.data_ptr(), bhat.data_ptr(), c.data_ptr(), batch, batch, dev.stream)
    dev.sync()
    bad = check_negacyclic_shifts(torch, c, b, plan.moduli, batch, n)
    assert not bad, f"dense: X^j * b wrong at (prime, frames) {bad}"
    b1 = b.view(primes, batch, n)[:, 0].contiguous().view(-1)      # frame 0 of every prime
    bhat1 = torch.empty_like(b1)
    plan.forward(b1.data_ptr(), bhat1.data_ptr(), 1, dev.stream)
    c.zero_()
    plan.polymul_ntt(a.data_ptr(), bhat1.data_ptr(), c.data_ptr(), batch, 1, dev.stream)
    dev.sync()
    b.view(primes, batch, n)[:] = b1.view(primes, 1, n)
    bad = check_negacyclic_shifts(torch, c, b, plan.moduli, batch, n)
    assert not bad, f"broadcast: X^j * b wrong at (prime, frames) {bad}"
    # in place on the same shape
    plan.polymul_ntt(a.data_ptr(), bhat1.data_ptr(), a.data_ptr(), batch, 1, dev.stream)
    dev.sync()
    assert torch.equal(a, c), "in place differs from out of place"
    plan.close()


@pytest.mark.parametrize("n,bits,batch", [(32, 60, 100), (4096, 60, 9), (4096, 30, 9), (16384, 60, 300)])
def test_calls_are_graph_capturable(agx, orc, dev, n, bits, batch):
    """a dense and a broadcast call captured one after the other on a side stream (no parallel branches), replayed twice on new
    data: the same words as the eager calls"""
    torch = dev.torch
    primes = 2
    plan, tabs = plan_from_oracle_tables(agx, orc, n, bits, primes)
    rng = np.random.default_rng(n + batch)
    a, b = _operands(rng, tabs, batch, n, bits)
    d_a, d_b = dev.to_device(a), dev.to_device(b)
    d_bhat, d_bhat1 = dev.empty(a.size), dev.empty(primes * n)
    plan.forward(d_b.data_ptr(), d_bhat.data_ptr(), batch, dev.stream)
    b1 = np.concatenate([b[p * batch * n:p * batch * n + n] for p in range(primes)])
    d_b1 = dev.to_device(b1)
    plan.forward(d_b1.data_ptr(), d_bhat1.data_ptr(), 1, dev.stream)
    c_dense, c_bcast = dev.empty(a.size), dev.empty(a.size)

    def dense_then_broadcast(s):
        plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), c_dense.data_ptr(), batch, batch, s)
        plan.polymul_ntt(d_a.data_ptr(), d_bhat1.data_ptr(), c_bcast.data_ptr(), batch, 1, s)

    graph = capture(dev, lambda s: plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), c_dense.data_ptr(), batch, batch, s), dense_then_broadcast)
    e_dense, e_bcast = dev.empty(a.size), dev.empty(a.size)
    for _ in range(2):
        a, _unused = _operands(rng, tabs, batch, n, bits)
        d_a.copy_(torch.from_numpy(a.view(np.int64).copy()))
        c_dense.zero_()
        c_bcast.zero_()
        graph.replay()
        plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), e_dense.data_ptr(), batch, batch, dev.stream)
        plan.polymul_ntt(d_a.data_ptr(), d_bhat1.data_ptr(), e_bcast.data_ptr(), batch, 1, dev.stream)
        dev.sync()
        assert torch.equal(c_dense, e_dense) and torch.equal(c_bcast, e_bcast), "replay differs from the eager calls"
        _assert_frames(dev.to_host(c_dense), _oracle(orc, a, b, tabs, batch, n, frames=[0, batch - 1]), batch, n, "replayed dense")
    plan.close()


def test_group_equals_the_single_plan(agx, orc, dev):
    """DeviceGroup.polymul_ntt on devices [0, 0]: an odd frame count dealt to two shards, one dense and one broadcast, against
    Plan.polymul_ntt on the same words"""
    torch = dev.torch
    n, primes, frames = 4096, 2, 41
    moduli = moduli_for(orc.find_prime, n, [60] * primes)
    tabs = [oracle_tables(orc, n, q) for q in moduli]
    grp, plan, batches = group_of_two(agx, orc, n, moduli, frames)
    rng = np.random.default_rng(17)
    d_a, d_bhat, d_c, d_w, bb = [], [], [], [], []
    for i, bt in enumerate(batches):
        a, b = _operands(rng, tabs, bt, n, 60, b_batch=bt if i == 0 else 1)
        bb.append(bt if i == 0 else 1)
        d_a.append(dev.to_device(a))
        d_b = dev.to_device(b)
        d_bhat.append(dev.empty(b.size))
        plan.forward(d_b.data_ptr(), d_bhat[i].data_ptr(), bb[i], dev.stream)
        d_c.append(dev.empty(a.size))
        d_w.append(dev.empty(a.size))
        plan.polymul_ntt(d_a[i].data_ptr(), d_bhat[i].data_ptr(), d_w[i].data_ptr(), bt, bb[i], dev.stream)
    torch.cuda.synchronize()
    grp.polymul_ntt([d.data_ptr() for d in d_a], [d.data_ptr() for d in d_bhat], [d.data_ptr() for d in d_c], batches, bb)
    grp.synchronize()
    for i in range(2):
        assert torch.equal(d_c[i], d_w[i]), f"shard {i} differs from the single plan"
    # default bhat_batch (= batch) through the group: shard 1 again with a dense bhat
    d_t = d_bhat[1].view(primes, 1, n).expand(primes, batches[1], n).contiguous().view(-1)
    d_c[1].zero_()
    torch.cuda.synchronize()
    grp.polymul_ntt([d_a[0].data_ptr(), d_a[1].data_ptr()], [d_bhat[0].data_ptr(), d_t.data_ptr()], [d.data_ptr() for d in d_c], batches)
    grp.synchronize()
    assert torch.equal(d_c[1], d_w[1])
    grp.close()
    plan.close()
