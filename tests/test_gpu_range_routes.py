"""agx_ntt_forward_range and agx_ntt_inverse_range on every route a plan can take: each product registry entry at its own size on ranges that start
behind prime 0, the forward companions of n = 4096 (ids 165 and 159) on both sides of the frame count where the plan switches to them, the companion of
n = 16384 (id 164), and the ticket-drawing loop inverse of n = 16384 / 32768 on more frames than its resident grid holds, eagerly and replayed from a graph
(its stateless fixed-stride form).  These are the launches every RNS call since the key switch is built from (prime_range, csrc/rb_registry.hpp).

The reference is the CPU oracle on the range's moduli; the second witness is a plan created over just those primes with the same roots, which has the
same tables and so must write the same words.  Small launches are judged on every word by both; large ones on every word against the second witness on
the device, and on gpu_util.judged_frames by the oracle.  Every comparison is word for word, and every case asserts that it reached the route it names."""
import numpy as np
import pytest

from gpu_util import (PRODUCT_IDS, Q60C_REGISTRY, REGISTRY, canary, capture, companion_batches, judged_frames, loop_batch, moduli_for, oracle_tables,
                      radix2_twin, rand_coeffs, resident_grid, select_entry)
from modulus_cases import edge_moduli
from q60c_skip_cases import SKIP_MAX_C, prime_above_c
from rns_cases import device_words
from rns_ref import oracle_forward_set, oracle_inverse_set

pytestmark = pytest.mark.gpu

TAIL = 64      # canary words kept behind every output
MAIN_4096, COMPANION_Q60C, COMPANION_GENERAL = 93, 165, 159
COMPANION_16384 = 164
# what forward_kernel reports for the default 60-bit plans whose inverse is the loop kernel's (main entries 117 / 119)
LOOP_PLAN_FORWARD = {16384: COMPANION_16384, 32768: 119}


def _plan(agx, orc, n, moduli):
    """a plan over `moduli` with the oracle's (least) roots: two such plans have the same tables for the primes they share, and psi() reports the root"""
    return agx.Plan(n, list(moduli), psi=[oracle_tables(orc, n, q)[1] for q in moduli])


def _hi(bits):
    """inputs anywhere in [0, 4q); [0, 3q) above 2^61"""
    return 4 if bits < 62 else 3


def _reduced(x, moduli):
    return x % np.array(moduli, dtype=np.uint64)[:, None]


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


# ---- every product registry entry at its own size ------------------------------------------------------------------------------------------
ENTRIES = [e for e in REGISTRY if e[0] in PRODUCT_IDS] + Q60C_REGISTRY


def _select(agx, plan, config):
    """select_entry for the entries of REGISTRY; id 165 stands apart from it (and from PRODUCT_IDS) and is a product entry: named directly"""
    if config in [e[0] for e in Q60C_REGISTRY]:
        plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    else:
        select_entry(agx, plan, config)


def _check_ranges(agx, orc, dev, config, n, bits, batch):
    """forward and inverse on the ranges (1, 2), (P - 1, 1) and (0, P) of a plan with the entry selected: out of place into a buffer with canary words
    behind it (the input unchanged), and in place, against the oracle on the range's moduli and against a plan over just those primes"""
    P = 4 if n < 16384 else 3
    moduli = moduli_for(orc.find_prime, n, [bits] * P)
    plan = _plan(agx, orc, n, moduli)
    _select(agx, plan, config)
    assert plan.forward_kernel(batch) == config, (config, bits, plan.forward_kernel(batch))
    rng = np.random.default_rng(config * 131 + bits + batch)
    x = np.stack([rand_coeffs(rng, batch * n, q, hi_mult=_hi(bits)) for q in moduli])
    want = {"forward": oracle_forward_set(orc, n, moduli, _reduced(x, moduli)), "inverse": oracle_inverse_set(orc, n, moduli, x)}
    st = dev.stream
    for first, count in ((1, 2), (P - 1, 1), (0, P)):
        sub = None
        if count < P:
            sub = _plan(agx, orc, n, moduli[first:first + count])
            _select(agx, sub, config)
            assert sub.forward_kernel(batch) == config and all(sub.psi(k) == plan.psi(first + k) for k in range(count))
        x_r = x[first:first + count].reshape(-1)
        for name in ("forward", "inverse"):
            what = (config, bits, batch, name, first, count)
            w = want[name][first:first + count].reshape(-1)
            d_in, d_out = dev.to_device(x_r), dev.to_device(canary(0, x_r.size + TAIL))
            getattr(plan, name + "_range")(d_in.data_ptr(), d_out.data_ptr(), batch, first, count, st)
            got = dev.to_host(d_out)
            assert np.array_equal(got[:x_r.size], w), (what, "out of place against the oracle", _first_bad(got[:x_r.size], w))
            assert np.array_equal(got[x_r.size:], canary(x_r.size, TAIL)), (what, "a word behind the output changed")
            assert np.array_equal(dev.to_host(d_in), x_r), (what, "the input changed")
            d_wit = dev.to_device(x_r)      # the second witness: a plan over those primes; for the whole range, the whole-plan call
            getattr(plan if sub is None else sub, name)(d_wit.data_ptr(), d_wit.data_ptr(), batch, st)
            assert np.array_equal(dev.to_host(d_wit), w), (what, "the plan over those primes against the oracle")
            getattr(plan, name + "_range")(d_in.data_ptr(), d_in.data_ptr(), batch, first, count, st)
            got = dev.to_host(d_in)
            assert np.array_equal(got, w), (what, "in place against the oracle", _first_bad(got, w))
        if sub is not None:
            sub.close()
    plan.close()


@pytest.mark.parametrize("config,n,max_bits", ENTRIES)
def test_every_registry_entry_on_ranges_that_start_behind_prime_0(agx, orc, dev, config, n, max_bits):
    """each product entry selected explicitly (AGX_VARIANT_REGBLOCK_BASE + id) at the size it serves, under the widest modulus it admits and under a
    30-bit one where it admits that (id 165 admits 2^60 - c alone); a plan of 4 primes (3 from n = 16384 on), batch 3, and below n = 1024 also batch 67:
    a wave is partly filled there and frames of two primes meet in one wave"""
    widths = (max_bits,) if (config, n, max_bits) in Q60C_REGISTRY else tuple(dict.fromkeys((max_bits, 30)))
    for bits in widths:
        for batch in (3, 67) if n < 1024 else (3,):
            _check_ranges(agx, orc, dev, config, n, bits, batch)


# ---- the forward companions of n = 4096 on a range ---------------------------------------------------------------------------------------------
def _companion_moduli(agx, orc, which):
    n = 4096
    six = list(agx.find_primes(60, n, 6))
    assert all(0 < (1 << 60) - q <= SKIP_MAX_C for q in six)
    if which == "skip":
        return tuple(six), COMPANION_Q60C
    if which == "general":      # one c above the skip form's limit, inside the class: id 165's kernel with the subtract on every stage
        q_out, c_out = prime_above_c(orc, SKIP_MAX_C)
        assert SKIP_MAX_C < c_out < 1 << 28 and q_out not in six
        return tuple(six[:2] + [q_out] + six[2:5]), COMPANION_Q60C
    q = edge_moduli(orc, n)["c_out"]      # the prime next to the class 2^60 - c, outside it: the plan gets the general companion
    assert (1 << 60) - q > 1 << 28 and q not in six
    return tuple(six[:4] + [q] + six[4:5]), COMPANION_GENERAL


@pytest.mark.parametrize("which", ["skip", "general", "c_out"])
def test_forward_companion_of_4096_on_a_range(agx, orc, dev, which):
    """six primes; b_hi the smallest batch the companion serves (6 b_hi frames just at or above its threshold), b_lo = b_hi - 1 the largest the main
    entry serves.  At both, forward_range on (1, 3) and (4, 2) must equal, on every word, the forward of a plan over those primes -- which stays below its
    own threshold and runs the main kernel: an independent shape -- and the oracle on the first, last and boundary frames; in place as out of place"""
    torch = dev.torch
    n, st = 4096, dev.stream
    moduli, companion = _companion_moduli(agx, orc, which)
    P = len(moduli)
    plan = _plan(agx, orc, n, moduli)
    b_lo, b_hi = companion_batches(plan, MAIN_4096, companion)
    assert plan.forward_kernel(b_hi) == companion and plan.forward_kernel(b_lo) == MAIN_4096 and P == 6
    for first, count in ((1, 3), (4, 2)):
        sub_moduli = moduli[first:first + count]
        sub = _plan(agx, orc, n, sub_moduli)
        assert all(sub.psi(k) == plan.psi(first + k) for k in range(count))
        for batch in (b_hi, b_lo):
            what = (which, first, count, batch)
            assert sub.forward_kernel(batch) == MAIN_4096, (what, "the plan over the range must stay on the main kernel")
            words = count * batch * n
            d_x = torch.cat([device_words(torch, dev, batch * n, q, first * 100 + p) for p, q in enumerate(sub_moduli)])
            d_keep = d_x.clone()
            d_out, d_wit = dev.to_device(canary(0, words + TAIL)), dev.empty(words)
            plan.forward_range(d_x.data_ptr(), d_out.data_ptr(), batch, first, count, st)
            sub.forward(d_x.data_ptr(), d_wit.data_ptr(), batch, st)
            dev.sync()
            assert torch.equal(d_out[:words], d_wit), (what, "out of place: differs from the plan over those primes")
            assert np.array_equal(dev.to_host(d_out[words:]), canary(words, TAIL)), (what, "a word behind the output changed")
            assert torch.equal(d_x, d_keep), (what, "the input changed")
            plan.forward_range(d_x.data_ptr(), d_x.data_ptr(), batch, first, count, st)
            dev.sync()
            assert torch.equal(d_x, d_wit), (what, "in place: differs from the plan over those primes")
            frames = judged_frames(batch, 12)
            idx = torch.tensor(frames, device=dev.device)
            got = dev.to_host(d_x.view(count, batch, n)[:, idx].contiguous()).reshape(count, -1)
            x_h = dev.to_host(d_keep.view(count, batch, n)[:, idx].contiguous()).reshape(count, -1)
            want = oracle_forward_set(orc, n, sub_moduli, _reduced(x_h, sub_moduli))
            bad = [(p, frames[f]) for p in range(count) for f in range(len(frames)) if not np.array_equal(got[p, f * n:(f + 1) * n], want[p, f * n:(f + 1) * n])]
            assert not bad, (what, "(prime of the range, frame) differ from the oracle", bad[:8])
        sub.close()
    plan.close()


# ---- n = 16384 and 32768 -----------------------------------------------------------------------------------------------------------------
def test_forward_companion_of_16384_on_a_range(agx, orc, dev):
    """three 60-bit primes, batch 3: id 164 serves every forward launch of such a plan; ranges (1, 2) and (2, 1) against the oracle on every word, the
    plan over those primes and the radix-2 twin of that plan (an independent kernel family)"""
    n, batch, st = 16384, 3, dev.stream
    moduli = moduli_for(orc.find_prime, n, [60] * 3)
    plan = _plan(agx, orc, n, moduli)
    assert plan.forward_kernel(batch) == COMPANION_16384
    rng = np.random.default_rng(164)
    x = np.stack([rand_coeffs(rng, batch * n, q, hi_mult=4) for q in moduli])
    want = oracle_forward_set(orc, n, moduli, _reduced(x, moduli))
    for first, count in ((1, 2), (2, 1)):
        x_r, w = x[first:first + count].reshape(-1), want[first:first + count].reshape(-1)
        d_in, d_out = dev.to_device(x_r), dev.to_device(canary(0, x_r.size + TAIL))
        plan.forward_range(d_in.data_ptr(), d_out.data_ptr(), batch, first, count, st)
        got = dev.to_host(d_out)
        assert np.array_equal(got[:x_r.size], w), (first, count, "out of place against the oracle", _first_bad(got[:x_r.size], w))
        assert np.array_equal(got[x_r.size:], canary(x_r.size, TAIL)) and np.array_equal(dev.to_host(d_in), x_r), (first, count)
        plan.forward_range(d_in.data_ptr(), d_in.data_ptr(), batch, first, count, st)
        assert np.array_equal(dev.to_host(d_in), w), (first, count, "in place against the oracle")
        sub = _plan(agx, orc, n, moduli[first:first + count])
        twin = radix2_twin(agx, sub)
        assert sub.forward_kernel(batch) == COMPANION_16384 and twin.forward_kernel(batch) == -1
        for other in (sub, twin):
            d_wit = dev.to_device(x_r)
            other.forward(d_wit.data_ptr(), d_wit.data_ptr(), batch, st)
            assert np.array_equal(dev.to_host(d_wit), w), (first, count, "a plan over those primes against the oracle")
        twin.close(), sub.close()
    plan.close()


def _loop_case(agx, orc, dev, n, P, first, count):
    """(plan, sub, twin, batch, d_x, d_want): a plan of P 60-bit primes and the plan over its range with that plan's radix-2 twin; lazy NTT-form words of
    the range on more frames per prime than the loop inverse's resident grid, a ragged last round; the twin's inverse of them"""
    torch = dev.torch
    moduli = moduli_for(orc.find_prime, n, [60] * P)
    plan = _plan(agx, orc, n, moduli)
    sub = _plan(agx, orc, n, moduli[first:first + count])
    twin = radix2_twin(agx, sub)
    assert plan.forward_kernel(1) == LOOP_PLAN_FORWARD[n] == sub.forward_kernel(1), "both plans must be on their registry entries"
    assert twin.forward_kernel(1) == -1, "the twin must be on the generic route"
    batch, resident = loop_batch(torch, n), resident_grid(torch, n)
    assert batch > resident and batch % resident != 0 and (count * batch) % resident != 0, (batch, resident)
    d_x = torch.cat([device_words(torch, dev, batch * n, q, n + p) for p, q in enumerate(moduli[first:first + count])])
    d_want = dev.empty(d_x.numel())
    twin.inverse(d_x.data_ptr(), d_want.data_ptr(), batch, dev.stream)
    dev.sync()
    return plan, sub, twin, batch, d_x, d_want


def _judge_inverse(orc, dev, d_x, d_got, moduli, batch, n, resident, what):
    """the first, last and boundary frames, both sides of the resident grid among them, against the oracle"""
    torch = dev.torch
    frames = sorted(set(judged_frames(batch, 10)) | {resident - 1, resident})
    idx = torch.tensor(frames, device=dev.device)
    count = len(moduli)
    got = dev.to_host(d_got.view(count, batch, n)[:, idx].contiguous()).reshape(count, -1)
    want = oracle_inverse_set(orc, n, moduli, dev.to_host(d_x.view(count, batch, n)[:, idx].contiguous()).reshape(count, -1))
    bad = [(p, frames[f]) for p in range(count) for f in range(len(frames)) if not np.array_equal(got[p, f * n:(f + 1) * n], want[p, f * n:(f + 1) * n])]
    assert not bad, (what, "(prime of the range, frame) differ from the oracle", bad[:8])


@pytest.mark.parametrize("n,P,first,count", [(16384, 3, 1, 2), (32768, 2, 1, 1)])
def test_loop_inverse_on_a_range_past_its_resident_grid(agx, orc, dev, n, P, first, count):
    """inverse_range out of place and in place: every word equals the inverse of the plan over those primes and of its radix-2 twin (the generic
    route, an independent kernel family); the oracle on the edge frames"""
    torch = dev.torch
    plan, sub, twin, batch, d_x, d_want = _loop_case(agx, orc, dev, n, P, first, count)
    words, st = d_x.numel(), dev.stream
    d_keep = d_x.clone()
    d_out, d_wit = dev.to_device(canary(0, words + TAIL)), dev.empty(words)
    plan.inverse_range(d_x.data_ptr(), d_out.data_ptr(), batch, first, count, st)
    sub.inverse(d_x.data_ptr(), d_wit.data_ptr(), batch, st)
    dev.sync()
    assert torch.equal(d_wit, d_want), "the plan over those primes differs from its radix-2 twin"
    assert torch.equal(d_out[:words], d_want), "out of place: differs from the radix-2 twin of the plan over those primes"
    assert np.array_equal(dev.to_host(d_out[words:]), canary(words, TAIL)), "a word behind the output changed"
    assert torch.equal(d_x, d_keep), "the input changed"
    _judge_inverse(orc, dev, d_keep, d_out[:words], sub.moduli, batch, n, resident_grid(torch, n), (n, first, count))
    plan.inverse_range(d_x.data_ptr(), d_x.data_ptr(), batch, first, count, st)
    dev.sync()
    assert torch.equal(d_x, d_want), "in place: differs from the radix-2 twin of the plan over those primes"
    for h in (twin, sub, plan):
        h.close()


def test_loop_inverse_on_a_range_in_a_graph(agx, orc, dev):
    """n = 16384, range (1, 2), captured: the loop inverse takes its stateless fixed-stride form.  Capturing must launch nothing (the output keeps its
    fill), the replay must write the eager call's words"""
    torch = dev.torch
    n, first, count = 16384, 1, 2
    plan, sub, twin, batch, d_x, d_want = _loop_case(agx, orc, dev, n, 3, first, count)
    words = d_x.numel()
    d_eager, d_warm, d_out = dev.empty(words), dev.empty(words), dev.empty(words)
    plan.inverse_range(d_x.data_ptr(), d_eager.data_ptr(), batch, first, count, dev.stream)
    dev.sync()
    assert torch.equal(d_eager, d_want), "the eager call differs from the radix-2 twin of the plan over those primes"
    d_out.fill_(-1)
    graph = capture(dev, lambda s: plan.inverse_range(d_x.data_ptr(), d_warm.data_ptr(), batch, first, count, s),      # warm-up into a buffer of its own
                    lambda s: plan.inverse_range(d_x.data_ptr(), d_out.data_ptr(), batch, first, count, s))
    dev.sync()
    assert bool((d_out == -1).all()), "the capture itself wrote the output"
    assert torch.equal(d_warm, d_eager), "the warm-up call on the side stream differs from the eager call"
    graph.replay()
    dev.sync()
    assert torch.equal(d_out, d_eager), "the replay differs from the eager call"
    for h in (twin, sub, plan):
        h.close()
