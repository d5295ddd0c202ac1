"""Self-test of the whole-buffer checkers of gpu_util.py that test_gpu_ops_at_scale.py relies on (and of the chunked comparison of the RNS calls' tests
at scale), on the CPU: the output of the GPU is
replaced by the oracle's, once untouched and once per planted fault; every checker must pass the first and name a word of the second.
The expected words of the rescale identity are compared with Python integers (X by CRT, Y = floor((X + {0, h}) / q_L)), the reference
of test_gpu_rescale.py."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import (assert_equals_chunked_calls, check_automorphism_coeff, check_automorphism_ntt, check_fixed_shifts, check_rescale_identity, fill_rescale_constants,
                      moduli_for, ntt_pi, oracle_polymul, rand_coeffs, rescale_identity_constants, rescale_identity_sum_, rescale_reference, sigma,
                      spread_lazy_, thin_frames)

CPU = torch.device("cpu")
FLOOR, ROUND = 0, 1
N, BATCH, TRIP = 64, 9, 256      # a "grid-stride trip" of 256 words: frames 0 .. 3 are the first trip, frames 4 .. 7 the second


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy())


# ---- the rescale identity against Python integers -------------------------------------------------------------------------------
def _identity_inputs(orc, rng, moduli, count):
    """(y [P][count] with the boundary remainders planted in the last slab, the residues x of X = Y q_L + r built as the GPU test builds
    them: the product y o C through the oracle's pointwise in place of the plan's, the sum with rescale_identity_sum_)"""
    P, qL = len(moduli), moduli[-1]
    h = (qL - 1) // 2
    y = np.stack([rand_coeffs(rng, count, q) for q in moduli])
    special = np.array([0, 1, h - 1, h, h + 1, qL - 1], dtype=np.uint64)
    y[P - 1, :special.size] = special
    y[P - 1, -special.size:] = special[::-1]
    c = fill_rescale_constants(torch, torch.empty(P * count, dtype=torch.int64), moduli).numpy().view(np.uint64).reshape(P, count)
    prod = np.stack([orc.pointwise(y[p], c[p], q) for p, q in enumerate(moduli)])
    x = rescale_identity_sum_(torch, _t(prod.reshape(-1)), _t(y.reshape(-1)), moduli)
    return y, x.numpy().view(np.uint64).reshape(P, count)


@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("spec", [(60, 60, 60), (60, 30, 61), (30, 30, 30), (62, 62), (30, 30), (61, 60, 30), (62, 62, 62)], ids=str)
def test_identity_words_equal_the_python_integer_reference(orc, n, spec):
    moduli = list(moduli_for(orc.find_prime, n, spec))
    batch = 5
    rng = np.random.default_rng(n + sum(spec))
    y, x = _identity_inputs(orc, rng, moduli, batch * n)
    qL = moduli[-1]
    assert rescale_identity_constants(moduli) == [qL % q for q in moduli[:-1]] + [0]
    assert all(int(x[p].max()) < q for p, q in enumerate(moduli)) and np.array_equal(x[-1], y[-1])
    # X rebuilt from x alone, one Python integer per coefficient
    Q = int(np.prod([int(q) for q in moduli], dtype=object))
    X = [0] * (batch * n)
    for p, q in enumerate(moduli):
        w = (Q // q) * pow(Q // q, -1, q)
        X = [(v + int(r) * w) % Q for v, r in zip(X, x[p].tolist())]
    for mode in (FLOOR, ROUND):
        h = (qL - 1) // 2 if mode == ROUND else 0
        Y = [(v + h) // qL for v in X]
        ref = np.stack([np.array([v % q for v in Y], dtype=np.uint64) for q in moduli[:-1]])
        assert np.array_equal(rescale_reference(x, moduli, mode), ref), "rescale_reference differs from the plain loop"
        assert check_rescale_identity(torch, _t(ref.reshape(-1)), _t(y.reshape(-1)), moduli, batch, n, mode, CPU) == [], (spec, mode)
        if mode == FLOOR:
            assert np.array_equal(ref, y[:-1]), "floor must give back Y"
    # the round bit is taken somewhere and left somewhere, so both branches of the identity were compared
    up = y[-1] > np.uint64((qL - 1) // 2)
    assert up.any() and not up.all()


def test_rescale_reference_on_drawn_integers(orc):
    """X drawn as Python integers, its residues handed over: the CRT inside rescale_reference must find the same X"""
    n = 64
    for spec in [(60, 60, 60), (60, 30, 61), (62, 62)]:
        moduli = list(moduli_for(orc.find_prime, n, spec))
        Q = int(np.prod([int(q) for q in moduli], dtype=object))
        qL = moduli[-1]
        h = (qL - 1) // 2
        rng = np.random.default_rng(len(spec))
        limbs = rng.integers(0, 1 << 63, size=(200, 4), dtype=np.uint64).tolist()
        X = [(((a << 63 | b) << 63 | c) << 63 | d) % Q for a, b, c, d in limbs] + [0, Q - 1, qL - 1, qL, h, h + 1, Q - h - 1, Q - h - 2]
        res = np.stack([np.array([v % q for v in X], dtype=np.uint64) for q in moduli])
        for mode in (FLOOR, ROUND):
            want = np.stack([np.array([((v + (h if mode else 0)) // qL) % q for v in X], dtype=np.uint64) for q in moduli[:-1]])
            assert np.array_equal(rescale_reference(res, moduli, mode), want), (spec, mode)


# ---- planted faults ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(orc, kind):
    """(the oracle's output [primes][BATCH][N] for `kind`, a function judging such an output with the checker of that kind)"""
    spec = (60, 30, 61) if kind != "rescale_round" and kind != "rescale_floor" else (60, 60, 61)
    moduli = list(moduli_for(orc.find_prime, N, spec))
    P = len(moduli)
    rng = np.random.default_rng(len(kind))
    tabs = [(q, orc.min_root(q, N)) for q in moduli]
    fwd = lambda p, v: orc.forward(np.ascontiguousarray(v), moduli[p], *orc.make_tables(*tabs[p], N), N)      # noqa: E731
    a = np.stack([rand_coeffs(rng, BATCH * N, q) for q in moduli])
    lazy = spread_lazy_(torch, _t(a.reshape(-1)), moduli, 5)
    if kind == "ntt":
        g = 5
        ahat = _t(np.concatenate([fwd(p, a[p]) for p in range(P)]))
        out = np.stack([fwd(p, sigma(a[p], g, N, moduli[p])) for p in range(P)])
        assert np.array_equal(out.reshape(-1, N), ahat.numpy().view(np.uint64).reshape(-1, N)[:, ntt_pi(N, g)])
        judge = lambda got: check_automorphism_ntt(torch, got, ahat, BATCH, N, g, CPU)      # noqa: E731
    elif kind == "coeff":
        g = 2 * N - 1
        out = np.stack([sigma(lazy.numpy().view(np.uint64).reshape(P, -1)[p], g, N, moduli[p]) for p in range(P)])
        judge = lambda got: check_automorphism_coeff(torch, got, lazy, moduli, BATCH, N, g, CPU)      # noqa: E731
    elif kind in ("rescale_floor", "rescale_round"):
        mode = ROUND if kind == "rescale_round" else FLOOR
        y, x = _identity_inputs(orc, rng, moduli, BATCH * N)
        out = rescale_reference(x, moduli, mode)
        yt = _t(y.reshape(-1))
        judge = lambda got: check_rescale_identity(torch, got, yt, moduli, BATCH, N, mode, CPU)      # noqa: E731
    else:
        shifts = [3, N - 1, 17]
        lz = lazy.numpy().view(np.uint64).reshape(P, BATCH, N)
        mono = np.zeros((P, N), dtype=np.uint64)
        mono[np.arange(P), shifts] = 1
        out = np.stack([np.stack([oracle_polymul(orc, lz[p, f], mono[p], *tabs[p], N) for f in range(BATCH)]) for p in range(P)])
        judge = lambda got: check_fixed_shifts(torch, got, lazy, moduli, BATCH, N, shifts, CPU)      # noqa: E731
        if kind == "shift_frame1":      # what a broadcast with a poly stride of n reads for frame 1 of prime 0: prime 1's operand
            out[0, 1] = oracle_polymul(orc, lz[0, 1], mono[1], *tabs[0], N)
    out = out.reshape(-1, BATCH, N)
    out.setflags(write=False)
    return out, judge


KINDS = ["ntt", "coeff", "rescale_floor", "rescale_round", "shift"]


@pytest.mark.parametrize("kind", KINDS)
def test_checkers_pass_the_oracles_output(orc, kind):
    out, judge = _case(orc, kind)
    assert judge(_t(out.reshape(-1))) == []


def _wrong_word(out):
    out[-1, -1, N - 1] ^= np.uint64(1)
    return (out.shape[0] - 1, BATCH - 1, N - 1)


def _swapped(out):
    out[0, [2, 3]] = out[0, [3, 2]]
    return (0, 2, None)


def _second_trip_unwritten(out):
    """every prime's words TRIP .. 2 TRIP - 1 keep what the buffer held before the call"""
    out.reshape(out.shape[0], -1)[:, TRIP:2 * TRIP] = np.uint64((1 << 64) - 1)
    return (0, TRIP // N, 0)


FAULTS = [_wrong_word, _swapped, _second_trip_unwritten]


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__.strip("_") for f in FAULTS])
@pytest.mark.parametrize("kind", KINDS)
def test_checkers_name_every_planted_fault(orc, kind, fault):
    out, judge = _case(orc, kind)
    bad = out.copy()
    prime, frame, element = fault(bad)
    assert not np.array_equal(bad, out), "the planted fault changed nothing"
    found = judge(_t(bad.reshape(-1)))
    assert found, f"{kind}: {fault.__name__} not noticed"
    assert found[0][:2] == (prime, frame) and (element is None or found[0][2] == element), (kind, fault.__name__, found)
    assert len(found) <= 4


def test_shift_checker_catches_a_broadcast_that_took_frame_1s_operand(orc):
    out, judge = _case(orc, "shift_frame1")
    found = judge(_t(out.reshape(-1)))
    assert found and all(f[:2] == (0, 1) for f in found), found


def test_one_dimensional_second_trip_of_the_ntt_form(orc):
    """the NTT-form kernels number the words of all primes together: the second trip lies wherever TRIP falls, prime boundaries or not"""
    out, judge = _case(orc, "ntt")
    bad = out.copy()
    flat = bad.reshape(-1)
    lo = (BATCH * N // TRIP + 1) * TRIP      # the first trip boundary inside prime 1
    flat[lo:lo + TRIP] = flat[lo - TRIP:lo]
    found = judge(_t(flat))
    assert found and found[0] == (lo // (BATCH * N), (lo // N) % BATCH, 0), found


# ---- the chunked comparison of the RNS calls ----------------------------------------------------------------------------------------------------
def _fake_call(ins, outs, frames):
    """a stand-in for an RNS call of two inputs ([2][frames][N], [1][frames][N]) and two outputs: every output word depends on its own frame alone"""
    assert ins[0].shape == (2, frames, N) and ins[1].shape == (1, frames, N) and all(bool((o == -1).all()) for o in outs)
    outs[0][:] = ins[0] * 3 + ins[1]
    outs[1][:] = ins[0][:1] - ins[1].flip(2)
    ins[0].zero_()      # a call may consume its operands: the helper hands out copies


@pytest.mark.parametrize("chunk", [2, 4, 9, 16])
@pytest.mark.parametrize("fault", ["none", "dropped", "shifted", "one word of the last frame"])
def test_chunked_comparison_fails_when_the_second_trip_is_dropped_or_shifted(fault, chunk):
    """the large call's outputs are the fake call's own, with frames 4 .. 7 of every slab -- the second "trip" -- left unwritten, or written one frame late"""
    g = torch.Generator().manual_seed(7)
    inputs = [torch.randint(0, 1 << 60, (s, BATCH, N), generator=g, dtype=torch.int64) for s in (2, 1)]
    keep = [v.clone() for v in inputs]
    outputs = [torch.full((s, BATCH, N), -1, dtype=torch.int64) for s in (2, 1)]
    _fake_call([v.clone() for v in inputs], outputs, BATCH)
    first, last = TRIP // N, 2 * TRIP // N
    if fault == "dropped":
        outputs[1][:, first:last] = -1
    elif fault == "shifted":
        outputs[0][:, first + 1:last + 1] = outputs[0][:, first:last].clone()
    elif fault != "none":
        outputs[0][-1, -1, N - 1] ^= 1
    if fault == "none":
        assert_equals_chunked_calls(torch, _fake_call, inputs, outputs, BATCH, chunk)
    else:
        with pytest.raises(AssertionError, match="differs from the call on frames"):
            assert_equals_chunked_calls(torch, _fake_call, inputs, outputs, BATCH, chunk)
    assert all(torch.equal(a, b) for a, b in zip(inputs, keep)), "the helper let the call consume the inputs themselves"


def test_thin_frames_keeps_what_it_must():
    frames = list(range(0, 700, 7)) + [1, 511, 512, 697, 699]
    keep = [0, 1, 697, 699, 511, 512]
    got = thin_frames(frames, keep, 16)
    assert len(got) == 16 and set(keep) <= set(got) and set(got) <= set(frames) and got == sorted(got)
    assert thin_frames([3, 1, 2], [2], 16) == [1, 2, 3]
