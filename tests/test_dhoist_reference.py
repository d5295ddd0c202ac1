"""The reference of the double-hoisted linear transform alone, no device (tests/dhoist_ref.py on the CPU oracle): the weighted, accumulating inner product
followed by ONE ModDown.  Without a weight and an old acc it is rns_ref.apply_decomposed_ref word for word; a weight of ones is no weight; accumulating
rotation by rotation is the one big-integer sum; and with noise-free rotation keys the transformed ciphertext decrypts to sum_r w_r sigma_{g_r}(c s) within
p_count (1 + ||s||_1) whatever the weights are -- a condition, not a measurement -- where a ModDown per rotation does not."""
import numpy as np
import pytest

from dhoist_ref import accumulate_ref, linear_transform_ref, mod_down_pair_ref, rotation_keys, transform_deviation
from gpu_util import moduli_for, ntt_pi
from rns_cases import FIVE, FIVE_IDS
from rns_ref import active_of, apply_decomposed_ref, decompose_ref, digits_of, rotation_bound, spread

N, BATCH = 64, 2


def _case(orc, shape, seed):
    """(moduli, active, ext [digits][A][BATCH N], rng): the digits of a random chat"""
    moduli = moduli_for(orc.find_prime, N, [60] * 6)
    active = active_of(moduli, shape)
    rng = np.random.default_rng(seed)
    chat = np.stack([rng.integers(0, int(q), size=(BATCH, N), dtype=np.uint64) for q in active[:shape[0]]])
    return moduli, active, chat, decompose_ref(orc, N, moduli, shape, chat), rng


def _key(rng, active, shape):
    return np.stack([rng.integers(0, int(q), size=(len(digits_of(shape)), 2, N), dtype=np.uint64) for q in active], axis=2)      # [D][2][A][n]


def _weight(rng, active, frames):
    return np.stack([rng.integers(0, int(q), size=(frames, N), dtype=np.uint64) for q in active])      # [A][frames][n]


@pytest.mark.parametrize("g", [1, 5, 2 * N - 1])
@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_the_two_halves_are_apply_decomposed(orc, shape, g):
    moduli, active, _, ext, rng = _case(orc, shape, 11 + sum(shape))
    key = _key(rng, active, shape)
    acc = accumulate_ref(N, moduli, shape, ext, key, None, None, BATCH, g)
    want = apply_decomposed_ref(orc, N, moduli, shape, ext, key, BATCH, g)
    assert np.array_equal(mod_down_pair_ref(orc, N, moduli, shape, acc).reshape(want.shape), want)
    # lazy words of ext and the key are the same inputs
    lazy = accumulate_ref(N, moduli, shape, spread(rng, ext.reshape(len(ext), len(active), -1), active, axis=1), spread(rng, key, active, axis=2), None, None, BATCH, g)
    assert np.array_equal(lazy, acc)


@pytest.mark.parametrize("frames", [1, BATCH])
@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_a_weight_of_ones_is_no_weight(orc, shape, frames):
    moduli, active, _, ext, rng = _case(orc, shape, 23 + sum(shape))
    key = _key(rng, active, shape)
    old = _weight(rng, active, 2 * BATCH).reshape(len(active), 2, -1).swapaxes(0, 1)      # [2][A][BATCH N]
    ones = np.ones((len(active), frames, N), dtype=np.uint64)
    for acc_old in (None, old):
        assert np.array_equal(accumulate_ref(N, moduli, shape, ext, key, ones, acc_old, BATCH, 5), accumulate_ref(N, moduli, shape, ext, key, None, acc_old, BATCH, 5))
    assert not np.array_equal(accumulate_ref(N, moduli, shape, ext, key, None, old, BATCH, 5), accumulate_ref(N, moduli, shape, ext, key, None, None, BATCH, 5))


@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_accumulating_one_by_one_is_the_one_sum(orc, shape):
    """R = 3 rotations accumulated call by call (the old acc spread over [0, 4q) in between) against sum_r w_r (sum_d ext_d[pi_r] key_{r,d,o}) formed in
    Python integers without any reduction before the last"""
    moduli, active, _, ext, rng = _case(orc, shape, 37 + sum(shape))
    A, D = len(active), len(digits_of(shape))
    rotations = [(g, _key(rng, active, shape), _weight(rng, active, frames)) for g, frames in ((5, 1), (2 * N - 1, BATCH), (1, 1))]
    acc = None
    for g, key, w in rotations:
        acc = accumulate_ref(N, moduli, shape, ext, key, w, None if acc is None else spread(rng, acc, active, axis=1), BATCH, g)
    e = ext.reshape(D, A, BATCH, N)
    for o in range(2):
        for j, q in enumerate(active):
            total = np.zeros((BATCH, N), dtype=object)
            for g, key, w in rotations:
                t = np.zeros((BATCH, N), dtype=object)
                for d in range(D):
                    t = t + e[d, j][:, ntt_pi(N, g)].astype(object) * key[d, o, j].astype(object)
                total = total + t * w[j].astype(object)
            assert np.array_equal(acc[o, j], (total % int(q)).astype(np.uint64).reshape(-1)), (shape, o, j)


@pytest.mark.parametrize("shape", FIVE, ids=FIVE_IDS)
def test_one_mod_down_leaves_noise_independent_of_the_weights(orc, shape):
    """out_0 + out_1 s - sum_r w_r sigma_{g_r}(c) sigma_{g_r}(s), CRT-centred modulo Q, is at most p_count (1 + ||s||_1) for R = 3 rotation keys that share
    one s and full-size random weights (any residue tuple is one element of R_QP): sum_r w_r acc_r = P M (mod QP) exactly, and the lifts V_o of its special
    slabs satisfy V_0 + V_1 s = 0 (mod P) with coefficients below p_count P (1 + ||s||_1).  The single-hoisted composition sum_r w_r o ModDown(acc_r)
    multiplies what each ModDown leaves by a full-size weight, and exceeds the bound"""
    elements = (5, 2 * N - 1, 25)
    moduli, active, chat, ext, rng = _case(orc, shape, 51 + sum(shape))
    s, shat, keys = rotation_keys(orc, N, moduli, shape, elements, 2000 + sum(shape))
    rotations = [(g, keys[g], _weight(rng, active, 1)) for g in elements]
    bound = rotation_bound(shape, s)
    out = linear_transform_ref(orc, N, moduli, shape, ext, rotations, BATCH)
    worst = transform_deviation(orc, N, moduli, shape, BATCH, chat, shat, out, rotations)
    print(f"shape {shape}: double-hoisted worst deviation {worst}, bound {bound}")
    assert worst <= bound, (shape, worst, bound)
    # one rotation with one weight holds the bound too: it does not grow with R
    single = linear_transform_ref(orc, N, moduli, shape, ext, rotations[:1], BATCH)
    assert transform_deviation(orc, N, moduli, shape, BATCH, chat, shat, single, rotations[:1]) <= bound
    # a ModDown per rotation, then the weights
    q_count, Q = shape[0], active[:shape[0]]
    summed = np.zeros((2, q_count, BATCH, N), dtype=object)
    for g, key, w in rotations:
        part = mod_down_pair_ref(orc, N, moduli, shape, accumulate_ref(N, moduli, shape, ext, key, None, None, BATCH, g)).reshape(2, q_count, BATCH, N)
        summed = summed + part.astype(object) * w[:q_count].astype(object)[None]
    summed = np.stack([np.stack([(summed[o, j] % int(q)).astype(np.uint64) for j, q in enumerate(Q)]) for o in range(2)])
    apart = transform_deviation(orc, N, moduli, shape, BATCH, chat, shat, summed, rotations)
    print(f"shape {shape}: single-hoisted worst deviation {apart}")
    assert apart > bound, (shape, apart, bound)
