"""The skip form of the two-twiddle butterfly for q = 2^60 - c, c <= 2^27 (csrc/modarith.hpp: reduction by the top four bits on the even stages only,
lazy-range constant 7q), as an integer model of the whole n = 4096 forward transform in Python integers (tests/q60c_skip_cases.py).  No GPU.

The model asserts at every butterfly that hi, every partial sum of the chain, x' and y' stay inside [0, 2^64), and its fully reduced outputs are compared
with the oracle's forward.  The oracle takes inputs below 4q; the transform is linear over Z_q, so for frames of arbitrary 64-bit words (which the kernel's
first stage accepts) the oracle transforms the words reduced modulo q.

That the assertions can fail is shown on the butterfly itself: with every operand word at its own maximum -- the premise of the static proof
q60c_skip_bounds -- the model passes for the largest admissible c at or below the limit and raises WordOverflow (y' = 7q - Q negative) for the smallest
admissible c above it.  A whole transform of real data stays far from those maxima, so a transform alone could not show it."""
import numpy as np
import pytest

from gpu_util import oracle_tables
from q60c_skip_cases import M64, N, SKIP_MAX_C, WordOverflow, forward_model, prime_above_c, prime_at_or_below_c, worst_case_pair


@pytest.fixture(scope="module")
def moduli(orc):
    """the largest c at or below 2^27 + 1, a c near 2^26, the benchmark's smallest c"""
    top, mid, low = prime_at_or_below_c(orc, SKIP_MAX_C + 1), prime_at_or_below_c(orc, 1 << 26), (orc.find_prime(60, N, 0), 16383)
    assert low[0] == (1 << 60) - low[1] and top[1] <= SKIP_MAX_C and (1 << 25) < mid[1] < (1 << 26)
    return {"largest c": top[0], "c near 2^26": mid[0], "benchmark's smallest c": low[0]}


def _frames(q):
    rng = np.random.default_rng(q % 1000003)
    return {
        "all 2^64 - 1": [M64 - 1] * N,
        "all 4q - 1": [4 * q - 1] * N,
        "all q - 1": [q - 1] * N,
        "zeros": [0] * N,
        "random 64-bit words": [int(v) for v in rng.integers(0, M64, size=N, dtype=np.uint64)],
    }


@pytest.mark.parametrize("which", ["largest c", "c near 2^26", "benchmark's smallest c"])
def test_whole_transform_stays_in_64_bits_and_matches_the_oracle(orc, moduli, which):
    q = moduli[which]
    _, _, tw, pre = oracle_tables(orc, N, q)
    for kind, x in _frames(q).items():
        got = forward_model(x, q, tw)      # raises WordOverflow where a word leaves [0, 2^64)
        want = orc.forward(np.array([v % q for v in x], dtype=np.uint64), q, tw, pre, N)
        assert got == [int(v) for v in want], (which, kind)


def test_worst_case_words_pass_at_the_limit_and_trip_the_assertion_just_above_it(orc):
    q_in, c_in = prime_at_or_below_c(orc, SKIP_MAX_C + 1)
    q_out, c_out = prime_above_c(orc, SKIP_MAX_C + 1)
    assert c_in <= SKIP_MAX_C < c_out < SKIP_MAX_C + (1 << 20)
    assert worst_case_pair(q_in) == M64 - q_in - 1      # 15q + 16c - 1
    assert worst_case_pair((1 << 60) - 1) < M64      # c = 1, the other end of the class
    with pytest.raises(WordOverflow, match="y' = tx"):
        worst_case_pair(q_out)


def test_a_schedule_with_two_unreduced_stages_in_a_row_trips_the_assertion(orc, moduli):
    """the whole-transform assertions can fail too: reduce on every third stage only, and a frame of 2^64 - 1 wraps"""
    q = moduli["largest c"]
    _, _, tw, _ = oracle_tables(orc, N, q)
    with pytest.raises(WordOverflow):
        forward_model([M64 - 1] * N, q, tw, reduces=lambda s: s % 3 == 0)
