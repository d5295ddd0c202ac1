"""The flag of the rare last subtract (csrc/modarith.hpp: q60c_tail_bounds, q60c_tail_flag) in Python integers, at the edges of the class q = 2^60 - c,
0 < c < 2^28: c = 1, 2^27 and 2^28 - 1, every fold count k <= 15.  The kernel subtracts q only in a wave where some output t = r + k c (r < 2^60) has
hi32(t) >= 0x0FFFFFFF.  That is sound if every t >= q is flagged, and cheap if few t < q are; both are pinned here, with the exact edge of each."""
import pytest

from q60c_rare_cases import TAIL_HI, csub_q, finish_wave, flagged, reduce_top4

CS = (1, 1 << 27, (1 << 28) - 1)
TWO60 = 1 << 60


@pytest.mark.parametrize("c", CS)
def test_every_t_at_or_above_q_is_flagged(c):
    """hi32 is monotone in t, so the least t >= q decides; per k the ends of [q, 2^60 - 1 + k c] and their neighbours are checked as the fold makes them"""
    q = TWO60 - c
    assert flagged(q) and not flagged((TAIL_HI << 32) - 1) and (TAIL_HI << 32) - 1 < q
    for k in range(16):
        t_max = TWO60 - 1 + k * c
        assert reduce_top4((k << 60) | (TWO60 - 1), c) == t_max and t_max < 2 * q and t_max < (1 << 63)
        for t in {q, q + 1, q + k * c, t_max - 1, t_max} - {q - 1}:
            if q <= t <= t_max:
                assert flagged(t), (c, k, t)
                assert csub_q(t, q) == t - q < 16 * c      # r < 2^60 = q + c: the reduced output is below (k + 1) c
    # every value the fold can produce from a word whose residue needs the subtract: v = r + k 2^60 with t = r + k c >= q
    for k in range(16):
        for r in (q - k * c, q - k * c + 1, TWO60 - 1):
            if 0 <= r < TWO60:
                t = reduce_top4((k << 60) | r, c)
                assert t == r + k * c and (t < q or flagged(t))


@pytest.mark.parametrize("c", CS)
def test_the_flag_only_over_approximates(c):
    """the largest t below q passes the flag (a false positive, which the cold block's subtract leaves alone); the flagged t below q are exactly
    [0x0FFFFFFF 2^32, q): 2^32 - c of the q residues, under 2^-28 of them"""
    q = TWO60 - c
    assert flagged(q - 1) and csub_q(q - 1, q) == q - 1
    first = TAIL_HI << 32
    assert flagged(first) and not flagged(first - 1) and first < q
    assert q - first == (1 << 32) - c and (q - first) << 28 < q
    for t in (0, 1, 15 * c - 1, 15 * c, first - 1):
        assert not flagged(t) and csub_q(t, q) == t


@pytest.mark.parametrize("c", CS)
def test_a_wave_s_results_are_those_of_a_subtract_per_coefficient(c):
    q = TWO60 - c
    first = TAIL_HI << 32
    quiet = [0, 5, 15 * c, first - 1, 12345678901234567]
    assert finish_wave(quiet, q) == quiet == [csub_q(t, q) for t in quiet]      # no flag: stored as they are, and nothing was owed
    for hot in (q, q + 15 * c - 1, TWO60 - 1 + 15 * c, q - 1, first):
        ts = quiet + [hot]
        assert finish_wave(ts, q) == [t - q if t >= q else t for t in ts]
        assert all(v < q for v in finish_wave(ts, q))
