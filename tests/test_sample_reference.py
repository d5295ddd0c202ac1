"""tests/sample_ref.py, the Python-integer model of agx_ntt_sample_*, judged on the CPU: the block function on the two standard ChaCha20 vectors; every uniform
word below q; a batch split at frame_first and a prime range equal the whole; n = 2 and n = 4 use cell 0 only; the rejection path is run (a third block for
q = 17 and the primes just above 2^31 and 2^60, never a second for a 2^60 - c prime); and the small kinds' statistics over 8,192 coefficients under one fixed
key, so nothing can flake: cbd(21) mean within +-0.15 and variance within 10.5 +- 1.05, each ternary frequency within 1/3 +- 0.03."""
import numpy as np
import pytest

import sample_ref as ref
from modulus_cases import edge_moduli

KEY = bytes(range(32))
KEY2 = bytes((7 * i + 3) & 0xFF for i in range(32))


def test_block_zero_key():
    o = ref.block(bytes(32), 0, 0, 0, 0)
    assert ref.keystream(o)[:32].hex() == "76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"


def test_block_rfc8439_2_3_2():
    o = ref.block(KEY, 1, 0x09000000, 0x4A000000, 0)
    assert o[:4] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3]
    assert o[-2:] == [0xE883D0CB, 0x4E3C50A2]


def test_candidates_are_pairs_of_words():
    o = ref.block(KEY, 0x0003_0050 | 2, 9, 0x11223344, 0x55667788)
    assert list(ref.candidates(KEY, 0x5566778811223344, 3, 9, 5, 2)) == [o[2 * i] | o[2 * i + 1] << 32 for i in range(8)]


@pytest.fixture(scope="module")
def moduli(orc):
    e = edge_moduli(orc, 64)
    q60c = orc.find_prime(60, 64, 0)
    assert 0 < (1 << 60) - q60c < 1 << 28
    return {"q60c": q60c, "above60": e["above60"], "above31": e["above31"], "below31": e["below31"], "tiny": edge_moduli(orc, 8)["min"]}


def test_uniform_words_are_below_q(moduli):
    qs = [moduli[k] for k in ("q60c", "above60", "above31", "below31")]
    out = ref.uniform(KEY, 5, qs, 64, 3)
    for i, q in enumerate(qs):
        assert int(out[i].max()) < q
    assert len({int(v) for v in out.reshape(-1)}) > out.size - 4      # words differ
    tiny = ref.uniform(KEY, 5, [17], 8, 40)
    assert int(tiny.max()) < 17 and set(range(17)) == {int(v) for v in tiny.reshape(-1)}


def test_a_split_batch_and_a_prime_range_equal_the_whole(moduli):
    qs = [moduli["q60c"], moduli["above31"], moduli["below31"]]
    whole = ref.uniform(KEY, 1, qs, 16, 5, frame_first=7)
    assert np.array_equal(whole[:, :2], ref.uniform(KEY, 1, qs, 16, 2, frame_first=7))
    assert np.array_equal(whole[:, 2:], ref.uniform(KEY, 1, qs, 16, 3, frame_first=9))
    assert np.array_equal(whole[1:], ref.uniform(KEY, 1, qs[1:], 16, 5, frame_first=7, prime_first=1))
    assert not np.array_equal(whole[1:], ref.uniform(KEY, 1, qs[1:], 16, 5, frame_first=7))      # the prime's index is in the words
    for kind, eta in (("ternary", None), ("cbd", 21)):
        v = ref.small_values(KEY, 2, kind, 16, 5, 7, eta)
        assert np.array_equal(v[2:], ref.small_values(KEY, 2, kind, 16, 3, 9, eta))
        s = ref.small(KEY, 2, kind, qs, 16, 5, 7, eta)
        assert np.array_equal(s[1:], ref.small(KEY, 2, kind, qs[1:], 16, 5, 7, eta))      # the small kinds do not read the prime's index
    top = (1 << 32) - 3
    assert np.array_equal(ref.uniform(KEY, 1, qs[:1], 16, 3, frame_first=top)[:, 1:], ref.uniform(KEY, 1, qs[:1], 16, 2, frame_first=top + 1))


@pytest.mark.parametrize("n", [2, 4])
def test_small_n_uses_cell_0_only(orc, n):
    q = edge_moduli(orc, n)["above31"]
    out = ref.uniform(KEY, 3, [q], n, 4, frame_first=2)
    for f in range(4):
        words, _ = ref.uniform_cell(KEY, 3, 0, 2 + f, 0, q, 8)
        assert list(out[0, f]) == words[:n]      # the first n accepted values of cell 0
    for kind, eta in (("ternary", None), ("cbd", 32)):
        v = ref.small_values(KEY, 3, kind, n, 4, 2, eta)
        assert np.array_equal(v, ref.small_values(KEY, 3, kind, 8, 4, 2, eta)[:, :n])


def test_the_rejection_path_is_run(moduli):
    for name, n, batch in (("tiny", 8, 64), ("above31", 64, 8), ("above60", 64, 8)):
        blocks = []
        ref.uniform(KEY, 11, [moduli[name]], n, batch, blocks=blocks)
        assert max(blocks) >= 3, (name, max(blocks))
    blocks = []
    ref.uniform(KEY, 11, [moduli["q60c"]], 64, 8, blocks=blocks)
    assert max(blocks) == 1


def test_a_cell_that_never_accepts_is_written_zero(monkeypatch):
    monkeypatch.setattr(ref, "candidates", lambda *a: [(1 << 64) - 1] * 8)
    words, used = ref.uniform_cell(KEY, 0, 0, 0, 0, 17, 8)
    assert words == [0] * 8 and used == 16


def test_ternary_and_cbd_words():
    ones = (1 << 64) - 1
    assert ref.ternary_value(ones) == 0 and ref.ternary_value(ones - 2) == 1 and ref.ternary_value(ones - 1) == -1
    for r in (0, 15, 31):
        low = (1 << 2 * r) - 1      # fields below r are 3
        assert ref.ternary_value(low | 1 << 2 * r) == 1 and ref.ternary_value(low | 2 << 2 * r) == -1 and ref.ternary_value(low) == 0
    alt = 0xFFFFFFFF
    for eta in (1, 21, 32):
        assert ref.cbd_value(0, eta) == 0 and ref.cbd_value(ones, eta) == 0
        assert ref.cbd_value(alt, eta) == eta and ref.cbd_value(alt << 32, eta) == -eta


def test_statistics_under_a_fixed_key(moduli):
    n, batch = 1024, 8      # 8,192 coefficients
    v = ref.small_values(KEY2, 77, "cbd", n, batch, eta=21).reshape(-1).astype(np.float64)
    print("cbd(21): mean", v.mean(), "variance", v.var())
    assert abs(v.mean()) <= 0.15 and abs(v.var() - 10.5) <= 1.05
    assert v.min() >= -21 and v.max() <= 21
    t = ref.small_values(KEY2, 77, "ternary", n, batch).reshape(-1)
    freq = [float(np.mean(t == s)) for s in (-1, 0, 1)]
    print("ternary frequencies", freq)
    assert all(abs(f - 1 / 3) <= 0.03 for f in freq) and set(np.unique(t)) == {-1, 0, 1}
    s = ref.small(KEY2, 77, "ternary", [moduli["q60c"], 17], n, 1)
    assert {int(x) for x in s[0].reshape(-1)} == {0, 1, moduli["q60c"] - 1} and {int(x) for x in s[1].reshape(-1)} == {0, 1, 16}
