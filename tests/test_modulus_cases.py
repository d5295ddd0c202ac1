"""tests/modulus_cases.py and the references at its moduli, no device: every named modulus against a primality test written here, every mix against
its stated class, the oracle's transforms against its own naive forms, the library's host maths against the oracle's words, and the two identities of
test_rns_ref.py on every mix.  These hold before test_gpu_modulus_classes.py lets any of it judge a kernel."""
import numpy as np
import pytest

from gpu_util import rescale_reference
from modulus_cases import MIX_NAMES, MIXES, edge_bounds, edge_moduli, expected_class, prime_above, prime_below
from rns_ref import convert, lift, mod_down, product, residues, special_values, spread

SIZES = (2, 8, 64, 1024, 4096, 16384, 32768)
# the classes the issue states per mix; where a size has no 16q-lazy entry (n <= 16) the fast entries serve those plans
STATED = {"ckks40": 60, "seal": 60, "edge60": 60, "edge61": 61, "edge62": 62, "tiny": 30, "tier2": 30, "tier1": 31, "over31": 60}


def is_prime(q):
    """deterministic Miller-Rabin on Python integers: the first twelve primes as bases decide every q < 3.3 * 10^24"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    if q < 2:
        return False
    for p in bases:
        if q % p == 0:
            return q == p
    d, s = q - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        x = pow(a, d, q)
        if x in (1, q - 1):
            continue
        for _ in range(s - 1):
            x = x * x % q
            if x == q - 1:
                break
        else:
            return False
    return True


def distinct_moduli(orc, n):
    return sorted(set(edge_moduli(orc, n).values()) | {q for m in MIXES(orc, n).values() for q in m})


def test_the_primality_test_itself():
    small = [q for q in range(200) if is_prime(q)]
    assert small == [q for q in range(2, 200) if all(q % d for d in range(2, q))]
    assert is_prime((1 << 61) - 1) and is_prime(0xFFFFFFFF00000001) and not is_prime((1 << 59) - 1)
    assert not is_prime(3215031751) and not is_prime(3825123056546413051)      # strong pseudoprimes to the bases 2..7 and 2..23


@pytest.mark.parametrize("n", SIZES)
def test_named_moduli(orc, n):
    """prime, = 1 (mod 2n), on the stated side of the bound, and no admitted prime between it and the bound"""
    e, bounds = edge_moduli(orc, n), edge_bounds()
    assert set(e) == set(bounds)
    for name, q in e.items():
        side, bound = bounds[name]
        assert is_prime(q) and q % (2 * n) == 1 and 3 <= q < 1 << 62, (n, name, q)
        assert (q > bound) if side > 0 else (q < bound), (n, name, q)
        between = range(q - 2 * n, bound, -2 * n) if side > 0 else range(q + 2 * n, bound, 2 * n)
        assert abs(q - bound) < 200 * 2 * n and not any(is_prime(c) for c in between), (n, name, q)
    assert e["min"] == {2: 5, 8: 17, 64: 257, 1024: 12289, 4096: 40961, 16384: 65537, 32768: 65537}[n]
    assert 0 < (1 << 60) - e["c_max"] < 1 << 28 < (1 << 60) - e["c_out"]
    # the k-th prime is the next one behind the (k-1)-th
    for k in (1, 2):
        assert prime_above(orc, 1 << 40, n, k) == prime_above(orc, prime_above(orc, 1 << 40, n, k - 1), n)
        assert prime_below(orc, 1 << 40, n, k) == prime_below(orc, prime_below(orc, 1 << 40, n, k - 1), n)
    with pytest.raises(ValueError):
        prime_above(orc, (1 << 62) - 2, n)
    with pytest.raises(ValueError):
        prime_below(orc, 2 * n + 1, n)


@pytest.mark.parametrize("n", SIZES)
def test_mixes(orc, n):
    mixes = MIXES(orc, n)
    assert tuple(mixes) == MIX_NAMES
    for name, m in mixes.items():
        assert len(m) == 6 and len(set(m)) == 6, (n, name)
        assert all(is_prime(q) and q % (2 * n) == 1 and q < 1 << 62 for q in m), (n, name)
        want = STATED[name] if n >= 32 or STATED[name] != 60 else 61
        assert expected_class(n, m) == want, (n, name)
    e = edge_moduli(orc, n)
    c = mixes["ckks40"]
    assert [q.bit_length() for q in c] == [60, 40, 40, 40, 60, 60] and c[0] > c[4] > c[5] and c[1] > c[2] > c[3]
    assert [q.bit_length() for q in mixes["seal"]] == [43, 43, 44, 44, 50, 54]
    assert mixes["tiny"] == tuple(sorted(mixes["tiny"])) and mixes["tiny"][0] == e["min"]
    assert not any(is_prime(q) for q in range(1 + 2 * n, mixes["tiny"][5], 2 * n) if q not in mixes["tiny"])
    assert e["min"] in mixes["edge61"] and e["min"] in mixes["edge62"] and e["min"] in mixes["over31"]
    assert max(mixes["tier2"]) < 1 << 30 <= max(mixes["tier1"]) < 1 << 31 <= min(mixes["over31"][:2]) and max(mixes["over31"]) < 1 << 34
    # single moduli decide their class alone
    for name, bits in (("below30", 30), ("above30", 31), ("below31", 31), ("above60", 61), ("below61", 61), ("above61", 62), ("below62", 62)):
        assert expected_class(n, (e[name],)) == bits, (n, name)
    for name in ("above31", "below32", "above32", "below58", "above58", "below60", "c_max", "c_out", "below40"):
        assert expected_class(n, (e[name],)) == (60 if n >= 32 else 61), (n, name)


@pytest.mark.parametrize("n", SIZES)
def test_the_oracle_at_every_distinct_modulus(orc, n):
    """forward = naive_forward (n <= 1024), the inverse round trip (every n), the product against the schoolbook (n = 8 and 64)"""
    rng = np.random.default_rng(n)
    for q in distinct_moduli(orc, n):
        psi = orc.min_root(q, n)
        assert pow(psi, n, q) == q - 1, (n, q)
        tw, pre = orc.make_tables(q, psi, n)
        itw, _ = orc.make_inv_tables(q, psi, n)
        x = rng.integers(0, q, size=2 * n, dtype=np.uint64)
        x[:min(n, 3)] = np.array([0, q - 1, q - 1], dtype=np.uint64)[:min(n, 3)]
        y = orc.forward(x, q, tw, pre, n)
        assert np.array_equal(orc.inverse(y, q, itw, n), x), (n, q)
        if n <= 1024:
            assert np.array_equal(y[:n], orc.naive_forward(x[:n], q, psi, n)), (n, q)
        if n in (8, 64):
            c = orc.inverse(orc.pointwise(y[:n], y[n:], q), q, itw, n)
            assert np.array_equal(c, orc.schoolbook(x[:n], x[n:], q, n)), (n, q)


@pytest.mark.parametrize("n", SIZES)
def test_the_librarys_host_maths_equals_the_oracles(agx, orc, n):
    """agx_ntt_min_root, agx_ntt_make_tables and agx_ntt_make_inverse_tables, word for word"""
    for q in distinct_moduli(orc, n):
        psi = orc.min_root(q, n)
        assert agx.min_root(q, n) == psi, (n, q)
        for inverse, want in ((False, orc.make_tables(q, psi, n)), (True, orc.make_inv_tables(q, psi, n))):
            tw, pre = agx.make_tables(q, psi, n, inverse=inverse)
            assert np.array_equal(tw, want[0]) and np.array_equal(pre, want[1]), (n, q, inverse)


@pytest.mark.parametrize("name", MIX_NAMES)
@pytest.mark.parametrize("n", SIZES)
def test_rns_ref_on_every_mix(orc, n, name):
    """convert is residues(lift) with V = X + u D, 0 <= u < S, and ModDown from one source is the rescale in floor mode: the identities of
    test_rns_ref.py, from tiny sources under wide targets and the reverse"""
    m = MIXES(orc, n)[name]
    rng = np.random.default_rng(n + len(name))
    for src, dst in ((m[2:3], m), (m[3:5], m), (m[4:6], m[:4]), (m[:4], m[2:]), (m[1:2], m[:1] + m[2:])):
        D, special = product(src), special_values(src)
        x = np.concatenate([residues(special, src), np.stack([rng.integers(0, q, size=64, dtype=np.uint64) for q in src])], axis=1)
        V = lift(x, src)
        assert all(int(v) % D == X and int(v) // D < len(src) for v, X in zip(V[:len(special)], special))
        got = convert(x, src, dst)
        assert np.array_equal(got, np.array([[int(v) % q for v in V] for q in dst], dtype=np.uint64))
        assert np.array_equal(convert(spread(rng, x, src), src, dst), got)
        for j, q in enumerate(dst):
            if q in src:
                assert np.array_equal(got[j], x[src.index(q)])
    for moduli in (m, m[3:] + m[:3], tuple(sorted(m)), tuple(sorted(m, reverse=True))):
        x = np.stack([rng.integers(0, q, size=96, dtype=np.uint64) for q in moduli])
        x[:, :4] = np.array([[0, 1, q - 1, q // 2] for q in moduli], dtype=np.uint64)
        assert np.array_equal(mod_down(x[:-1], x[-1:], moduli[-1:], moduli[:-1]), rescale_reference(x, moduli, 0))
